"""Cases of tests/test_gpu_small_queue_forms.py and tests/test_small_queue_cases_host.py: the form table of full_bp_small.hip's
non-persistent instances, the shapes, the host-sampled inputs with their reference (oracle.decode_bp, once per shape, eps and
chain end) and the conditions on the inputs that say which queue branches a forced capacity must reach.  Host code only: the
inputs come from the sampler's CPU twin, so every condition can be checked without a GPU.

Branches of the kernel and what reaches them (qcap = entries per frontier queue, SCLDPC_DEBUG_DECODER_QCAP):
  front  the opening scan finds more CNs with one erased neighbour than a queue holds: the fixpoint form clamps (SC_OVF), the
         level forms take their snapshot one queue-full at a time
  push   a level form's pushes of one iteration exceed the queue (LV_OVF: the next iteration is a scan round) — the oracle's
         deg_1_iter of an iteration t >= 1 exceeds qcap, and an iteration pushes at least the next one's degree-1 CNs
  caps   a checkpoint of the CAPS forms is taken right after such a scan round
The fixpoint form's append overflow and its private phase's depend on how entries are dealt to waves; builds that lose
those paths show them: profiles/full_bp_small_queue_mutations.txt lists the cases that fail under each."""
import functools
import os
import re

import numpy as np

from conftest import ROOT

KEEP = [0, 1, 2, 3, 4, 6, 7]                                             # every counter except the barrier-round count
PAIRS = ((4, 8), (3, 6), (5, 10))
MODES = ("fix", "level", "traj", "caps")
CAPS = (1, 2, 3, 5, 9, 1000000)
ROWS_CAP = 512
SEED = 2027

# ---- the forms: (pair index, mode, CN table holds sockets, wide) — kernel_of()'s keys without the persistent grid ------------
FORMS = ([(0, m, sock, False) for m in MODES for sock in (False, True)] + [(0, m, True, True) for m in MODES[1:]] +
         [(pi, m, True, False) for pi in (1, 2) for m in MODES] + [(pi, m, True, True) for pi in (1, 2) for m in MODES[1:]])


def form_id(form):
    pi, mode, sock, wide = form
    return "dv%d-%s-%s%s" % (PAIRS[pi][0], mode, "sock" if sock else "cn", "-wide" if wide else "")


def kernel_of_keys():
    """The non-persistent instances kernel_of() lists in full_bp_small.hip, as FORMS keys."""
    src = open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "full_bp_small.hip")).read()
    keys = []
    for mode, table, width, persist, pair in re.findall(
            r"case form_key\(M_(\w+), k(Cn|Sock)Table, k(Narrow|Wide), (true|false)(?:, (\d))?\):", src):
        if persist == "false":
            keys.append((int(pair or 0), mode.lower(), table == "Sock", width == "Wide"))
    return keys


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
# tiny: n = 462 is no multiple of 32 and nk is a few hundred, so a queue of 1, 8 or 32 entries overflows everywhere and a private
# half-queue (below 64 entries) is never allowed.  mid: nk between 5 and 6 thousand; with 512 entries the fixpoint form's
# half-queue is exactly 64, the smallest that lets the waves go private.  priv (fixpoint forms only): the same with a longer chain
# and eps where the decoding wave is narrow, so that a wave's private frontier outgrows its half-queue and what it drops is not
# recovered by another path: all four fixpoint instances fail here under a build whose private append no longer reports its
# overflow (profiles/full_bp_small_queue_mutations.txt, (b)).
SIZES = {"tiny": (7, 66, 24), "mid": (8, 1024, 8), "priv": (12, 1024, 8)}            # L, N, trials
EPS = (0.05, 0.30, 0.47, 0.60)                                           # floods the first frontier / … / long tails / stops at once
EPS_OF = {"tiny": EPS, "mid": EPS, "priv": (0.40, 0.45, 0.485)}
QCAPS = {"tiny": (None, 1, 8, 32), "mid": (512,), "priv": (512,)}        # None: the knob unset (the control)
KSWITCHES = (None, 0, 256)                                               # mid, fixpoint forms: default / never private / as early as allowed

# where each condition must hold (every pair, both chain ends): size, qcap -> {condition: eps values}
EXPECT = {
    ("tiny", 1): {"front": (0.05, 0.30, 0.47), "push": (0.30, 0.47), "caps": (0.30, 0.47)},
    ("tiny", 8): {"front": (0.05, 0.30, 0.47), "push": (0.30, 0.47), "caps": (0.30, 0.47)},
    ("tiny", 32): {"front": (0.05, 0.30), "push": (0.30,), "caps": (0.30,)},
    ("mid", 512): {"front": (0.05, 0.30), "push": (0.30,), "caps": (0.30,)},
    ("priv", 512): {"front": (0.40, 0.45)},
}


def params(pair, size):
    from fl_scaling_sc_ldpc_amd import engine as E
    L, N, _T = SIZES[size]
    return E.make_params(pair[0], pair[1], L, N)


def natural_qcap(p, mode, wide):
    """Entries per queue of the launch's own carve (make_args / carve / per_cu_of in full_bp_small.hip), in host arithmetic."""
    level = mode != "fix"
    nw, ncw = (p.n + 31) // 32, (p.nk + 7) // 8
    pad = lambda words: (words + 3) & ~3
    state = pad(ncw) + pad(nw) + pad(2 * p.L) + pad(18) + (pad((ncw + 3) // 4) if level else 0)
    per_cu = 1 if wide else 6 if (p.dv == 5 and mode == "traj") else 7
    while True:
        qwords = ((160 * 1024 // per_cu // 4 - 128 - state) // 2) & ~3
        if qwords > 2048 and not wide:
            qwords = 2048
        if qwords >= 128 or per_cu == 1:
            break
        per_cu -= 1
    assert qwords >= 128
    return qwords if wide else 2 * qwords


def ones0(p, adj16, chan, is_term=True):
    """Per trial, the CNs below cn_lim with exactly one erased neighbour — the first frontier — in numpy from the sampled VN -> CN
    rows [T, n, dv] (position-local) and the channel words [T, nw] alone."""
    from fl_scaling_sc_ldpc_amd import engine as E
    adj, bits = E.adj16_to_global(p, adj16), E.unpack_bits(chan, p.n)
    cn_lim = p.nk if is_term else p.L * p.cns_pos                        # BPT:944-948
    return np.array([(np.bincount(a[b != 0].ravel(), minlength=p.nk)[:cn_lim] == 1).sum() for a, b in zip(adj, bits)])


def front_overflows(p, adj16, chan, qcap, is_term=True):
    """The `front` condition: the first frontier exceeds a queue of qcap entries in at least 3/4 of the trials."""
    n1 = ones0(p, adj16, chan, is_term)
    return int((n1 > qcap).sum()) * 4 >= 3 * len(n1)


# ---- inputs and reference ---------------------------------------------------------------------------------------------------------
class Case:
    """One (pair, size, eps): T host-sampled trials and, per chain end, what decodeBP reports for them."""


@functools.lru_cache(maxsize=None)
def case(pair, size, eps):
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    p = params(pair, size)
    T = SIZES[size][2]
    po = O.Params(pair[0], pair[1], p.L, p.cns_pos, p.vns_pos)
    c = Case()
    c.p, c.T, c.eps = p, T, eps
    adj, chan = zip(*(O.sample_philox(po, SEED, (100 * EPS.index(eps) if eps in EPS else int(10000 * eps)) + t, eps) for t in range(T)))
    adj, c.chan = np.stack(adj), np.stack(chan)                          # global CN ids [T, n, dv]; channel words [T, nw]
    c.adj16 = E.global_to_adj16(p, adj)
    bits = E.unpack_bits(c.chan, p.n)
    graphs = [O.Graph.from_vn_adj(po, adj[t]) for t in range(T)]
    c.ref = {}
    for is_term in (True, False):
        r = Case()
        r.counters = np.zeros((T, 8), dtype=np.int32)
        r.erased = np.zeros((T, p.n), dtype=np.uint8)
        r.rows, r.ones0 = [], np.zeros(T, dtype=np.int64)
        r.caps = np.zeros((len(CAPS), T, 8), dtype=np.int32)
        for t in range(T):
            def report(res):
                assert res["status"] == 0
                return [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"], res["num_blocks_err_exp"], 0,
                        res["iterations"], 0, int(bits[t].sum())]
            res, erased, rows = O.decode_bp(graphs[t], bits[t], is_term=int(is_term), literal=(t == 0 and size == "tiny"),
                                             rows_cap=ROWS_CAP)
            assert res["iterations"] <= ROWS_CAP
            r.counters[t], r.erased[t] = report(res), erased
            r.rows.append(np.stack([rows["deg1"], rows["recovered"], rows["first_pos"]], axis=1))
            for k, cap in enumerate(CAPS if size != "priv" else ()):     # priv: fixpoint forms only
                r.caps[k, t] = report(O.decode_bp(graphs[t], bits[t], max_it=cap, is_term=int(is_term), literal=False)[0])
        r.ones0[:] = ones0(p, c.adj16, c.chan, is_term)
        for a in (r.counters, r.erased, r.caps, r.ones0):
            a.setflags(write=False)
        c.ref[is_term] = r
    return c


def conditions(ref, qcap):
    """Which branches a queue of qcap entries must reach on these inputs, from the reference alone."""
    T = len(ref.rows)
    front = int((ref.ones0 > qcap).sum()) * 4 >= 3 * T
    push = sum(bool((rows[1:, 0] > qcap).any()) for rows in ref.rows) * 2 >= T
    caps = any(sum(len(rows) > cap - 1 and rows[cap - 1, 0] > qcap for rows in ref.rows) * 2 >= T for cap in CAPS[1:-1])
    return {"front": front, "push": push, "caps": caps}


def check_conditions(pair, size, qcap, form_mode="level", wide=False):
    """Asserts EXPECT for one forced capacity (qcap None: the control, for which no condition may hold at the launch's own
    capacity) on every eps and both chain ends; returns what held, per (eps, is_term)."""
    held = {}
    for eps in EPS_OF[size]:
        c = case(pair, size, eps)
        for is_term in (True, False):
            q = natural_qcap(c.p, form_mode, wide) if qcap is None else qcap
            assert q <= natural_qcap(c.p, form_mode, wide)               # the knob only ever shrinks the queues
            got = conditions(c.ref[is_term], q)
            held[eps, is_term] = got
            for name, ok in got.items():
                if qcap is None:
                    assert not ok, ("control", pair, size, eps, is_term, name)
                elif eps in EXPECT[size, qcap].get(name, ()):
                    assert ok, (pair, size, qcap, eps, is_term, name, c.ref[is_term].ones0.tolist())
    return held
