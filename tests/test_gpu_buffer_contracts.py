"""Buffer contracts of the device entries (-m gpu): what the "Buffers" paragraph of include/scldpc.h promises, entry by entry.

Every case of cases() runs an engine wrapper with engine._uninit (the one allocator of outputs and workspaces) replaced by a
poison.Arena, so that the kernels get memory filled with 0xFF, with 0x5A, or with what a run on other inputs left behind,
between two guard zones:
  * every element the contract defines equals the CPU reference (oracle.decode_bp / decode_sw, pd_oracle's peel twins, the
    sampler twin, numpy), under each fill — so a skipped element, or a workspace word assumed to be zero, fails;
  * no guard byte changes, the bytes of a trial beyond the launched ones stay untouched, the inputs are bit for bit unchanged;
  * padding bits of the channel's last word change nothing and the output bitmaps' padding bits are 0;
  * a trial's result does not depend on the launch it was part of (13 trials as 13, 1 + 12 and 7 + 6);
  * a call on a side stream next to one on the default stream gives both the reference.
Columns that count a kernel's own barrier rounds or re-scans (ITERATIONS of the fixpoint forms, columns 5 and 6 of the sweep
forms) depend on how the waves interleave — two runs of one kernel differ there — so for them the tests assert only that the
kernel wrote a count, not a poison pattern.  Everything else is integer work: exact, no tolerance."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import poison
from conftest import require_gpu

pytestmark = pytest.mark.gpu

T = 5                       # trials per launch (the split test: 13)
T_SPLIT = 13                # one more than a multiple of 2, 4 and 6, no multiple of 7
ROWS_CAP = 12               # below the iteration count of the slow trials: rows beyond the cap must be dropped, not written
CAPS = (1, 3, 1000000)
PICK_STEPS_WS = 300         # num_steps of the pick forms on the workspace shapes (the CPU twin is O(steps * CNs))


# ---- shapes ----------------------------------------------------------------------------------------------------------------
class Shape:
    def __init__(self, key, dv, dc, L, N, eps, seed, term=True, doped=(), W=3, sw_it=8, sw_init=12):
        self.key, self.dv, self.dc, self.L, self.N, self.eps, self.seed = key, dv, dc, L, N, eps, seed
        self.term, self.doped, self.W = term, tuple(doped), W
        self.sw_it, self.sw_init = sw_it, sw_init                 # the window decoders: max_it, and init_it of the square window

    @property
    def p(self):
        from fl_scaling_sc_ldpc_amd import engine as E
        return E.make_params(self.dv, self.dc, self.L, self.N)

    @property
    def po(self):
        from oracle import oracle as O
        p = self.p
        return O.Params(self.dv, self.dc, self.L, p.cns_pos, p.vns_pos)

    @property
    def n(self):
        return self.L * self.N

    @property
    def ragged(self):
        return self.n % 32 != 0

    @property
    def total_size(self):
        """PD:609-611: the CNs of the terminated chain, or of its first L positions."""
        p = self.p
        return p.cns_pos * (self.L + self.dv - 1 if self.term else self.L)

    def __repr__(self):
        return self.key


def _first_L(pred, lo=2, hi=200):
    for L in range(lo, hi):
        if pred(L):
            return L
    raise AssertionError("no chain length in [%d, %d) meets the workspace rule" % (lo, hi))


def _ws_bytes(op, p, ntrials, arg0=0, arg1=0):
    from fl_scaling_sc_ldpc_amd import engine as E
    return int(E.lib().scldpc_workspace_bytes(op, C.byref(p), ntrials, arg0, arg1))


@functools.lru_cache(maxsize=None)
def shapes():
    """The small shapes (the smallest at which each layout can still go wrong) and, found by asking the library, the smallest
    (4,8) chains whose state leaves the LDS for a caller-owned workspace."""
    from fl_scaling_sc_ldpc_amd import engine as E
    s = {}
    s["a"] = Shape("48-L9-N24", 4, 8, 9, 24, 0.50, 11)                              # n = 216, ragged, cns_pos = 12
    s["b"] = Shape("36-L7-N86-nt-doped", 3, 6, 7, 86, 0.22, 19, term=False, doped=(3,), W=2)  # n = 602, ragged, CNs >= total_size
    s["c"] = Shape("510-L3-N50", 5, 10, 3, 50, 0.78, 13, W=1)                        # n = 150: chain shorter than the ring
    s["d"] = Shape("510-L6-N70", 5, 10, 6, 70, 0.53, 14, W=2)                        # n = 420, ragged
    s["e"] = Shape("48-L5-N40", 4, 8, 5, 40, 0.53, 15, W=4)                          # n = 200: the (4,8)-only forms' second shape
    mk = lambda L, N=2500: E.make_params(4, 8, L, N)
    Lf = _first_L(lambda L: _ws_bytes(E.WS_FULL_BP, mk(L), T, 1) > 0 and _ws_bytes(E.WS_FULL_BP, mk(L), T, 0) > 0)
    s["ws_full"] = Shape("48-L%d-N2500-ws" % Lf, 4, 8, Lf, 2500, 0.486, 21, W=6)
    Ls = _first_L(lambda L: _ws_bytes(E.WS_SW_BP, mk(L), T, 8) > 0, lo=16)
    s["ws_sw"] = Shape("48-L%d-N2500-ws-sw" % Ls, 4, 8, Ls, 2500, 0.48, 21, W=8, sw_it=20, sw_init=30)
    Lp = _first_L(lambda L: _ws_bytes(E.WS_PEEL_SWEEP, mk(L), T, 0) > 0 and _ws_bytes(E.WS_PEEL_SWEEP, mk(L), T, 1) > 0)
    s["ws_sweep"] = Shape("48-L%d-N2500-ws-sweep" % Lp, 4, 8, Lp, 2500, 0.49, 22)
    # the pick forms: CN words in the workspace (G) from a sixteenth of the LDS on, the degree-1 bitmap too (D1G) beyond it
    cn_bytes = lambda p: (T * p.nk * 4 + 255) & ~255
    Ng = next(N for N in range(100, 4000, 50) if all(_ws_bytes(E.WS_PEEL_PICK, mk(6, N), T, mk(6, N).nk, mt) > 0 for mt in (0, 1)))
    s["ws_pick_g"] = Shape("48-L6-N%d-ws-pick" % Ng, 4, 8, 6, Ng, 0.45, 23)
    assert _ws_bytes(E.WS_PEEL_PICK, mk(6, Ng), T, mk(6, Ng).nk, 0) == cn_bytes(mk(6, Ng))
    Ld = _first_L(lambda L: _ws_bytes(E.WS_PEEL_PICK, mk(L), T, mk(L).nk, 0) > cn_bytes(mk(L)), lo=8)
    s["ws_pick_d1g"] = Shape("48-L%d-N2500-ws-pick-d1" % Ld, 4, 8, Ld, 2500, 0.45, 24)
    Lw = _first_L(lambda L: _ws_bytes(E.WS_SAMPLE, mk(L, 2600), T) > 0, lo=4)
    s["ws_sample"] = Shape("48-L%d-N2600-ws-sample" % Lw, 4, 8, Lw, 2600, 0.45, 25)
    # the wide second-generation sampler takes 8192 < cns_pos * dc <= 20480 only: just beyond 8192 sockets per position
    s["wide_a"] = Shape("48-L3-N2050-wide-sampler", 4, 8, 3, 2050, 0.45, 31)          # n = 6150, ragged
    s["wide_b"] = Shape("36-L4-N2750-wide-sampler", 3, 6, 4, 2750, 0.45, 32)          # n = 11000, ragged
    return s


SMALL = ("a", "b", "c", "d", "e")
STREAM_SHAPES = ((4, 8, 20, 10, 0.47, 6, (5, 6)), (3, 6, 20, 10, 0.45, 7, (5, 6)))      # N = 10: ragged position words


# ---- inputs: the device's own samples, and their host copies -----------------------------------------------------------------
class Inputs:
    def __init__(self, sh, ntrials, trial0=0, alt=False):
        import torch
        from fl_scaling_sc_ldpc_amd import engine as E
        self.sh, self.T, self.trial0, p = sh, ntrials, trial0, sh.p
        seed, eps = (sh.seed + 1000, 0.9 - sh.eps) if alt else (sh.seed, sh.eps)        # alt: what a stale run decodes first
        self.a16, self.ch = E.sample_philox(p, seed, trial0, ntrials, eps, sh.doped, adj16=True)
        self.A = E.adj16_to_global(p, self.a16.cpu().numpy())                            # int32 [T, n, dv], global CN ids
        self.a32 = torch.from_numpy(self.A).to(self.a16.device)
        self.cs = E.cn_sockets(p, self.a16) if p.vns_pos * p.dv <= 65535 else None
        self.cn = None
        if (sh.dv, sh.dc) == (4, 8) and E.cn16_supported(p):
            self.cn = torch.from_numpy(E.cn_adj_from_vn_adj(p, self.a16.cpu().numpy())).to(self.a16.device)
        self.words = self.ch.cpu().numpy().view(np.uint32)
        self.bits = E.unpack_bits(self.words, p.n)                                        # uint8 [T, n]
        torch.cuda.synchronize()

    def sliced(self, lo, hi):
        """Trials lo .. hi-1 as a launch of their own (slices along dim 0 are contiguous)."""
        x = object.__new__(Inputs)
        x.sh, x.T, x.trial0 = self.sh, hi - lo, self.trial0 + lo
        for k in ("a16", "ch", "a32", "cs", "cn", "A", "words", "bits"):
            v = getattr(self, k)
            setattr(x, k, None if v is None else v[lo:hi])
        return x

    def padded(self):
        """The same trials with the padding bits of the channel's last word set (on a copy)."""
        x = self.sliced(0, self.T)
        x.ch = self.ch.clone()
        x.ch[:, -1] |= int(np.int32(np.uint32(poison.padding_mask(self.sh.n)).view(np.int32)))
        return x

    def device_tensors(self):
        return [v for v in (self.a16, self.a32, self.cs, self.cn, self.ch) if v is not None]


@functools.lru_cache(maxsize=None)
def inputs(key, ntrials=T, alt=False):
    return Inputs(shapes()[key], ntrials, alt=alt)


# ---- CPU references (cached per shape; never modified) -------------------------------------------------------------------------
def _graphs(inp):
    from oracle import oracle as O
    O.build(with_reference=False)
    if not hasattr(inp, "_graphs"):
        inp._graphs = [O.Graph.from_vn_adj(inp.sh.po, inp.A[t]) for t in range(inp.T)]
    return inp._graphs


def _memo(inp, key, make):
    if not hasattr(inp, "_memo"):
        inp._memo = {}
    if key not in inp._memo:
        inp._memo[key] = make()
    return inp._memo[key]


def bp_ref(inp, max_it, rows_cap=0):
    """decodeBP per trial: counters [T,8], erased words [T,nw], rows [T,rows_cap,3] + the mask of its defined elements."""
    def make():
        from oracle import oracle as O
        sh = inp.sh
        cnt = np.zeros((inp.T, 8), dtype=np.int32)
        er = np.zeros((inp.T, sh.n), dtype=np.uint8)
        rows = np.zeros((inp.T, max(rows_cap, 1), 3), dtype=np.int32)
        for t, g in enumerate(_graphs(inp)):
            res, erased, orows = O.decode_bp(g, inp.bits[t], max_it=max_it, is_term=int(sh.term), literal=(t == 0 and sh.n < 5000),
                                             rows_cap=rows_cap)
            cnt[t] = [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"], res["num_blocks_err_exp"], 0,
                      res["iterations"], res["status"], int(inp.bits[t].sum())]
            er[t] = erased
            for col, name in enumerate(("deg1", "recovered", "first_pos")):
                rows[t, :len(orows), col] = orows[name]
        return dict(counters=cnt, erased=poison.bitmap_expected(er), rows=rows[:, :rows_cap],
                    rows_mask=poison.rows_defined(cnt[:, 5], rows_cap))
    return _memo(inp, ("bp", max_it, rows_cap), make)


def sw_ref(inp, W, max_it, init_it, classical):
    def make():
        from oracle import oracle as O
        cnt = np.zeros((inp.T, 8), dtype=np.int32)
        er = np.zeros((inp.T, inp.sh.n), dtype=np.uint8)
        for t, g in enumerate(_graphs(inp)):
            res, erased = O.decode_sw(g, inp.bits[t], W, max_it, init_it, literal=True, square=not classical)
            cnt[t] = [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"], res["num_blocks_err_exp"],
                      res["num_erasures_p1"], res["iterations"], 0, int(inp.bits[t].sum())]
            er[t] = erased
        return dict(counters=cnt, erased=poison.bitmap_expected(er))
    return _memo(inp, ("sw", W, max_it, init_it, classical), make)


def sweep_ref(inp):
    """simulate_sc_ldpc's loop body (PD:650-691) as pd_oracle.sc_ldpc_trial_stats computes it, with the lost set kept:
    out columns 0, 1, 2, 7 and the lost bitmap."""
    def make():
        from oracle import pd_oracle as P
        sh, cpp, ts = inp.sh, inp.sh.p.cns_pos, inp.sh.total_size
        out = np.zeros((inp.T, 8), dtype=np.int32)
        lost_bits = np.zeros((inp.T, sh.n), dtype=np.uint8)
        for t in range(inp.T):
            tr, mask = inp.A[t].astype(np.int64), inp.bits[t].astype(bool)
            alive = P.peel_closure(tr, mask, ts, 0)
            lost = alive & ((tr >= 0) & (tr < ts)).any(axis=1) & (tr < ts).all(axis=1)               # PD:659-666
            sizes, comp, idx = P.components(tr, lost)
            big = sizes[comp] > 2 if len(idx) else np.zeros(0, dtype=bool)
            out[t, 0], out[t, 1] = int(lost.sum()), int(sizes[sizes > 2].sum())
            out[t, 2] = len(np.unique((tr[idx, 0] // cpp)[big]))
            out[t, 7] = int(mask.sum())
            lost_bits[t] = lost
            if sh.term:                                                                          # the twin itself, where it applies
                s = P.sc_ldpc_trial_stats(tr, mask, sh.dv, sh.dc, sh.L, sh.N, True, True, list(sh.doped))
                assert (out[t, 0], out[t, 1], out[t, 2]) == (s["num_lost"], s["num_lost_exp"], s["blocks_failed_exp"])
        return dict(out=out, lost=poison.bitmap_expected(lost_bits))
    return _memo(inp, "sweep", make)


def pick_steps(sh):
    npos = sh.L + sh.dv - 1 if sh.term else sh.L
    return PICK_STEPS_WS if sh.key.endswith(("-ws-pick", "-ws-pick-d1")) else int(sh.N * npos * (sh.eps + 0.1))


def pick_ref(inp, mt):
    """simulate_peeling_decoder_ldpc's loop body (PD:750-785): r1, out, moments of the batch, and (mt) the advanced
    MT19937 states.  Philox: PhiloxPickStream(seed, trial0 + t); mt: CPython's random.Random(1000 + trial0 + t)."""
    def make():
        from oracle import pd_oracle as P
        sh = inp.sh
        steps = pick_steps(sh)
        npos = sh.L + sh.dv - 1 if sh.term else sh.L
        e = (steps + 0.5) / (sh.N * npos) - 0.1                          # random_pick_trial derives its step count from e
        assert int(sh.N * npos * (e + 0.1)) == steps
        r1 = np.zeros((inp.T, steps + 1), dtype=np.int64)
        out = np.zeros((inp.T, 4), dtype=np.int32)
        state0 = np.zeros((inp.T, 625), dtype=np.uint32)
        state1 = np.zeros((inp.T, 625), dtype=np.uint32)
        for t in range(inp.T):
            rng = random.Random(1000 + inp.trial0 + t) if mt else P.PhiloxPickStream(sh.seed, inp.trial0 + t)
            if mt:
                state0[t] = rng.getstate()[1]
            r1[t], plr = P.random_pick_trial(inp.A[t].astype(np.int64), inp.bits[t].astype(bool), sh.dv, sh.dc, sh.L, sh.N, e,
                                             sh.term, rng)
            if mt:
                state1[t] = rng.getstate()[1]
            picks = int(np.count_nonzero(r1[t, :-1] > 0))
            gen = sh.L * sh.N
            assert plr == (gen - (gen - int(inp.bits[t].sum()) + picks)) / gen           # PD:753, 771, 785
            out[t] = [int(inp.bits[t].sum()), picks, r1[t, -1], picks]
        mom = np.stack([(r1 != 0).sum(0), r1.sum(0), (r1 ** 2).sum(0)]).astype(np.int64)
        return dict(r1=r1.astype(np.int32), out=out, moments=mom, state0=state0, state1=state1)
    return _memo(inp, ("pick", mt), make)


def sock_ref(inp):
    """numpy: the CN -> socket table as a sorted set per CN (0xFFFF pads), from the 2-byte rows."""
    def make():
        p = inp.sh.p
        a = inp.a16.cpu().numpy().view(np.uint16).astype(np.int64)
        out = np.full((inp.T, p.nk, p.dc), 0xFFFF, dtype=np.uint16)
        j = np.arange(p.n)
        for t in range(inp.T):
            fill = np.zeros(p.nk, dtype=np.int64)
            for i in range(p.dv):
                cn = (j // p.vns_pos + i) * p.cns_pos + a[t, :, i]
                sock = p.dv * (j % p.vns_pos) + i
                order = np.argsort(cn, kind="stable")
                cn_s, so_s = cn[order], sock[order]
                first = np.searchsorted(cn_s, cn_s, side="left")
                slot = fill[cn_s] + (np.arange(p.n) - first)
                out[t, cn_s, slot] = so_s
                fill += np.bincount(cn, minlength=p.nk)
        return np.sort(out, axis=2)
    return _memo(inp, "sock", make)


def sampler_ref(sh, ntrials, trial0):
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    adj = np.stack([O.sample_philox(sh.po, sh.seed, trial0 + t, sh.eps, sh.doped)[0] for t in range(ntrials)])
    ch = np.stack([O.sample_philox(sh.po, sh.seed, trial0 + t, sh.eps, sh.doped)[1] for t in range(ntrials)])
    return adj.astype(np.int32), E.global_to_adj16(sh.p, adj), ch.view(np.uint32)


# ---- the case table ------------------------------------------------------------------------------------------------------------
# A case: name, the header symbols it covers, the shapes it is to run on, supported(E, shape) (the entry's own *_supported),
# run(E, inp, x) -> {output name: tensor} (x: the harness, for caller-passed buffers) and expect(inp) -> {output name: (want,
# mask or None)}.  "count" marks columns that hold a kernel's own round count.
class Case:
    def __init__(self, name, symbols, shape_keys, run, expect, supported=None, counts=None, env=None, split=True):
        self.name, self.symbols, self.shape_keys, self.run, self.expect = name, tuple(symbols), tuple(shape_keys), run, expect
        self.supported = supported or (lambda E, sh: True)
        self.counts = counts or {}                       # output name -> columns that are a kernel's own count
        self.env, self.split = env or {}, split


def _bp_expect(max_it, rows_cap=0, erased=True):
    def expect(inp):
        r = bp_ref(inp, max_it, rows_cap)
        e = {"counters": (r["counters"], None)}
        if erased:
            e["erased"] = (r["erased"], None)
        if rows_cap:
            e["rows"] = (r["rows"], r["rows_mask"])
        return e
    return expect


def _fix_expect(inp):
    r = bp_ref(inp, 0)
    c = r["counters"].copy()
    c[:, 6] = 0                                          # STATUS of a fixpoint form is always 0
    return {"counters": (c, None), "erased": (r["erased"], None)}


def _caps_expect(inp):
    return {"counters": (np.stack([bp_ref(inp, k)["counters"] for k in CAPS]), None)}


def _tables(inp, form):
    """The tables a 4-bit form reads: (a16, CN -> VN table) or (a16, CN -> socket table)."""
    return (inp.a16, inp.cn) if form == "cn16" else (inp.a16, inp.cs)


def _level_cases():
    cases = []
    first_ws = ("ws_full",)
    for adj in ("a32", "a16"):
        sym = "scldpc_full_bp_device" + ("_adj16" if adj == "a16" else "")
        for max_it in (0, 3):
            for rows_cap in (0, ROWS_CAP):
                cases.append(Case("full_bp-%s-it%d-rows%d" % (adj, max_it, rows_cap), [sym], SMALL + first_ws,
                                  lambda E, inp, x, adj=adj, max_it=max_it, rows_cap=rows_cap:
                                  (E.full_bp(inp.sh.p, getattr(inp, adj), inp.ch, max_it=max_it, is_term=inp.sh.term,
                                                   rows_cap=rows_cap, want_erased=True, counters=x.counters(inp))),
                                  _bp_expect(max_it, rows_cap)))
        cases.append(Case("full_bp_fixpoint-%s" % adj, ["scldpc_full_bp_fixpoint_device" + ("_adj16" if adj == "a16" else "")],
                          SMALL + first_ws,
                          lambda E, inp, x, adj=adj: E.full_bp_fixpoint(inp.sh.p, getattr(inp, adj), inp.ch, is_term=inp.sh.term,
                                                                        want_erased=True, counters=x.counters(inp)),
                          _fix_expect, counts={"counters": [5]}))
    sup48 = {"cn16": lambda E, sh: (sh.dv, sh.dc) == (4, 8) and E.cn16_supported(sh.p),
             "sock16": lambda E, sh: (sh.dv, sh.dc) == (4, 8) and E.full_bp_sock16_supported(sh.p)}
    for form in ("cn16", "sock16"):
        sk = form == "sock16"
        cases.append(Case("full_bp_fixpoint_" + form, ["scldpc_full_bp_fixpoint_device_" + form], SMALL,
                          lambda E, inp, x, form=form, sk=sk: E.full_bp_fixpoint_cn16(inp.sh.p, *_tables(inp, form), inp.ch,
                                                                                       is_term=inp.sh.term, want_erased=True,
                                                                                       counters=x.counters(inp), sockets=sk),
                          _fix_expect, sup48[form], counts={"counters": [5]}))
        for max_it in (0, 3):
            cases.append(Case("full_bp_%s-it%d" % (form, max_it), ["scldpc_full_bp_device_" + form], SMALL,
                              lambda E, inp, x, form=form, sk=sk, max_it=max_it:
                              E.full_bp_cn16(inp.sh.p, *_tables(inp, form), inp.ch, max_it=max_it, is_term=inp.sh.term,
                                             want_erased=True, counters=x.counters(inp), sockets=sk),
                              _bp_expect(max_it), sup48[form]))
            cases.append(Case("full_bp_traj_%s-it%d" % (form, max_it), ["scldpc_full_bp_traj_device_" + form], SMALL,
                              lambda E, inp, x, form=form, sk=sk, max_it=max_it:
                              (E.full_bp_cn16(inp.sh.p, *_tables(inp, form), inp.ch, max_it=max_it, is_term=inp.sh.term,
                                                    want_erased=True, counters=x.counters(inp), sockets=sk, rows_cap=ROWS_CAP)),
                              _bp_expect(max_it, ROWS_CAP), sup48[form]))
        cases.append(Case("full_bp_caps_" + form, ["scldpc_full_bp_caps_device_" + form], SMALL,
                          lambda E, inp, x, form=form, sk=sk: {"counters": E.full_bp_caps_cn16(
                              inp.sh.p, *_tables(inp, form), inp.ch, CAPS, is_term=inp.sh.term, sockets=sk)},
                          _caps_expect, sup48[form]))
    supw = lambda E, sh: (sh.dv, sh.dc) == (4, 8) and E.full_bp_wide_supported(sh.p)
    for max_it in (0, 3):
        for rows_cap in (0, ROWS_CAP):
            sym = "scldpc_full_bp_traj_device_wide" if rows_cap else "scldpc_full_bp_device_wide"
            cases.append(Case("full_bp_wide-it%d-rows%d" % (max_it, rows_cap), [sym], SMALL,
                              lambda E, inp, x, max_it=max_it, rows_cap=rows_cap:
                              (E.full_bp_wide(inp.sh.p, inp.a16, inp.cs, inp.ch, max_it=max_it, is_term=inp.sh.term,
                                                    rows_cap=rows_cap, want_erased=True, counters=x.counters(inp))),
                              _bp_expect(max_it, rows_cap), supw))
    cases.append(Case("full_bp_caps_wide", ["scldpc_full_bp_caps_device_wide"], SMALL,
                      lambda E, inp, x: {"counters": E.full_bp_caps_wide(inp.sh.p, inp.a16, inp.cs, inp.ch, CAPS, is_term=inp.sh.term)},
                      _caps_expect, supw))
    for wide in (False, True):
        sfx = "_wide" if wide else ""
        supd = lambda E, sh, wide=wide: E.full_bp_deg_supported(sh.p, wide=wide)
        for max_it in (0, 3):
            for rows_cap in (0, ROWS_CAP):
                sym = "scldpc_full_bp_%sdevice_deg%s" % ("traj_" if rows_cap else "", sfx)
                cases.append(Case("full_bp_deg%s-it%d-rows%d" % (sfx, max_it, rows_cap), [sym], SMALL,
                                  lambda E, inp, x, wide=wide, max_it=max_it, rows_cap=rows_cap:
                                  (E.full_bp_deg(inp.sh.p, inp.a16, inp.cs, inp.ch, max_it=max_it, is_term=inp.sh.term,
                                                       rows_cap=rows_cap, want_erased=True, counters=x.counters(inp), wide=wide)),
                                  _bp_expect(max_it, rows_cap), supd))
        cases.append(Case("full_bp_caps_deg" + sfx, ["scldpc_full_bp_caps_device_deg" + sfx], SMALL,
                          lambda E, inp, x, wide=wide: {"counters": E.full_bp_caps_deg(inp.sh.p, inp.a16, inp.cs, inp.ch, CAPS,
                                                                                         is_term=inp.sh.term, wide=wide)},
                          _caps_expect, supd))
    cases.append(Case("full_bp_fixpoint_deg", ["scldpc_full_bp_fixpoint_device_deg"], SMALL,
                      lambda E, inp, x: E.full_bp_fixpoint_deg(inp.sh.p, inp.a16, inp.cs, inp.ch, is_term=inp.sh.term,
                                                               want_erased=True, counters=x.counters(inp)),
                      _fix_expect, lambda E, sh: E.full_bp_deg_supported(sh.p), counts={"counters": [5]}))
    return cases


SW_MIXED = {"e": (False, True), "ws_sw": (False, True), "b": (False,)}   # shape -> the windows (classical?) whose trials both
# decode and fail there: asserted by mixed_outcomes.  Window decoding of the other small shapes fails (a, c, d) or decodes
# (b, classical) every trial at the eps that mixes their full-BP outcomes.


def _sw_expect(classical):
    def expect(inp):
        r = sw_ref(inp, inp.sh.W, inp.sh.sw_it, 0 if classical else inp.sh.sw_init, classical)
        return {"counters": (r["counters"], None), "erased": (r["erased"], None)}
    return expect


def _sw_cases():
    cases = []
    for adj in ("a32", "a16"):
        a = "_adj16" if adj == "a16" else ""
        cases.append(Case("sw_bp-" + adj, ["scldpc_sw_bp_device" + a], SMALL + ("ws_sw",),
                          lambda E, inp, x, adj=adj: E.sw_bp(inp.sh.p, getattr(inp, adj), inp.ch, inp.sh.W, inp.sh.sw_it, inp.sh.sw_init,
                                                             want_erased=True, counters=x.counters(inp), ring=False),
                          _sw_expect(False)))
        cases.append(Case("swc_bp-" + adj, ["scldpc_swc_bp_device" + a], SMALL + ("ws_sw",),
                          lambda E, inp, x, adj=adj: E.sw_bp(inp.sh.p, getattr(inp, adj), inp.ch, inp.sh.W, inp.sh.sw_it, want_erased=True,
                                                             counters=x.counters(inp), classical=True),
                          _sw_expect(True)))
    cases.append(Case("sw_bp_ring", ["scldpc_sw_bp_ring_device"], SMALL,
                      lambda E, inp, x: E.sw_bp(inp.sh.p, inp.a16, inp.ch, inp.sh.W, inp.sh.sw_it, inp.sh.sw_init, want_erased=True,
                                                counters=x.counters(inp), ring=True, d_cn_sock=inp.cs),
                      _sw_expect(False), lambda E, sh: E.sw_ring_supported(sh.p, sh.W)))
    cases.append(Case("sw_bp_ring_deg", ["scldpc_sw_bp_ring_device_deg"], SMALL,
                      lambda E, inp, x: E.sw_bp(inp.sh.p, inp.a16, inp.ch, inp.sh.W, inp.sh.sw_it, inp.sh.sw_init, want_erased=True,
                                                counters=x.counters(inp), ring=True, d_cn_sock=inp.cs, deg=True),
                      _sw_expect(False), lambda E, sh: E.sw_ring_deg_supported(sh.p, sh.W)))
    cases.append(Case("swc_bp_ring", ["scldpc_swc_bp_ring_device"], SMALL,
                      lambda E, inp, x: E.sw_bp(inp.sh.p, inp.a16, inp.ch, inp.sh.W, inp.sh.sw_it, want_erased=True,
                                                counters=x.counters(inp), classical=True, ring=True, d_cn_sock=inp.cs),
                      _sw_expect(True), lambda E, sh: E.swc_ring_supported(sh.p, sh.W)))
    cases.append(Case("cn_sockets", ["scldpc_cn_sockets_device"], SMALL + ("ws_full",),
                      lambda E, inp, x: {"sockets": E.cn_sockets(inp.sh.p, inp.a16)},
                      lambda inp: {"sockets": (sock_ref(inp), None)}))
    return cases


def _sweep_expect(inp):
    r = sweep_ref(inp)
    return {"out": (r["out"], None), "lost": (r["lost"], None)}


def _sweep_args(inp):
    ts = inp.sh.total_size
    return dict(total_size=ts, sweep_start=0, lost_lo=0, lost_hi=ts, want_lost=True)


def _peel_cases():
    cases = []
    for adj in ("a32", "a16"):
        a = "_adj16" if adj == "a16" else ""
        cases.append(Case("peel_sweep-" + adj, ["scldpc_peel_sweep_device" + a], SMALL + ("ws_sweep",),
                          lambda E, inp, x, adj=adj: E.peel_sweep(inp.sh.p, getattr(inp, adj), inp.ch, **_sweep_args(inp)),
                          _sweep_expect, counts={"out": [5]}))
    cases.append(Case("peel_sweep_sock16", ["scldpc_peel_sweep_device_sock16"], SMALL,
                      lambda E, inp, x: E.peel_sweep_sock16(inp.sh.p, inp.a16, inp.cs, inp.ch, **_sweep_args(inp)),
                      _sweep_expect, lambda E, sh: E.peel_sweep_sock16_supported(sh.p), counts={"out": [5, 6]}))
    cases.append(Case("peel_sweep_sock16_wide", ["scldpc_peel_sweep_device_sock16_wide"], SMALL,
                      lambda E, inp, x: E.peel_sweep_sock16_wide(inp.sh.p, inp.a16, inp.cs, inp.ch, **_sweep_args(inp)),
                      _sweep_expect, lambda E, sh: E.peel_sweep_wide_supported(sh.p), counts={"out": [5, 6]}))

    def pick(E, inp, x, adj, mt=False, moments=False, want_r1=True):
        import torch
        kw = {}
        if mt:
            kw["mt_state"] = x.filled(torch.from_numpy(pick_ref(inp, True)["state0"].view(np.int32)))
        if moments:
            kw["moments"] = x.filled(torch.full((3, pick_steps(inp.sh) + 1), 7, dtype=torch.int64))
        r = E.peel_pick(inp.sh.p, getattr(inp, adj), inp.ch, inp.sh.total_size, pick_steps(inp.sh), seed=inp.sh.seed,
                        trial0=inp.trial0, want_r1=want_r1, **kw)
        return {"out": r["out"], "r1": r["r1"], "moments": r["moments"], "mt_state": kw.get("mt_state")}

    def pick_expect(mt=False, moments=False, want_r1=True):
        def expect(inp):
            r = pick_ref(inp, mt)
            e = {"out": (r["out"], None)}
            if want_r1:
                e["r1"] = (r["r1"], poison.r1_defined(inp.T, pick_steps(inp.sh)))
            if moments:
                e["moments"] = (r["moments"] + 7, None)                   # accumulated in place onto what the caller put there
            if mt:
                e["mt_state"] = (r["state1"].view(np.int32), None)
            return e
        return expect
    pick_shapes = SMALL + ("ws_pick_g", "ws_pick_d1g")
    for adj in ("a32", "a16"):
        sym = ["scldpc_peel_pick_device" + ("_adj16" if adj == "a16" else "")]
        for name, kw in (("philox", {}), ("mt", dict(mt=True)), ("moments", dict(moments=True)),
                         ("moments-no-r1", dict(moments=True, want_r1=False)), ("mt-no-r1", dict(mt=True, want_r1=False))):
            cases.append(Case("peel_pick-%s-%s" % (adj, name), sym, pick_shapes,
                              lambda E, inp, x, adj=adj, kw=kw: pick(E, inp, x, adj, **kw), pick_expect(**kw),
                              split=not kw.get("moments")))        # moments are a sum over the launch, not a per-trial row
    for name, env in (("", {}), ("-tpw4", {"SCLDPC_DEBUG_PICK_TPW": "4"}), ("-noprebuild", {"SCLDPC_DEBUG_PICK_PREBUILD": "0"})):
        # the same environment switches reach peel_pick_multi_kernel behind scldpc_peel_pick_device_adj16 on the D1G shape
        cases.append(Case("peel_pick_deg" + name, ["scldpc_peel_pick_device_adj16_deg"], SMALL + ("ws_pick_d1g",),
                          lambda E, inp, x: E.peel_pick_deg(inp.sh.p, inp.a16, inp.ch, inp.sh.total_size, pick_steps(inp.sh),
                                                            seed=inp.sh.seed, trial0=inp.trial0),
                          pick_expect(), lambda E, sh: E.peel_pick_deg_supported(sh.p, sh.total_size), env=env))
        if env:
            cases.append(Case("peel_pick-a16-philox" + name, ["scldpc_peel_pick_device_adj16"], ("ws_pick_d1g",),
                              lambda E, inp, x: pick(E, inp, x, "a16"), pick_expect(), env=env))
    return cases


def _sampler_cases():
    def expect(tables=None):
        def f(inp):
            adj, a16, ch = sampler_ref(inp.sh, inp.T, inp.trial0)
            e = {"adj": (adj if tables == "a32" else a16.view(np.int16), None), "chan": (ch.view(np.int32), None)}
            if tables == "sock":
                e["table"] = (sock_ref(inp), None)
            if tables == "cn":
                from fl_scaling_sc_ldpc_amd import engine as E
                e["table"] = (np.sort(E.cn_adj_from_vn_adj(inp.sh.p, a16).view(np.uint16), axis=2), None)
            return e
        return f

    def two(E, inp, x, adj16):
        sh = inp.sh
        out = x.sampler_out(inp, [(sh.p.n, sh.p.dv, "int16" if adj16 else "int32"), (sh.p.nw, "int32")])
        a, ch = E.sample_philox(sh.p, sh.seed, inp.trial0, inp.T, sh.eps, sh.doped, out=out, adj16=adj16)
        return {"adj": a[:inp.T], "chan": ch[:inp.T]}

    def three(fn, table):
        def run(E, inp, x):
            sh = inp.sh
            out = x.sampler_out(inp, [(sh.p.n, sh.p.dv, "int16"), (sh.p.nk, sh.p.dc, "int16"), (sh.p.nw, "int32")])
            a, cn, ch = getattr(E, fn)(sh.p, sh.seed, inp.trial0, inp.T, sh.eps, sh.doped, out=out)
            return {"adj": a[:inp.T], "table": cn[:inp.T], "chan": ch[:inp.T]}
        return run

    def ens_case(ens):
        def run(E, inp, x):
            sh = inp.sh
            out = x.sampler_out(inp, [(sh.p.n, sh.p.dv, "int32"), (sh.p.nw, "int32")])
            a, ch = E.sample_philox(sh.p, sh.seed, inp.trial0, inp.T, sh.eps, sh.doped, out=out, ensemble=ens)
            return {"adj": a[:inp.T], "chan": ch[:inp.T]}

        def exp(inp):
            from oracle import oracle as O
            sh = inp.sh
            tw = [O.sample_philox(sh.po, sh.seed, inp.trial0 + t, sh.eps, sh.doped, ensemble=ens) for t in range(inp.T)]
            return {"adj": (np.stack([a for a, _ in tw]).astype(np.int32), None),
                    "chan": (np.stack([c for _, c in tw]).view(np.int32), None)}
        # no *_supported of its own: the entry refuses a tail-biting chain shorter than dv with a message that names the rule
        return Case("sample_philox-" + ens, ["scldpc_sample_philox_ensemble_device"], SMALL, run, exp,
                    lambda E, sh: ens != "tail_biting" or sh.L >= sh.dv)
    cases = [Case("sample_philox-a32", ["scldpc_sample_philox_device"], SMALL + ("ws_sample",),
                  lambda E, inp, x: two(E, inp, x, False), expect("a32")),
             Case("sample_philox-a16", ["scldpc_sample_philox_device_adj16"], SMALL + ("ws_sample",),
                  lambda E, inp, x: two(E, inp, x, True), expect()),
             Case("sample_philox_sock", ["scldpc_sample_philox_device_adj16_sock"], SMALL + ("ws_sample",), three("sample_philox_sock", "sock"),
                  expect("sock"), lambda E, sh: E.sample_philox_sock_supported(sh.p)),
             Case("sample_philox_cn16", ["scldpc_sample_philox_device_cn16"], SMALL, three("sample_philox_cn16", "cn"), expect("cn"),
                  lambda E, sh: (sh.dv, sh.dc) == (4, 8) and E.cn16_supported(sh.p)),
             Case("sample_philox_sock16", ["scldpc_sample_philox_device_sock16"], SMALL, three("sample_philox_sock16", "sock"),
                  expect("sock"), lambda E, sh: (sh.dv, sh.dc) == (4, 8) and E.sock16_supported(sh.p)),
             Case("sample_philox_deg_sock16", ["scldpc_sample_philox_device_deg_sock16"], SMALL, three("sample_philox_deg_sock16", "sock"),
                  expect("sock"), lambda E, sh: E.deg_sock16_supported(sh.p)),
             Case("sample_philox_wide_sock16", ["scldpc_sample_philox_device_wide_sock16"], ("wide_a", "wide_b"),
                  three("sample_philox_wide_sock16", "sock"), expect("sock"), lambda E, sh: E.wide_sock16_supported(sh.p)),
             ens_case("tail_biting"), ens_case("protograph")]
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_level_cases() + _sw_cases() + _peel_cases() + _sampler_cases())


# Entries of the header with a d_ output pointer that the table above does not run through the poison harness, each with the
# reason.  Only two kinds are allowed: host-only functions, and entries whose buffers the caller initialises by contract —
# those run in test_caller_initialised_entries below (exact values, red zones), without poison of the in/out buffer itself.
EXCLUDED = {
    "scldpc_stream_run_device": "d_state, d_counters: the caller zero-fills them and they carry over; d_trace runs below",
    "scldpc_stream_run_device_inputs": "d_state, d_counters: the caller zero-fills them and they carry over; d_trace runs below",
    "scldpc_stream_run_device_inputs_at": "d_state, d_counters: the caller zero-fills them and they carry over; d_trace runs below",
    "scldpc_accumulate_run_device": "d_run is accumulated in place: the caller initialises it",
    "scldpc_accumulate_peel_device": "d_run is accumulated in place: the caller initialises it",
    "scldpc_r1_moments_device": "d_moments is accumulated in place: the caller initialises it",
    "scldpc_clear_channel_range_device": "d_chan_bits is edited in place: the caller's channel",
}


def covered_symbols():
    return {s for c in cases() for s in c.symbols}


def runs_of(E):
    """(case, shape key) pairs that run: a pair is left out only where the entry's own *_supported answers 0."""
    return [(c, k) for c in cases() for k in c.shape_keys if c.supported(E, shapes()[k])]


def check_table(E):
    """Every case runs on at least two shapes, one of them ragged (so that a refusal cannot empty a row) — except the cases
    that exist for one workspace form only."""
    for c in cases():
        ks = [k for k in c.shape_keys if c.supported(E, shapes()[k])]
        if c.shape_keys == ("ws_pick_d1g",):
            assert ks == ["ws_pick_d1g"]
            continue
        assert len(ks) >= 2 and any(shapes()[k].ragged for k in ks), (c.name, ks)
    for c in cases():
        for k in c.shape_keys:
            if k.startswith("ws_"):
                assert c.supported(E, shapes()[k]), (c.name, k)         # a workspace shape is never silently dropped


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def _synchronize():
    """torch.cuda.synchronize(); a device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the buffer-contract tests, stopping: %s" % e, returncode=3)


class Harness:
    """One call of a case under one arena: hands out the caller-passed buffers (one trial longer than the launch)."""

    def __init__(self, arena, monkeypatch, E, poison_rows=True):
        self.arena, self.extra = arena, []
        if arena is None:                                                # the real allocator: torch.empty, as engine._uninit
            self.arena = None
            self.alloc = lambda shape, dtype, device: __import__("torch").empty(shape, dtype=dtype, device=device)
            return
        self.alloc = arena
        monkeypatch.setattr(E, "_uninit", arena)
        if poison_rows:
            monkeypatch.setattr(E, "_zeroed", arena)                     # the kernels' own rows: no zeros underneath

    def counters(self, inp):
        import torch
        buf = self.alloc((inp.T + 1, 8), dtype=torch.int32, device=inp.ch.device)
        self.extra.append((buf, inp.T, buf[inp.T:].clone()))
        return buf

    def sampler_out(self, inp, specs):
        import torch
        out = []
        for spec in specs:
            buf = self.alloc((inp.T + 1,) + tuple(spec[:-1]), dtype=getattr(torch, spec[-1]), device="cuda:0")
            self.extra.append((buf, inp.T, buf[inp.T:].clone()))
            out.append(buf)
        return tuple(out)

    def filled(self, host):
        """A caller-initialised in/out buffer (MT19937 states, moments) inside the guard zones."""
        buf = self.alloc(tuple(host.shape), dtype=host.dtype, device="cuda:0")
        buf.copy_(host)
        return buf

    def check(self, what):
        _synchronize()
        if self.arena is not None:
            self.arena.check_guards()
        import torch
        for buf, ntrials, before in self.extra:                           # the trial beyond the launch: untouched, under every fill
            assert torch.equal(buf[ntrials:], before), (what, "bytes of trial T were written", buf.shape)
            if self.arena is not None and self.arena.mode != "stale":
                assert (before.cpu().numpy().view(np.uint8) == self.arena.mode).all()


def _compare(case, what, got, want):
    for name, (w, mask) in want.items():
        g = got[name].cpu().numpy()
        if name in ("sockets", "table"):
            g = np.sort(g.view(np.uint16), axis=2)                          # a set per CN
        if name in ("erased", "lost"):
            g = g.view(np.uint32)
        cols = case.counts.get(name)
        if cols:
            keep = np.ones(w.shape[-1], dtype=bool)
            keep[cols] = False
            count = g[..., cols].astype(np.int64)
            assert ((count >= 0) & (count < 1 << 24)).all(), (what, name, "a round count was not written", count)
            g, w = g[..., keep], w[..., keep]
        poison.assert_defined_equal("%s %s" % (what, name), g, w, mask)
    for name, t in got.items():
        assert t is None or name in want, (what, name, "an output without an expectation")


def _run_case(E, monkeypatch, case, inp, mode, prime=None, poison_rows=True):
    import torch
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    arena = poison.Arena(mode)
    if mode == "stale":
        x = Harness(arena, monkeypatch, E, poison_rows)
        primed = case.run(E, prime, x)                                    # another seed and eps first
        x.check((case.name, "priming run"))
        for name, cols in case.counts.items():                            # a stale round count would pass for a written one
            primed[name][..., cols] = -1
        arena.recycle()
    x = Harness(arena, monkeypatch, E, poison_rows)
    got = case.run(E, inp, x)
    got = {k: v for k, v in (got.items() if isinstance(got, dict) else got) if v is not None}
    x.check((case.name, inp.sh.key, mode))
    out = {}
    for k, v in got.items():
        rows = inp.T if not (k == "counters" and v.dim() == 3) and k != "moments" else v.shape[0]
        out[k] = v[:rows].clone()
    return out


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    from oracle import oracle as O
    O.build(with_reference=False)
    return engine


def _ids():
    from fl_scaling_sc_ldpc_amd import engine
    return [(c, k) for c, k in runs_of(engine)]


def pytest_generate_tests(metafunc):
    if "case_shape" in metafunc.fixturenames:
        pairs = _ids()
        if metafunc.function.__name__ == "test_a_trial_does_not_depend_on_its_launch":
            seen, keep = set(), []
            for c, k in pairs:                                            # the first small shape each case runs on
                if c.split and c.name not in seen and k in SMALL:
                    seen.add(c.name)
                    keep.append((c, k))
            pairs = keep
        if metafunc.function.__name__ == "test_padding_bits_of_the_channel_are_ignored":
            pairs = [(c, k) for c, k in pairs if shapes()[k].ragged and k in SMALL and not c.name.startswith("sample_")]
        metafunc.parametrize("case_shape", pairs, ids=["%s@%s" % (c.name, shapes()[k].key) for c, k in pairs])


def test_the_table_runs_every_case_on_two_shapes_one_of_them_ragged(E):
    check_table(E)


def mixed_outcomes(inp, key):
    """Of the trials at least one decodes and at least one fails, on the reference of each family that runs on the shape: full
    BP to its fixpoint (small shapes, ws_full), the sweep peeling (small shapes, ws_sweep), the square and the classical
    window (SW_MIXED), the random-pick peeling (small shapes: a trial peeled to the end and one that stalls).  Also: the
    trajectory cap binds for some trial and not for another."""
    def mixed(failed):
        assert (failed == 0).any() and (failed > 0).any(), (key, failed)
    if key in SMALL + ("ws_full",):
        c = bp_ref(inp, 0)["counters"]
        mixed(c[:, 0])
        if key == "a":
            assert (c[:, 5] > ROWS_CAP).any() and (c[:, 5] <= ROWS_CAP).any(), (key, c[:, 5])
    if key in SMALL + ("ws_sweep",):
        mixed(sweep_ref(inp)["out"][:, 0])
    for classical in SW_MIXED.get(key, ()):
        mixed(sw_ref(inp, inp.sh.W, inp.sh.sw_it, 0 if classical else inp.sh.sw_init, classical)["counters"][:, 0])
    if key in PICK_MIXED:
        out = pick_ref(inp, False)["out"]
        mixed(out[:, 0] - out[:, 1])                                      # erased VNs the picks did not recover
    if key in ("ws_pick_g", "ws_pick_d1g"):
        # 300 steps of some 1500 (68 000) erased VNs: no trial can finish, so no mix is possible here; what these shapes add is
        # the other exit of the step loop — every trial stops at the step limit with degree-1 CNs left
        out = pick_ref(inp, False)["out"]
        assert (out[:, 1] == PICK_STEPS_WS).all() and (out[:, 2] > 0).all(), (key, out)


PICK_MIXED = ("a", "b", "d", "e")      # (c: 150 VNs at eps = 0.78 — every trial stalls)


@pytest.mark.parametrize("key", SMALL + ("ws_full", "ws_sw", "ws_sweep", "ws_pick_g", "ws_pick_d1g"))
def test_every_shape_has_a_trial_that_decodes_and_one_that_fails(E, key):
    """On the CPU references of the device's own samples (checked on the sampler's CPU twin when the seeds were chosen)."""
    mixed_outcomes(inputs(key), key)


def test_the_pick_cases_leave_the_step_loop_both_ways(E):
    """Across the table: trials that run out of degree-1 CNs before the last step (r1 ends at 0, the small shapes) and trials
    the step limit stops (the workspace shapes)."""
    small = np.concatenate([pick_ref(inputs(k), False)["out"] for k in SMALL])
    assert (small[:, 2] == 0).all() and (small[:, 1] < np.array([pick_steps(shapes()[k]) for k in SMALL]).repeat(T)).all()
    ws = np.concatenate([pick_ref(inputs(k), False)["out"] for k in ("ws_pick_g", "ws_pick_d1g")])
    assert (ws[:, 1] == PICK_STEPS_WS).all() and (ws[:, 2] > 0).all()


def test_poisoned_outputs_red_zones_and_read_only_inputs(E, monkeypatch, case_shape):
    import torch
    case, key = case_shape
    inp, prime = inputs(key), inputs(key, T, True)
    want = case.expect(inp)
    before = [t.clone() for t in inp.device_tensors()]
    got = {}
    for mode in poison.MODES:
        got[mode] = _run_case(E, monkeypatch, case, inp, mode, prime)
        _compare(case, (case.name, key, mode), got[mode], want)
    for a, b in zip(before, inp.device_tensors()):
        assert torch.equal(a, b), (case.name, key, "an input was written")
    # the wrapper's own promise: rows beyond the iteration count are zeros
    if "rows" in want:
        monkeypatch.undo()
        out = _run_case(E, monkeypatch, case, inp, 0xFF, poison_rows=False)
        w, mask = want["rows"]
        poison.assert_defined_equal("%s %s rows" % (case.name, key), out["rows"].cpu().numpy(), w * mask)


def test_padding_bits_of_the_channel_are_ignored(E, monkeypatch, case_shape):
    """n % 32 != 0, the padding bits of the channel's last word set: every defined output unchanged, the padding bits of the
    erased / lost bitmaps 0 (the expected words carry zeros there)."""
    case, key = case_shape
    inp = inputs(key)
    _compare(case, (case.name, key, "padding"), _run_case(E, monkeypatch, case, inp.padded(), 0xFF), case.expect(inp))


def test_a_trial_does_not_depend_on_its_launch(E, monkeypatch, case_shape):
    """13 trials as one launch, as 1 + 12 and as 7 + 6 (trial0 offsets on the Philox forms): identical rows, and the
    reference's."""
    import torch
    case, key = case_shape
    whole = inputs(key, T_SPLIT)
    one = _run_case(E, monkeypatch, case, whole, 0xFF)
    _compare(case, (case.name, key, "13"), one, case.expect(whole))
    for cut in (1, 7):
        parts = [_run_case(E, monkeypatch, case, whole.sliced(lo, hi), 0x5A) for lo, hi in ((0, cut), (cut, T_SPLIT))]
        for name, t in one.items():
            dim = 1 if name == "counters" and t.dim() == 3 else 0
            joined = torch.cat([q[name] for q in parts], dim=dim).cpu().numpy()
            ref = t.cpu().numpy()
            mask = None
            cols = case.counts.get(name)
            if cols:
                mask = np.ones(ref.shape, dtype=bool)
                mask[..., cols] = False
            if name == "rows":
                mask = poison.rows_defined(one["counters"][:, 5].cpu().numpy(), ROWS_CAP)
            if name in ("sockets", "table"):
                joined, ref = np.sort(joined.view(np.uint16), axis=2), np.sort(ref.view(np.uint16), axis=2)
            poison.assert_defined_equal("%s %s split at %d: %s" % (case.name, key, cut, name), joined, ref, mask)


SIDE = ("full_bp-a16-it0-rows0@ws_full", "sw_bp-a16@ws_sw", "peel_sweep-a16@ws_sweep", "peel_pick-a16-philox@ws_pick_g",
        "peel_pick_deg@a", "sample_philox-a16@ws_sample")


@pytest.mark.parametrize("which", SIDE)
def test_a_call_on_a_side_stream_next_to_one_on_the_default_stream(E, monkeypatch, which):
    """engine._workspace's note: a fresh buffer per call, so two calls in flight on two streams share no scratch."""
    import torch
    name, key = which.split("@")
    case = next(c for c in cases() if c.name == name)
    inp = inputs(key)
    want = case.expect(inp)
    arena = poison.Arena(0xFF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    x1, x2 = Harness(arena, monkeypatch, E), Harness(arena, monkeypatch, E)
    with torch.cuda.stream(side):
        a = case.run(E, inp, x1)
    b = case.run(E, inp, x2)                                              # queued at once: no synchronise in between
    _synchronize()
    x1.check((which, "side stream")), x2.check((which, "default stream"))
    for got in (a, b):
        got = {k: v[:inp.T] if k != "moments" else v for k, v in got.items() if v is not None}
        _compare(case, (which, "two streams"), got, want)
    # the same pair with the real engine._uninit, twice with the streams swapped: the caching allocator hands a freed block back
    # to the stream that used it only, so the second round's calls get the first round's blocks without sharing scratch
    monkeypatch.undo()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    del a, b, got
    for rnd in range(2):
        x1, x2 = Harness(None, monkeypatch, E), Harness(None, monkeypatch, E)
        with torch.cuda.stream(side):
            a = case.run(E, inp, x1 if rnd == 0 else x2)
        b = case.run(E, inp, x2 if rnd == 0 else x1)
        _synchronize()
        x1.check((which, "real allocator", rnd)), x2.check((which, "real allocator", rnd))
        for got in (a, b):
            got = {k: v[:inp.T] if k != "moments" else v for k, v in got.items() if v is not None}
            _compare(case, (which, "two streams, real allocator", rnd), got, want)
        del a, b, got


# ---- entries whose buffers the caller initialises: exact values and red zones ------------------------------------------------
def test_caller_initialised_entries(E, monkeypatch):
    import torch
    arena = poison.Arena(0x5A)
    x = Harness(arena, monkeypatch, E)
    rng = np.random.RandomState(3)
    # accumulate_run: plr_computation over all trials (stop rule off), onto a non-zero run
    cnt = rng.randint(0, 4, size=(37, 8)).astype(np.int32)
    run0 = np.arange(100, 100 + E.NRUN, dtype=np.int64)
    run = E.accumulate_run(x.filled(torch.from_numpy(cnt)), x.filled(torch.from_numpy(run0)), 0)
    ne, ee = cnt[:, 0].astype(np.int64), cnt[:, 2].astype(np.int64)
    add = [ne.sum(), (ne > 0).sum(), (cnt[:, 4] > 0).sum(), cnt[ne > 0, 1].sum(), ee.sum(), (ee > 0).sum(), cnt[ee > 0, 3].sum(),
           len(cnt), cnt[:, 5].sum()]
    # accumulate_peel: PD:668-699 over all trials
    out = rng.randint(0, 3, size=(41, 8)).astype(np.int32)
    prun0 = np.arange(7, 7 + E.NPEELRUN, dtype=np.int64)
    prun = E.accumulate_peel(x.filled(torch.from_numpy(out)), x.filled(torch.from_numpy(prun0)), 0)
    padd = np.zeros(E.NPEELRUN, dtype=np.int64)
    padd[:6] = [len(out), (out[:, 0] >= 1).sum(), out[:, 0].sum(), (out[:, 1] > 0).sum(), out[:, 1].sum(), out[:, 2].sum()]
    # r1_moments onto a non-zero table
    r1 = rng.randint(0, 300, size=(13, 77)).astype(np.int32)
    r1[:, 60:] = 0
    mom = E.r1_moments(x.filled(torch.from_numpy(r1)), x.filled(torch.full((3, 77), 5, dtype=torch.int64)))
    r64 = r1.astype(np.int64)
    # clear_channel_range at word boundaries, ragged n
    p = shapes()["a"].p
    cleared = []
    for lo, hi in ((0, 1), (31, 33), (5, 160), (200, 216)):
        ch = E.clear_channel_range(p, x.filled(torch.full((3, p.nw), -1, dtype=torch.int32)), lo, hi)
        cleared.append((lo, hi, ch))
    x.check("caller-initialised entries")
    assert run.cpu().numpy().tolist() == (run0 + np.array(add, dtype=np.int64)).tolist()
    assert prun.cpu().numpy().tolist() == (prun0 + padd).tolist()
    assert (mom.cpu().numpy() == 5 + np.stack([(r64 != 0).sum(0), r64.sum(0), (r64 ** 2).sum(0)])).all()
    for lo, hi, ch in cleared:
        exp = np.ones((3, p.nw * 32), dtype=np.uint8)
        exp[:, lo:hi] = 0
        assert (ch.cpu().numpy().view(np.uint32) == poison.bitmap_expected(exp)).all(), (lo, hi)


@pytest.mark.parametrize("mode", poison.MODES)
@pytest.mark.parametrize("dv,dc,L,N,eps,W,doped", STREAM_SHAPES)
def test_stream_traces_under_poison(E, monkeypatch, mode, dv, dc, L, N, eps, W, doped):
    """Streams.run / InputStreams.run / GlibcStreamRun.run with trace=True: every element of d_trace and the counters equal
    the CPU twins (the Philox twin with the node-level decoder; the glibc stream with the literal one), whatever the trace
    buffer held, with guard zones around the trace.  (d_state and d_counters are the caller's: zero-filled once, carried on.)"""
    import torch
    from oracle import oracle as O
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    assert E.stream_supported(p, W)
    arena = poison.Arena(mode)
    monkeypatch.setattr(E, "_uninit", arena)
    ns, chunks = 3, (23, 17)
    for rnd in range(2 if mode == "stale" else 1):                        # stale: the second round reads the first one's traces
        st = E.Streams(p, ns, seed=17 + rnd, eps=eps, W=W, doped=doped, stream0=5)
        ins = [E.stream_glibc_inputs(p, 40 + rnd + s, eps, doped, L // 2 + sum(chunks)) for s in range(2)]
        sti = E.InputStreams(p, np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins]), W, doped)
        gl = E.GlibcStreamRun(p, 60 + rnd, W, doped)
        gl.new_point(eps)
        tw = [O.Stream(po, 17 + rnd, eps, W, doped, rng_mode=1, decoder=1, sid=5 + s) for s in range(ns)]
        twi = [O.Stream(po, 40 + rnd + s, eps, W, doped, rng_mode=0, decoder=0) for s in range(2)]
        twg = O.Stream(po, 60 + rnd, eps, W, doped, rng_mode=0, decoder=0)
        for npos in chunks:
            cnt, tr = st.run(npos, trace=True)
            cnti, tri = sti.run(npos, trace=True)
            rows = gl.run(npos)
            _synchronize()
            arena.check_guards()
            for twins, trace, c in ((tw, tr, cnt), (twi, tri, cnti)):
                for s, twin in enumerate(twins):
                    want = np.array([[o[f] for f in O.Stream.FIELDS] for o in (twin.step() for _ in range(npos))])
                    poison.assert_defined_equal("trace of stream %d" % s, trace[s].cpu().numpy(), want)
                    assert c[s, :8].cpu().numpy().tolist() == want[-1, 2:].tolist()
            want = np.array([[o[f] for f in O.Stream.FIELDS] for o in (twg.step() for _ in range(npos))])
            poison.assert_defined_equal("trace of the glibc run", rows, want)
        arena.recycle()
