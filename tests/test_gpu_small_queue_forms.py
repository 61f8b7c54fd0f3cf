"""Every non-persistent instance of full_bp_small.hip with its frontier queues forced short (-m gpu): SCLDPC_DEBUG_DECODER_QCAP
at small shapes, so that the scan clamp, the dropped pushes, the snapshot taken one queue-full at a time, the scan rounds behind
an overflow, the checkpoints behind a scan round and (SCLDPC_DEBUG_DECODER_KSWITCH) the private phase all run — against the host
oracle (oracle.decode_bp), bit for bit: the work is integer, there is no tolerance.  Forms, shapes, inputs, reference and the
conditions on the inputs that say which branch a case reaches: tests/small_queue_cases.py; the same conditions are asserted
without a GPU in tests/test_small_queue_cases_host.py, and here again before the device is looked at."""
import functools

import numpy as np
import pytest

import small_queue_cases as S
from conftest import require_gpu

pytestmark = pytest.mark.gpu

QCAP, KSWITCH = "SCLDPC_DEBUG_DECODER_QCAP", "SCLDPC_DEBUG_DECODER_KSWITCH"

# (size, qcap, kswitch): every form at every capacity; the fixpoint forms at the mid shape also with the waves never private and
# private as early as the carve allows, and at the shape chosen for the private phase's own overflow
SETTINGS = [(size, q, None) for size in ("tiny", "mid") for q in S.QCAPS[size]]
FIX_SETTINGS = [("mid", q, k) for q in S.QCAPS["mid"] for k in S.KSWITCHES[1:]] + [("priv", q, k) for q in S.QCAPS["priv"] for k in (None, 256)]
RUNS = [(form,) + s for form in S.FORMS for s in SETTINGS + (FIX_SETTINGS if form[1] == "fix" else [])]


def _run_id(run):
    form, size, q, k = run
    return "%s-%s-q%s%s" % (S.form_id(form), size, "full" if q is None else q, "" if k is None else "-k%d" % k)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _device(pair, size, eps):
    """The case's tables on the device: VN -> CN rows, channel words, CN -> socket table and, for (4,8), the CN -> VN table."""
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    c = S.case(pair, size, eps)
    a, ch = E.to_device(c.adj16, c.chan)
    cn = torch.from_numpy(E.cn_adj_from_vn_adj(c.p, c.adj16)).to(a.device) if pair == (4, 8) else None
    return a, ch, E.cn_sockets(c.p, a), cn


def _decode(E, form, p, dev, is_term):
    """The form through its engine wrapper: the wrapper's dict, or the counters [K, T, 8] of a caps form."""
    pi, mode, sock, wide = form
    a, ch, cs, cn = dev
    rows_cap = S.ROWS_CAP if mode == "traj" else 0
    if pi == 0:
        tab = cs if sock else cn
        if mode == "fix":
            return E.full_bp_fixpoint_cn16(p, a, tab, ch, is_term=is_term, want_erased=True, sockets=sock)
        if mode == "caps":
            return (E.full_bp_caps_wide(p, a, cs, ch, S.CAPS, is_term=is_term) if wide else
                    E.full_bp_caps_cn16(p, a, tab, ch, S.CAPS, is_term=is_term, sockets=sock))
        if wide:
            return E.full_bp_wide(p, a, cs, ch, is_term=is_term, rows_cap=rows_cap, want_erased=True)
        return E.full_bp_cn16(p, a, tab, ch, is_term=is_term, want_erased=True, sockets=sock, rows_cap=rows_cap)
    if mode == "fix":
        return E.full_bp_fixpoint_deg(p, a, cs, ch, is_term=is_term, want_erased=True)
    if mode == "caps":
        return E.full_bp_caps_deg(p, a, cs, ch, S.CAPS, is_term=is_term, wide=wide)
    return E.full_bp_deg(p, a, cs, ch, is_term=is_term, rows_cap=rows_cap, want_erased=True, wide=wide)


def _compare(E, mode, c, ref, out, what):
    if mode == "caps":                                                   # block k: decode_bp(max_it = CAPS[k])
        got = out.cpu().numpy()
        assert got.shape == ref.caps.shape
        bad = np.argwhere(got != ref.caps)
        assert bad.size == 0, (what, bad[:4].tolist(), got[got != ref.caps][:4], ref.caps[got != ref.caps][:4])
        return
    cnt = out["counters"].cpu().numpy()
    cols = S.KEEP if mode == "fix" else list(range(8))                   # fixpoint: barrier rounds are not iterations
    bad = np.argwhere(cnt[:, cols] != ref.counters[:, cols])
    assert bad.size == 0, (what, bad[:4].tolist(), cnt[bad[0, 0]], ref.counters[bad[0, 0]])
    assert (E.unpack_bits(out["erased"].cpu().numpy(), c.p.n) == ref.erased).all(), what
    if mode == "traj":
        rows = out["rows"].cpu().numpy()
        for t, want in enumerate(ref.rows):                              # deg_1_iter, recovered, first erased position
            k = len(want)
            assert (rows[t, :k] == want).all(), (what, t, np.argwhere(rows[t, :k] != want)[:3].tolist())
            assert (rows[t, k:] == 0).all(), (what, t)


@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_form_with_short_queues_equals_the_host_oracle(E, monkeypatch, run):
    import torch
    form, size, qcap, kswitch = run
    pi, mode, _sock, wide = form
    pair = S.PAIRS[pi]
    S.check_conditions(pair, size, qcap, mode, wide)                     # no case passes empty: the reference alone, first
    if qcap is not None:
        monkeypatch.setenv(QCAP, str(qcap))
    if kswitch is not None:
        monkeypatch.setenv(KSWITCH, str(kswitch))
    for eps in S.EPS_OF[size]:
        c = S.case(pair, size, eps)
        dev = _device(pair, size, eps)
        for is_term in (True, False):
            out = _decode(E, form, c.p, dev, is_term)
            torch.cuda.synchronize()
            ref = c.ref[is_term]
            _compare(E, mode, c, ref, out, (_run_id(run), eps, is_term))
            if mode == "fix" and qcap is not None and size == "tiny":
                # the knob was read: a half-queue below 64 entries keeps the waves on the shared queue, and a shared round
                # releases at most one VN per queue entry
                rounds, released = out["counters"][:, 5].cpu().numpy(), ref.counters[:, 7] - ref.counters[:, 0]
                assert (rounds.astype(np.int64) * qcap >= released).all(), (_run_id(run), eps, is_term)


@pytest.mark.parametrize("value,one_entry", [("0", True), ("-5", True), ("1", True), ("1000000000", False), (None, False)])
def test_the_knob_has_a_floor_and_only_ever_shrinks_the_queues(E, monkeypatch, value, one_entry):
    """Values below the floor act as the floor — a queue of one entry, so the fixpoint form needs a barrier round (column 5) per
    released VN — and a value above the carve's capacity leaves the launch as it is: far fewer rounds than released VNs."""
    import torch
    c, dev = S.case((4, 8), "tiny", 0.30), _device((4, 8), "tiny", 0.30)
    if value is not None:
        monkeypatch.setenv(QCAP, value)
    out = _decode(E, (0, "fix", True, False), c.p, dev, True)
    torch.cuda.synchronize()
    ref = c.ref[True]
    _compare(E, "fix", c, ref, out, value)
    rounds, released = out["counters"][:, 5].cpu().numpy(), ref.counters[:, 7] - ref.counters[:, 0]
    assert (released > 64).all()                                         # eps = 0.30 of n = 462, all recovered
    assert (rounds >= released).all() if one_entry else (rounds * 4 < released).all(), (value, rounds, released)


def test_a_queue_too_short_for_the_packed_counts_of_the_shape_is_refused(E, monkeypatch):
    """The level forms add a wave's releases (15 bits) and the CNs it zeroes (17 bits) in one reduction; the bound behind it
    needs the queue's length once a trial has more CNs than 2^17 / dv.  (5,10), L = 50, N = 1000 has 27 000: a queue of 8 is
    refused before anything is launched, the launch's own queue is not."""
    import torch
    p = E.make_params(5, 10, 50, 1000)
    a, ch = E.sample_philox(p, 3, 0, 2, 0.2, adj16=True)
    cs = E.cn_sockets(p, a)
    ok = E.full_bp_deg(p, a, cs, ch)["counters"]
    monkeypatch.setenv(QCAP, "8")
    with pytest.raises(E.ScldpcError, match=QCAP):
        E.full_bp_deg(p, a, cs, ch)
    monkeypatch.setenv(QCAP, "2048")                                     # r = 6750 + 64 * 14 = 7646, 5 r < 2^17
    short = E.full_bp_deg(p, a, cs, ch)["counters"]
    torch.cuda.synchronize()
    assert torch.equal(ok, short)
