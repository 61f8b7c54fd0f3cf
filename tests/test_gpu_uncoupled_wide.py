"""The wide rejection sampler of the uncoupled ensemble (-m gpu): scldpc_sample_philox_uncoupled_wide_device against the loop over
the CPU twin that include/scldpc_uncoupled.h fixes as the law (tests/test_gpu_uncoupled.py::twin), below and beyond the first
entry's 8192 sockets and at every size where the kernel takes another path (one, two, four and eight Philox calls per thread; one
part and four); against the first entry, output for output, where both take the shape; the cap, the sharding, the lowered part
cap, and simulate_peeling_decoder_ldpc_uncoupled(rng="philox") trial by trial against pd_oracle.random_pick_trial_philox_fast on
the twin's graphs.  Integer work: exact, no tolerance."""
import numpy as np
import pytest

from conftest import require_gpu
from test_gpu_uncoupled import twin, params, simple, e2e_reference

pytestmark = pytest.mark.gpu

SEED, TRIAL0, EPS, CAP = 91, 5, 0.45, 1 << 16
# (dv, dc, M, trials) the first entry takes too: 8190 sockets at M = 2730
SMALL = [(3, 6, 16, 64), (3, 6, 100, 32), (3, 6, 342, 16), (2, 4, 32, 32), (3, 4, 16, 32), (4, 6, 48, 8), (3, 6, 2730, 4)]
# beyond 8192 sockets: 8196 (three Philox calls per thread); 12 288, a power of two; 16 386, the first size ranked in four parts;
# 30 000; 24 000 with dv = 4; 32 760 with dc = 4; 32 766 with odd cns_pos; exactly 32 768 with dc = 2.  Last column: the twin's
# attempts where the issue of this sampler lists them (None: not pinned)
BEYOND = [(2, 4, 4098, 8, None), (3, 6, 2732, 4, None), (3, 6, 4096, 4, None), (3, 6, 5462, 2, None), (3, 6, 10000, 2, [24, 5]),
          (4, 6, 6000, 1, [1079]), (3, 4, 10920, 2, None), (3, 6, 10922, 1, [372]), (2, 4, 16384, 3, [12, 12, 1])]
SHAPES = [s + (None,) for s in SMALL] + BEYOND


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def to_numpy(out):
    d_adj, d_ch, d_att = out
    return d_adj.cpu().numpy(), d_ch.cpu().numpy().view(np.uint32), d_att.cpu().numpy()


def device_sample(E, dv, dc, M, seed, trial0, T, eps, cap):
    out = E.sample_philox_uncoupled_wide(params(dv, dc, M), seed, trial0, T, eps, cap)
    assert tuple(out[0].shape) == (T, M, dv) and tuple(out[1].shape) == (T, (M + 31) // 32) and tuple(out[2].shape) == (T,)
    return to_numpy(out)


@pytest.mark.parametrize("dv,dc,M,T,pinned", SHAPES, ids=["%d-%d-M%d" % s[:3] for s in SHAPES])
def test_rows_channel_and_attempts_equal_the_twin(E, dv, dc, M, T, pinned):
    assert E.uncoupled_wide_supported(params(dv, dc, M))
    assert E.uncoupled_supported(params(dv, dc, M)) == (dv * M <= 8192)
    rows, words, att = twin(dv, dc, M, SEED, TRIAL0, T, EPS, CAP)
    assert (att > 0).all(), "the reference accepts every listed trial within the cap"
    if pinned is not None:
        assert att.tolist() == pinned
    g_rows, g_words, g_att = device_sample(E, dv, dc, M, SEED, TRIAL0, T, EPS, CAP)
    print("attempts", g_att.tolist())
    assert (g_att == att).all(), (g_att, att)
    assert (g_rows == rows).all() and (g_words == words).all()
    cns = dv * M // dc
    for t in range(T):
        assert simple(g_rows[t])                                                  # dv distinct CNs in every row
        assert (np.bincount(g_rows[t].reshape(-1), minlength=cns) == dc).all()    # every CN exactly dc sockets


@pytest.mark.parametrize("dv,dc,M,T", SMALL, ids=["%d-%d-M%d" % s[:3] for s in SMALL])
def test_the_wide_entry_equals_the_first_entry(E, dv, dc, M, T):
    first = to_numpy(E.sample_philox_uncoupled(params(dv, dc, M), SEED, TRIAL0, T, EPS, CAP))
    wide = device_sample(E, dv, dc, M, SEED, TRIAL0, T, EPS, CAP)
    assert (first[2] > 0).all()
    for f, w in zip(first, wide):
        assert f.dtype == w.dtype and (f == w).all()


def test_the_cap_leaves_zeros_and_attempts_zero(E):
    dv, dc, M, T = 3, 6, 16, 64
    rows, words, att = twin(dv, dc, M, SEED, TRIAL0, T, EPS, CAP)
    within = att <= 100
    assert within.any() and (~within).any() and att.min() >= 1
    g_rows, g_words, g_att = device_sample(E, dv, dc, M, SEED, TRIAL0, T, EPS, 100)
    assert (g_att[within] == att[within]).all() and (g_rows[within] == rows[within]).all() and (g_words[within] == words[within]).all()
    assert (g_att[~within] == 0).all() and (g_rows[~within] == 0).all() and (g_words[~within] == 0).all()


def test_one_call_equals_two_calls(E):
    whole = device_sample(E, 3, 6, 2732, SEED, TRIAL0, 4, EPS, CAP)
    a, b = device_sample(E, 3, 6, 2732, SEED, TRIAL0, 2, EPS, CAP), device_sample(E, 3, 6, 2732, SEED, TRIAL0 + 2, 2, EPS, CAP)
    assert (whole[2] > 0).all()
    for w, x, y in zip(whole, a, b):
        assert (w == np.concatenate([x, y])).all()
    assert E.sample_philox_uncoupled_wide(params(3, 6, 2732), SEED, 5, 0, EPS, 10)[2].numel() == 0     # an empty batch


def test_a_part_beyond_its_room_ends_the_trial_with_minus_one(E, monkeypatch):
    """The kernel has no trap: a part of the keys that outgrows its room is reported per trial.  Real keys never get there (a
    quarter of at most 32 768 keys against 12 288 words), so the diagnostic cap is lowered below what every candidate has:
    600 keys against 50 where the keys are one part, a quarter of 30 000 (7500, standard deviation 75) against 7000 where
    they are four."""
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    monkeypatch.setenv("SCLDPC_DEBUG_UNCOUPLED_WIDE_PART_CAP", "50")
    g_rows, g_words, g_att = device_sample(E, 3, 6, 100, SEED, TRIAL0, 8, EPS, CAP)
    assert (g_att == -1).all() and (g_rows == 0).all() and (g_words == 0).all()
    monkeypatch.setenv("SCLDPC_DEBUG_UNCOUPLED_WIDE_PART_CAP", "7000")
    g_rows, g_words, g_att = device_sample(E, 3, 6, 10000, SEED, TRIAL0, 2, EPS, CAP)
    assert (g_att == -1).all() and (g_rows == 0).all() and (g_words == 0).all()
    with pytest.raises(RuntimeError, match="trial 0: a part of the keys outgrew its room"):
        PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 3, 6, 10000, 2, rng="philox", seed=SEED)
    monkeypatch.delenv("SCLDPC_DEBUG_UNCOUPLED_WIDE_PART_CAP")
    assert (device_sample(E, 3, 6, 100, SEED, TRIAL0, 8, EPS, CAP)[2] > 0).all()
    assert device_sample(E, 3, 6, 10000, SEED, TRIAL0, 2, EPS, CAP)[2].tolist() == [24, 5]


# ---- end to end ------------------------------------------------------------------------------------------------------------
# (l, r, M, e, trials, trials of the CPU reference that end with erased VNs left: plr > 0, wide by default).  The residual
# column pins the reference, not the device: it is what pd_oracle gives on the twin's graphs with seed 91 and trials 0 .. T - 1.
E2E = [(3, 6, 10000, 0.425, 4, 1, False), (2, 4, 16384, 0.31, 4, 1, False), (3, 6, 10922, 0.43, 2, 1, False),
       (3, 6, 24, 0.45, 16, 14, True), (3, 4, 16, 0.6, 8, 6, True)]


@pytest.mark.parametrize("l,r,M,e,T,residual,by_default", E2E, ids=["%d-%d-M%d" % c[:3] for c in E2E])
def test_the_simulator_equals_the_reference_trial_by_trial(E, monkeypatch, l, r, M, e, T, residual, by_default):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    r1s, plrs, nv = e2e_reference(l, r, M, e, T)
    assert int((plrs > 0).sum()) == residual                                 # the reference keeps a residual in these trials

    def not_the_first(*a, **k):
        raise AssertionError("the first sampler was called")
    calls, wide = [], E.sample_philox_uncoupled_wide
    monkeypatch.setattr(E, "sample_philox_uncoupled", not_the_first)
    monkeypatch.setattr(E, "sample_philox_uncoupled_wide", lambda *a, **k: (calls.append(a[3]), wide(*a, **k))[1])
    monkeypatch.setattr(PD, "UNCOUPLED_WIDE_BY_DEFAULT", by_default)
    first, r1, plr, num_vns = PD.simulate_peeling_decoder_ldpc_uncoupled(e, l, r, M, T, rng="philox", seed=SEED)
    assert calls == [T]
    assert first is None and r1.shape == (T, int(M * (e + 0.1)) + 1) and isinstance(num_vns, list)
    assert (r1 == r1s).all() and (plr == plrs).all() and num_vns == nv
    b = 5 if T > 5 else T - 1
    _, r1b, plrb, nvb = PD.simulate_peeling_decoder_ldpc_uncoupled(e, l, r, M, T, rng="philox", seed=SEED, batch=b)
    assert (r1b == r1).all() and (plrb == plr).all() and nvb == num_vns
    _, mom, plrm, nvm = PD.simulate_peeling_decoder_ldpc_uncoupled(e, l, r, M, T, rng="philox", seed=SEED, batch=b, want_moments=True)
    assert mom.dtype == np.int64 and mom.shape == (3, r1.shape[1])
    assert (mom == np.stack([(r1s != 0).sum(0), r1s.sum(0), (r1s * r1s).sum(0)])).all()
    assert (plrm == plr).all() and nvm == num_vns
