"""Random-pick peeling for the pairs (3,6), (4,8), (5,10) through engine.peel_pick_deg (-m gpu): cn_build.hip's ring of dv CN
positions and peel_pick_multi_kernel<TPW, DV> against engine.peel_pick (one trial per wave, its own build) and against the CPU
twin oracle.pd_oracle.random_pick_trial on the device's own inputs.  Equality is exact everywhere.

The shapes are the smallest that reach each way the kernels can go wrong: chains shorter than the ring (L < dv), cns_pos = 25 (the
channel words straddle positions), CNs at or beyond total_size (non-terminated chains), a doped position, odd sizes, and two with
more than 8192 pickable CNs (three rank-select blocks, 19 sub-blocks, about 7 000 picks).  T = 5 trials: the last wave holds
fewer trials than it has room for, with two and with four trials per wave.  Inputs and references are computed once per shape."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

T = 5
#         l, r,  L,  M,   e,    terminated, doped
SHAPES = [(3, 6, 1, 50, 0.30, True, ()),
          (3, 6, 2, 50, 0.40, True, ()),
          (5, 10, 3, 50, 0.45, False, ()),
          (5, 10, 6, 70, 0.47, True, ()),
          (3, 6, 7, 86, 0.42, False, (3,)),
          (3, 6, 30, 600, 0.41, True, ()),
          (5, 10, 28, 600, 0.47, False, ())]
IDS = ["%d-%d-L%d-M%d-%s%s" % (s[0], s[1], s[2], s[3], "T" if s[5] else "N", "-doped" if s[6] else "") for s in SHAPES]
SEED = 17


@pytest.fixture(scope="module")
def PD():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import peeling_decoding
    return peeling_decoding


_cache = {}


def case(PD, shape):
    """Inputs of T trials of `shape` on the device, and what engine.peel_pick makes of them (computed once, never changed)."""
    if shape in _cache:
        return _cache[shape]
    E = PD.E
    l, r, L, M, e, term, doped = shape
    cpp = int(l / r * M)
    npos = L + l - 1 if term else L
    c = dict(p=E.CodeParams(l, r, L, cpp, M), total_size=cpp * npos, steps=int(M * npos * (e + 0.1)), generated=(L - len(doped)) * M)
    c["adj"], c["ch"] = E.sample_philox(c["p"], SEED, 0, T, e, list(doped), adj16=True)
    first = E.peel_pick(c["p"], c["adj"], c["ch"], c["total_size"], c["steps"], seed=SEED, trial0=0)
    c["first"] = dict(r1=first["r1"].cpu().numpy(), out=first["out"].cpu().numpy())
    c["first"]["plrs"] = plrs_of(c["first"]["out"], c["generated"])
    _cache[shape] = c
    return c


def plrs_of(out, generated):
    return (out[:, 0] - out[:, 1]) / generated                              # as simulate_peeling_decoder_ldpc (PD:753,785)


def multi(PD, c, want_r1=True):
    res = PD.E.peel_pick_deg(c["p"], c["adj"], c["ch"], c["total_size"], c["steps"], seed=SEED, trial0=0, want_r1=want_r1)
    out = res["out"].cpu().numpy()
    return dict(r1=res["r1"].cpu().numpy() if want_r1 else None, out=out, plrs=plrs_of(out, c["generated"]))


def same(a, b):
    return all(a[k].shape == b[k].shape and (a[k] == b[k]).all() for k in ("r1", "out", "plrs"))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_peel_pick_deg_equals_peel_pick(PD, shape):
    c = case(PD, shape)
    assert PD.E.peel_pick_deg_supported(c["p"], c["total_size"])
    got = multi(PD, c)
    assert got["r1"].shape == (T, c["steps"] + 1) and got["out"].shape == (T, 4)
    assert same(got, c["first"])
    if shape[2] >= 28:                                                   # the large shapes do reach three rank-select blocks
        assert c["total_size"] > 8192 and got["out"][:, 1].max() > 5000


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_peel_pick_deg_equals_the_cpu_twin(PD, oracle, shape):
    from oracle import pd_oracle as P
    E = PD.E
    c = case(PD, shape)
    l, r, L, M, e, term, doped = shape
    got = multi(PD, c)
    A = E.adj16_to_global(c["p"], c["adj"].cpu().numpy()).astype(np.int64)
    bits = E.unpack_bits(c["ch"].cpu().numpy(), c["p"].n).astype(bool)
    for t in range(T):
        ref_r1, ref_plr = P.random_pick_trial(A[t], bits[t], l, r, L, M, e, term, P.PhiloxPickStream(SEED, t), len(doped))
        assert ref_r1.shape == got["r1"][t].shape and (got["r1"][t] == ref_r1).all() and got["plrs"][t] == ref_plr, (shape, t)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_four_trials_per_wave_and_the_kernels_own_build_give_the_same_arrays(PD, monkeypatch, shape):
    c = case(PD, shape)
    for env in (dict(SCLDPC_DEBUG_PICK_TPW="4"), dict(SCLDPC_DEBUG_PICK_PREBUILD="0"),
                dict(SCLDPC_DEBUG_PICK_TPW="4", SCLDPC_DEBUG_PICK_PREBUILD="0")):
        for k in ("SCLDPC_DEBUG_PICK_TPW", "SCLDPC_DEBUG_PICK_PREBUILD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert same(multi(PD, c), c["first"]), env


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_without_the_rows_out_is_unchanged(PD, shape):
    c = case(PD, shape)
    got = multi(PD, c, want_r1=False)
    assert got["r1"] is None and (got["out"] == c["first"]["out"]).all()


@pytest.mark.parametrize("L,M,e,term", [(9, 60, 0.46, False), (44, 4000, 0.04, True)])
def test_a_4_8_shape_through_the_new_entry_equals_the_existing_entry(PD, L, M, e, term):
    """(4,8): the DV = 4 instances.  The second shape is beyond the LDS budget, where the existing entry takes the same kernels."""
    c = case(PD, (4, 8, L, M, e, term, ()))
    assert same(multi(PD, c), c["first"])
    assert c["first"]["out"][:, 1].min() > 0


def test_simulate_peeling_decoder_ldpc_multi_equals_first(PD, capfd):
    args = (0.42, 3, 6, 7, 86, False, False, 7, [3])
    kw = dict(rng="philox", seed=4, batch=3)                              # a batch that does not divide num_repeats
    _, r1_f, plr_f = PD.simulate_peeling_decoder_ldpc(*args, pick="first", **kw)
    capfd.readouterr()
    _, r1_m, plr_m = PD.simulate_peeling_decoder_ldpc(*args, pick="multi", **kw)
    err = capfd.readouterr().err
    assert err.count("[scldpc] kernels: ") == 1 and "cn_build ring + peel_pick_multi" in err
    assert r1_m.shape == r1_f.shape and (r1_m == r1_f).all() and (plr_m == plr_f).all() and r1_f[:, 0].min() > 0
    _, mom_f, plr_f2 = PD.simulate_peeling_decoder_ldpc(*args, pick="first", want_moments=True, **kw)
    _, mom_m, plr_m2 = PD.simulate_peeling_decoder_ldpc(*args, pick="multi", want_moments=True, **kw)
    assert mom_m.shape == mom_f.shape and (mom_m == mom_f).all() and (plr_m2 == plr_f).all() and (plr_f2 == plr_f).all()
    assert (mom_f[1] == r1_f.sum(0)).all() and (mom_f[0] == (r1_f != 0).sum(0)).all()
    # the default asks for nothing new and takes the first path
    capfd.readouterr()
    _, r1_a, plr_a = PD.simulate_peeling_decoder_ldpc(*args, **kw)
    assert (r1_a == r1_f).all() and (plr_a == plr_f).all() and "[scldpc] kernels" not in capfd.readouterr().err


def test_pick_multi_on_a_refused_shape_raises(PD):
    with pytest.raises(ValueError, match="^pick='multi': the multi-trial pick kernel takes the pairs"):
        PD.simulate_peeling_decoder_ldpc(0.45, 5, 10, 50, 10000, True, False, 2, [], rng="philox", pick="multi")
    with pytest.raises(PD.E.ScldpcError, match="4220 words"):
        p = PD.E.make_params(5, 10, 50, 10000)
        import torch
        PD.E.peel_pick_deg(p, torch.zeros((1, p.n, p.dv), dtype=torch.int16, device="cuda"),
                           torch.zeros((1, p.nw), dtype=torch.int32, device="cuda"), 270000, 10)
