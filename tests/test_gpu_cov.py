"""engine.r1_gram (scldpc_r1_gram_device, csrc/r1_gram.hip) against numpy's int64 matmul, and simulate_pd_covariance against the
rows simulate_peeling_decoder_ldpc returns (-m gpu).  Integer work: exact equality, no tolerance.

The kernel's output tile is 64 x 64 and its trial chunk 32: the sizes below sit one below, at and one above both, cover more than
one tile and more than one chunk, one workgroup per tile and trials split over several."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

NCOLS = 307                                                             # a multiple of nothing


@pytest.fixture(scope="module")
def PD():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import peeling_decoding
    return peeling_decoding


def np_gram(r1, steps):
    x = np.asarray(r1)[:, np.asarray(steps)].astype(np.int64)
    m = (x != 0).astype(np.int64)
    return np.stack([m.T @ m, x.T @ m, x.T @ x])


def rows(T, ncols=NCOLS, seed=0, hi=3000):
    """int32 [T, ncols] in [1, hi) with a third of the entries zero."""
    rng = np.random.default_rng(1000 * T + ncols + seed)
    r = rng.integers(1, hi, size=(T, ncols), dtype=np.int64)
    r[rng.random((T, ncols)) < 1 / 3] = 0
    return r.astype(np.int32)


def steps_of(K, ncols=NCOLS, seed=0):
    """K strictly increasing, non-contiguous steps that include column 0 and the last column (K = 1: the last column)."""
    if K == 1:
        return np.array([ncols - 1])
    rng = np.random.default_rng(K + seed)
    inner = rng.choice(np.arange(1, ncols - 1), size=K - 2, replace=False)
    return np.sort(np.concatenate([[0, ncols - 1], inner])).astype(np.int64)


def device_gram(PD, r1, steps, gram=None):
    import torch
    g = PD.E.r1_gram(torch.from_numpy(r1).cuda(), steps, gram)
    return g


# every T of {1, 5, 63, 64, 65, 257, 1000} and K of {1, 2, 63, 64, 65, 129, 300}; T = 31, 32, 33 around the chunk of 32 trials
SIZES = [(1, 1), (5, 2), (63, 63), (64, 64), (65, 65), (257, 129), (1000, 300), (31, 300), (32, 1), (33, 129), (1000, 2), (5, 64),
         (64, 63), (257, 65)]


@pytest.mark.parametrize("T,K", SIZES, ids=["T%d-K%d" % s for s in SIZES])
def test_gram_equals_numpy_int64(PD, T, K):
    r1, steps = rows(T), steps_of(K)
    assert len(steps) == K and (np.diff(steps) > 0).all() and (K == 1 or (steps[0] == 0 and steps[-1] == NCOLS - 1))
    if K > 2:
        assert (np.diff(steps) > 1).any()
    assert abs((r1 == 0).mean() - 1 / 3) < 0.2
    got = device_gram(PD, r1, steps)
    want = np_gram(r1, steps)
    assert got.dtype.is_signed and tuple(got.shape) == (3, K, K)
    assert (got.cpu().numpy() == want).all()
    # the diagonal is r1_moments at the steps
    import torch
    mom = PD.E.r1_moments(torch.from_numpy(r1).cuda()).cpu().numpy()
    for k in range(3):
        assert (np.diag(want[k]) == mom[k][steps]).all()


def test_steps_as_list_tensor_and_int32(PD):
    import torch
    r1, steps = rows(40), steps_of(7)
    want = np_gram(r1, steps)
    for s in (steps.tolist(), torch.from_numpy(steps), torch.from_numpy(steps.astype(np.int32)).cuda(), steps.astype(np.int16)):
        assert (device_gram(PD, r1, s).cpu().numpy() == want).all()


def test_a_second_call_accumulates_in_place(PD):
    a, b, steps = rows(65, seed=1), rows(130, seed=2), steps_of(70)
    g = device_gram(PD, a, steps)
    g2 = device_gram(PD, b, steps, g)
    assert g2 is g
    assert (g.cpu().numpy() == np_gram(a, steps) + np_gram(b, steps)).all()
    assert (g.cpu().numpy() == np_gram(np.concatenate([a, b]), steps)).all()


def test_trials_split_over_several_workgroups(PD):
    T, K = 5000, 65
    assert PD.E.r1_gram_trial_splits(T, K) == 157 > 1                  # 4 tiles: each chunk of 32 trials its own workgroup
    r1, steps = rows(T), steps_of(K)
    assert (device_gram(PD, r1, steps).cpu().numpy() == np_gram(r1, steps)).all()
    # and several chunks per workgroup: 1024 / 25 tiles -> 41 shares of the 313 chunks, 8 chunks each
    T, K = 10000, 300
    assert PD.E.r1_gram_trial_splits(T, K) == 40
    r1, steps = rows(T), steps_of(K)
    assert (device_gram(PD, r1, steps).cpu().numpy() == np_gram(r1, steps)).all()


def test_wide_values_need_64_bit_products(PD):
    rng = np.random.default_rng(3)
    r1 = rng.integers((1 << 30) - 1000, (1 << 30) + 1, size=(4, 11)).astype(np.int32)
    r1[1, 3] = 0
    steps = [0, 2, 3, 7, 10]
    want = np_gram(r1, steps)
    assert want[2].max() > 1 << 61 and want[1].max() > 1 << 31
    assert (device_gram(PD, r1, steps).cpu().numpy() == want).all()


def test_the_limit_of_4096_steps(PD):
    T, K, ncols = 8, 4096, 4101
    r1, steps = rows(T, ncols), steps_of(K, ncols)
    got = device_gram(PD, r1, steps).cpu().numpy()
    assert (got == np_gram(r1, steps)).all()
    with pytest.raises(PD.E.ScldpcError, match="1 <= k <= 4096"):
        device_gram(PD, r1, np.arange(4097))


def test_a_non_default_stream(PD):
    import torch
    r1, steps = rows(257), steps_of(129)
    d = torch.from_numpy(r1).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = PD.E.r1_gram(d, steps)
        g = PD.E.r1_gram(d, steps, g)
    s.synchronize()
    assert (g.cpu().numpy() == 2 * np_gram(r1, steps)).all()


def test_a_step_out_of_range_is_clamped_and_reported(PD):
    """The kernel never reads outside d_r1: the row buffer is a view inside a larger one, and the sums are those of the
    clamped columns."""
    import torch
    r1 = rows(33)
    big = torch.zeros((35, NCOLS), dtype=torch.int32, device="cuda")
    big[1:34] = torch.from_numpy(r1).cuda()
    gram = torch.zeros((3, 4, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(PD.E.ScldpcError, match="clamped"):
        PD.E.r1_gram(big[1:34], [-5, 3, NCOLS, NCOLS + 100000], gram)
    assert (gram.cpu().numpy() == np_gram(r1, [0, 3, NCOLS - 1, NCOLS - 1])).all()
    # the next call starts from a clean status
    assert (PD.E.r1_gram(big[1:34], [0, 3]).cpu().numpy() == np_gram(r1, [0, 3])).all()


def test_an_empty_batch_touches_nothing(PD):
    import torch
    gram = torch.full((3, 2, 2), 7, dtype=torch.int64, device="cuda")
    g = PD.E.r1_gram(torch.zeros((0, 9), dtype=torch.int32, device="cuda"), [1, 4], gram)
    assert (g.cpu().numpy() == 7).all()


# ---- the simulator ---------------------------------------------------------------------------------------------------------
ARGS = (0.45, 4, 8, 10, 40, False, False, 48)                            # num_pd_steps = 220; stride 7: K = 32
SEED, STRIDE = 5, 7
_ref = {}


def reference(PD, args=ARGS):
    """The rows, moments and plrs of simulate_peeling_decoder_ldpc(rng="philox", seed=5), computed once."""
    if args not in _ref:
        _, r1, plrs = PD.simulate_peeling_decoder_ldpc(*args, [], rng="philox", seed=SEED)
        _, mom, plrs_m = PD.simulate_peeling_decoder_ldpc(*args, [], rng="philox", seed=SEED, want_moments=True)
        _ref[args] = dict(r1=r1, plrs=plrs, mom=mom, plrs_m=plrs_m)
    return _ref[args]


def check_against_rows(ref, out):
    steps, gram, mom, plrs = out
    want_steps = np.arange(0, ref["r1"].shape[1], STRIDE)
    assert steps.dtype == np.int64 and (steps == want_steps).all() and len(steps) == 32
    assert gram.dtype == np.int64 and gram.shape == (3, 32, 32) and (gram == np_gram(ref["r1"], steps)).all()
    assert mom.dtype == np.int64 and mom.shape == ref["mom"].shape and (mom == ref["mom"]).all()
    assert plrs.dtype == np.float64 and (plrs == ref["plrs_m"]).all() and (plrs == ref["plrs"]).all()
    for k in range(3):
        assert (np.diag(gram[k]) == mom[k][steps]).all()
    assert (gram[0] == gram[0].T).all() and (gram[2] == gram[2].T).all() and (gram[1] != gram[1].T).any()
    assert gram[0].max() > 0 and gram[2].max() > 0


def test_simulate_pd_covariance_equals_the_gram_of_the_rows(PD):
    ref = reference(PD)
    assert ref["r1"].shape == (48, 221)
    out = PD.simulate_pd_covariance(*ARGS, STRIDE, seed=SEED)
    check_against_rows(ref, out)
    cov, counts = PD.cov_from_gram(out[1])
    x = ref["r1"][:, out[0]].astype(np.float64)
    for i, j in ((0, 1), (1, 3), (2, 2), (5, 20)):
        both = (x[:, i] != 0) & (x[:, j] != 0)
        assert counts[i, j] == both.sum()
        if both.sum() > 1:
            want = np.cov(x[both, i], x[both, j], bias=True)[0, 1]
            assert abs(cov[i, j] - want) <= 1e-9 * max(abs(want), 1.0), (i, j)


def test_the_batch_does_not_change_the_result(PD):
    ref = reference(PD)
    a = PD.simulate_pd_covariance(*ARGS, STRIDE, seed=SEED, batch=16)
    b = PD.simulate_pd_covariance(*ARGS, STRIDE, seed=SEED, batch=48)
    check_against_rows(ref, a)
    for u, v in zip(a, b):
        assert (u == v).all()


def test_explicit_steps_and_pick_first(PD):
    ref = reference(PD)
    steps = [0, 1, 50, 219, 220]
    out = PD.simulate_pd_covariance(*ARGS, steps, seed=SEED, pick="first", batch=20)
    assert out[0].tolist() == steps and (out[1] == np_gram(ref["r1"], steps)).all() and (out[2] == ref["mom"]).all()


def test_pick_multi_at_3_6(PD, capfd):
    args = (0.42, 3, 6, 10, 40, False, False, 48)
    p = PD.E.CodeParams(3, 6, 10, 20, 40)
    assert PD.E.peel_pick_deg_supported(p, 200)                          # the shape is taken: the run below is the multi kernel's
    _, r1, plrs = PD.simulate_peeling_decoder_ldpc(*args, [], rng="philox", seed=SEED)
    _, mom, _ = PD.simulate_peeling_decoder_ldpc(*args, [], rng="philox", seed=SEED, want_moments=True)
    capfd.readouterr()
    steps, gram, mom_c, plrs_c = PD.simulate_pd_covariance(*args, STRIDE, seed=SEED, pick="multi", batch=20)
    assert "cn_build ring + peel_pick_multi" in capfd.readouterr().err
    assert (steps == np.arange(0, r1.shape[1], STRIDE)).all()
    assert (gram == np_gram(r1, steps)).all() and (mom_c == mom).all() and (plrs_c == plrs).all() and gram[2].max() > 0


def test_the_command_line_round_trips(PD, tmp_path):
    ref = reference(PD)
    out = tmp_path / "cov.pkl"
    PD.main_simulate_covariance([str(out), "4", "8", "10", "40", "0.45", "N", "U", "48", str(STRIDE), "--seed", str(SEED),
                                 "--batch", "16"])
    with open(out, "rb") as f:
        loaded = PD._ArraysOnly(f).load()
    assert isinstance(loaded, tuple) and len(loaded) == 4 and all(isinstance(x, np.ndarray) for x in loaded)
    check_against_rows(ref, loaded)
