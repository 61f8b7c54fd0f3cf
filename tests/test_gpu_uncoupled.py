"""The uncoupled ensemble in throughput mode (-m gpu): scldpc_sample_philox_uncoupled_device against the loop over the CPU twin
that include/scldpc_uncoupled.h fixes as its law — candidate a of trial t is oracle.sample_philox(Params(dv, dc, 1, cns_pos, M),
seed, t + (a << 40), eps, (), "tail_biting"), the first one without a repeated CN in a row is the trial's graph and channel —
the cap, the sharding, the acceptance rate against numpy's own generator, and simulate_peeling_decoder_ldpc_uncoupled(rng="philox")
trial by trial against pd_oracle.random_pick_trial_philox_fast on the twin's graph.  Integer work: exact, no tolerance, except the
one statistical test, whose bound is stated there."""
import functools

import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

SEED, TRIAL0, EPS = 91, 5, 0.45
# (dv, dc, M, trials): odd cns_pos and dc not a power of two at M = 342; 8190 sockets (two Philox calls per thread) at M = 2730
SHAPES = [(3, 6, 16, 64), (3, 6, 24, 64), (3, 6, 100, 32), (3, 6, 342, 16), (3, 6, 2730, 4), (2, 4, 32, 32), (3, 4, 16, 32), (4, 6, 48, 8)]


def params(dv, dc, M):
    from fl_scaling_sc_ldpc_amd import engine as E
    return E.CodeParams(dv, dc, 1, dv * M // dc, M)


def simple(adj):
    s = np.sort(adj, axis=1)
    return not (s[:, 1:] == s[:, :-1]).any()


@functools.lru_cache(maxsize=None)
def twin(dv, dc, M, seed, trial0, T, eps, cap):
    """(rows int32 [T, M, dv], words uint32 [T, nw], attempts int32 [T]) of the law's loop on the CPU; a trial without an accepted
    candidate within cap: attempts 0, zeros.  Never modified."""
    from oracle import oracle as O
    O.build(with_reference=False)
    po = O.Params(dv, dc, 1, dv * M // dc, M)
    rows = np.zeros((T, M, dv), dtype=np.int32)
    words = np.zeros((T, (M + 31) // 32), dtype=np.uint32)
    att = np.zeros(T, dtype=np.int32)
    for k in range(T):
        for a in range(cap):
            adj, ch = O.sample_philox(po, seed, trial0 + k + (a << 40), eps, (), "tail_biting")
            if simple(adj):
                rows[k], words[k], att[k] = adj, ch, a + 1
                break
    for x in (rows, words, att):
        x.setflags(write=False)
    return rows, words, att


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def device_sample(E, dv, dc, M, seed, trial0, T, eps, cap):
    d_adj, d_ch, d_att = E.sample_philox_uncoupled(params(dv, dc, M), seed, trial0, T, eps, cap)
    assert tuple(d_adj.shape) == (T, M, dv) and tuple(d_ch.shape) == (T, (M + 31) // 32) and tuple(d_att.shape) == (T,)
    return d_adj.cpu().numpy(), d_ch.cpu().numpy().view(np.uint32), d_att.cpu().numpy()


@pytest.mark.parametrize("dv,dc,M,T", SHAPES, ids=["%d-%d-M%d" % s[:3] for s in SHAPES])
def test_rows_channel_and_attempts_equal_the_twin(E, dv, dc, M, T):
    cap = 1 << 16
    assert E.uncoupled_supported(params(dv, dc, M))
    rows, words, att = twin(dv, dc, M, SEED, TRIAL0, T, EPS, cap)
    assert (att > 0).all(), "the reference accepts every listed trial within the cap"
    g_rows, g_words, g_att = device_sample(E, dv, dc, M, SEED, TRIAL0, T, EPS, cap)
    print("attempts mean %.1f max %d" % (g_att.mean(), g_att.max()))
    assert (g_att == att).all(), (g_att, att)
    assert (g_rows == rows).all() and (g_words == words).all()
    cns = dv * M // dc
    for t in range(T):
        assert simple(g_rows[t])                                                  # dv distinct CNs in every row
        assert (np.bincount(g_rows[t].reshape(-1), minlength=cns) == dc).all()    # every CN exactly dc sockets


def test_the_cap_leaves_zeros_and_attempts_zero(E):
    dv, dc, M, T = 3, 6, 16, 64
    rows, words, att = twin(dv, dc, M, SEED, TRIAL0, T, EPS, 1 << 16)
    within = att <= 100
    assert within.any() and (~within).any() and att.min() >= 1
    g_rows, g_words, g_att = device_sample(E, dv, dc, M, SEED, TRIAL0, T, EPS, 100)
    assert (g_att[within] == att[within]).all() and (g_rows[within] == rows[within]).all() and (g_words[within] == words[within]).all()
    assert (g_att[~within] == 0).all() and (g_rows[~within] == 0).all() and (g_words[~within] == 0).all()
    # a cap of one attempt: accepted iff the first candidate is simple
    g_rows, g_words, g_att = device_sample(E, 2, 4, 32, SEED, TRIAL0, 32, EPS, 1)
    r2, w2, a2 = twin(2, 4, 32, SEED, TRIAL0, 32, EPS, 1 << 16)
    first = a2 == 1
    assert first.any() and (~first).any()
    assert (g_att == first).all() and (g_rows[first] == r2[first]).all() and (g_rows[~first] == 0).all() and (g_words[~first] == 0).all()


def test_a_pair_that_is_never_simple_within_the_cap(E):
    """(5,10,8) has cns_pos = 4 < dv: no simple graph exists (the twin accepts none), and the header's shape rule refuses the shape
    before a launch that would run every trial to the cap; the simulator's RuntimeError there is the library's.  (5,10,16),
    cns_pos = 8, is the smallest (5,10) the entry takes: about exp(18) attempts per graph, none within 64."""
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert twin(5, 10, 8, SEED, TRIAL0, 2, EPS, 64)[2].tolist() == [0, 0]
    with pytest.raises(E.ScldpcError, match="no simple graph with dv > cns_pos"):
        device_sample(E, 5, 10, 8, SEED, TRIAL0, 2, EPS, 64)
    with pytest.raises(RuntimeError, match="no simple graph with dv > cns_pos"):
        PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 5, 10, 8, 2, rng="philox", seed=SEED, max_attempts=64)
    assert twin(5, 10, 16, SEED, TRIAL0, 2, EPS, 64)[2].tolist() == [0, 0] and twin(5, 10, 16, SEED, 0, 2, 0.4, 64)[2].tolist() == [0, 0]
    g_rows, g_words, g_att = device_sample(E, 5, 10, 16, SEED, TRIAL0, 2, EPS, 64)
    assert g_att.tolist() == [0, 0] and (g_rows == 0).all() and (g_words == 0).all()
    with pytest.raises(RuntimeError, match=r"trial 0 found no simple graph within max_attempts = 64.*exp\(\(l-1\)\(r-1\)/2\)"):
        PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 5, 10, 16, 2, rng="philox", seed=SEED, max_attempts=64)


def test_a_crowded_bucket_ends_the_trial_with_minus_one(E, monkeypatch):
    """The kernel has no trap: the ranking's nibble-wide counts giving up is reported per trial.  Real keys never get there
    (sixteen in a bucket of mean 0.25), so the diagnostic limit is lowered to two keys in one bucket, which 600 keys in 4096
    buckets always have."""
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    monkeypatch.setenv("SCLDPC_DEBUG_UNCOUPLED_CROWD_LIMIT", "1")
    g_rows, g_words, g_att = device_sample(E, 3, 6, 100, SEED, TRIAL0, 8, EPS, 1 << 16)
    assert (g_att == -1).all() and (g_rows == 0).all() and (g_words == 0).all()
    with pytest.raises(RuntimeError, match="trial 0: sixteen keys met in one bucket"):
        PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 3, 6, 100, 4, rng="philox", seed=SEED)
    monkeypatch.delenv("SCLDPC_DEBUG_UNCOUPLED_CROWD_LIMIT")
    assert (device_sample(E, 3, 6, 100, SEED, TRIAL0, 8, EPS, 1 << 16)[2] > 0).all()


def test_one_call_equals_two_calls(E):
    whole = device_sample(E, 3, 6, 16, SEED, 5, 64, EPS, 1 << 16)
    a, b = device_sample(E, 3, 6, 16, SEED, 5, 32, EPS, 1 << 16), device_sample(E, 3, 6, 16, SEED, 37, 32, EPS, 1 << 16)
    for w, x, y in zip(whole, a, b):
        assert (w == np.concatenate([x, y])).all()
    assert E.sample_philox_uncoupled(params(3, 6, 16), SEED, 5, 0, EPS, 10)[2].numel() == 0      # an empty batch


def test_the_acceptance_rate_is_that_of_numpys_generator(E):
    """The law against the reference's own generator: 2048 accepted graphs at (3,6,24) took sum(attempts) candidates, p~ = 2048 /
    sum; p^ is the accepted share of K = 200 000 candidates drawn as ldpc.gen_slots draws them from np.random.RandomState(3).
    Standard error sqrt(p^(1-p^)/K + p~^2 (1-p~)/T) (a binomial share, and the delta method on the mean of T geometric counts);
    bound 4.5 sigma, as the published-curve tests."""
    l, r, N, T, K = 3, 6, 24, 2048, 200000
    g_att = device_sample(E, l, r, N, 7, 0, T, EPS, 1 << 16)[2]
    assert (g_att > 0).all()
    rs = np.random.RandomState(3)
    cand = np.stack([rs.permutation(l * N) for _ in range(K)]).reshape(K, l, N) // r       # [K, l, N]: row d = edge d of every VN
    s = np.sort(cand, axis=1)
    p_hat = float((~(s[:, 1:, :] == s[:, :-1, :]).any(axis=(1, 2))).mean())
    p_til = T / float(g_att.sum())
    se = np.sqrt(p_hat * (1 - p_hat) / K + p_til ** 2 * (1 - p_til) / T)
    z = (p_til - p_hat) / se
    print("sum attempts %d  p~ %.5f  p^ %.5f  z %.2f" % (g_att.sum(), p_til, p_hat, z))
    assert abs(z) < 4.5, (p_til, p_hat, z)


# ---- end to end ------------------------------------------------------------------------------------------------------------
# (l, r, M, e, trials, trials of the CPU reference that end with erased VNs left: plr > 0).  The last column pins the reference,
# not the device: it is what pd_oracle gives on the twin's graphs with seed 91 and trials 0 .. T - 1, and every case has trials
# of both kinds.
E2E = [(3, 6, 24, 0.45, 16, 14), (3, 6, 342, 0.40, 8, 3), (3, 4, 16, 0.6, 8, 6)]


@functools.lru_cache(maxsize=None)
def e2e_reference(l, r, M, e, T):
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import pd_oracle
    rows, words, att = twin(l, r, M, SEED, 0, T, e, 1 << 16)
    assert (att > 0).all()
    r1s, plrs, nv = [], [], []
    for t in range(T):
        mask = E.unpack_bits(words[t], M).astype(bool)
        r1, plr = pd_oracle.random_pick_trial_philox_fast(rows[t], mask, l, r, 1, M, e, False, SEED, t)
        r1s.append(r1); plrs.append(plr); nv.append(int(mask.sum()))
    r1s, plrs = np.stack(r1s), np.array(plrs)
    r1s.setflags(write=False); plrs.setflags(write=False)
    return r1s, plrs, nv


@pytest.mark.parametrize("l,r,M,e,T,residual", E2E, ids=["%d-%d-M%d" % c[:3] for c in E2E])
def test_the_simulator_equals_the_reference_trial_by_trial(E, l, r, M, e, T, residual):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    r1s, plrs, nv = e2e_reference(l, r, M, e, T)
    assert int((plrs > 0).sum()) == residual                                 # the reference keeps a residual in these trials
    first, r1, plr, num_vns = PD.simulate_peeling_decoder_ldpc_uncoupled(e, l, r, M, T, rng="philox", seed=SEED)
    assert first is None and r1.shape == (T, int(M * (e + 0.1)) + 1) and isinstance(num_vns, list)
    assert (r1 == r1s).all() and (plr == plrs).all() and num_vns == nv
    _, r1b, plrb, nvb = PD.simulate_peeling_decoder_ldpc_uncoupled(e, l, r, M, T, rng="philox", seed=SEED, batch=5)
    assert (r1b == r1).all() and (plrb == plr).all() and nvb == num_vns
    _, mom, plrm, nvm = PD.simulate_peeling_decoder_ldpc_uncoupled(e, l, r, M, T, rng="philox", seed=SEED, batch=5, want_moments=True)
    assert mom.dtype == np.int64 and mom.shape == (3, r1.shape[1])
    assert (mom == np.stack([(r1s != 0).sum(0), r1s.sum(0), (r1s * r1s).sum(0)])).all()
    assert (plrm == plr).all() and nvm == num_vns
