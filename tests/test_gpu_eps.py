"""The eps-descending sweep on a real device (-m gpu): engine.channel_levels against the channel words of sample_philox,
engine.peel_sweep_eps against engine.peel_sweep point by point on the same code (sweep_start = 0), the condition that makes
that comparison mean something (trials fail, trials decode, residuals shrink without vanishing), the workspace form, the
overflow re-scan in a stage >= 1, and simulate_sc_ldpc_curve / ber_sim --eps-fused against the per-eps loop they replace, single
rank and two ranks.  Every reference is computed once per shape and shared (tests/test_gpu_buffer_contracts_eps.py imports it)."""
import numpy as np
import pytest

from conftest import require_gpu
from test_eps_host import ES, QCAP, WORKSPACE_M, same_tuples
from test_gpu_cli_ranks import _run, _same_files

pytestmark = pytest.mark.gpu
T = 256
SEED = 20261

# key -> (l, r, L, M, is_terminated, ensemble, doped, es).  The grids: ES where peel_sweep meets the condition below with it
# (numpy codes of the same law on the CPU: 94 ... 8 of 100 fail at (4,8) M = 32, 75 ... 0 at (5,10), 79 ... 0 on the protograph),
# lower for the tail-biting chain, which has no boundary to start from (100 ... 14 of 100), higher with a doped position (97 ... 0).
SHAPES = {
    "4-8-L12-M32": (4, 8, 12, 32, True, "olmos", (), ES),
    "3-6-L10-M40-open": (3, 6, 10, 40, False, "olmos", (), ES),          # 20 ignored tail positions, total_size < ncn
    "5-10-L10-M40": (5, 10, 10, 40, True, "olmos", (), ES),              # generic dv
    "4-8-L12-M64-tb": (4, 8, 12, 64, True, "tail_biting", (), [0.46, 0.44, 0.42, 0.40, 0.38, 0.36]),
    "4-8-L12-M64-proto": (4, 8, 12, 64, True, "protograph", (), ES),
    "4-8-L12-M64-doped3": (4, 8, 12, 64, True, "olmos", (3,), [0.54, 0.52, 0.50, 0.48, 0.46, 0.44]),
    "4-8-L12-M32-K1": (4, 8, 12, 32, True, "olmos", (), [0.46]),
}
CONDITION = ["4-8-L12-M32", "5-10-L10-M40", "4-8-L12-M64-doped3", "4-8-L12-M64-tb"]   # every terminated Olmos shape, and the ring


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the eps-sweep tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def geometry(key):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    l, r, L, M, term, ens, doped, es = SHAPES[key]
    return PD._Geometry(l, r, L, M, term, True, [])


_CACHE = {}


def case(E, key, ntrials=T):
    """The code of a shape, its levels, and per point of its grid the channel words and peel_sweep's answer: computed once."""
    if (key, ntrials) in _CACHE:
        return _CACHE[key, ntrials]
    l, r, L, M, term, ens, doped, es = SHAPES[key]
    g = geometry(key)
    p = g.params
    d_adj = None
    chans, refs = [], []
    for e in es:
        d_adj, d_ch = E.sample_philox(p, SEED, 7, ntrials, e, doped, adj16=(ens == "olmos"), ensemble=ens)
        ref = E.peel_sweep(p, d_adj, d_ch, g.total_size, 0, g.lost_lo, g.lost_hi, want_lost=True)
        synchronize()
        chans.append(d_ch.cpu().numpy().view(np.uint32))
        refs.append((ref["out"].cpu().numpy(), ref["lost"].cpu().numpy().view(np.uint32)))
    d_lev = E.channel_levels(p, SEED, 7, ntrials, es, doped)
    synchronize()
    c = dict(p=p, g=g, es=es, d_adj=d_adj, d_lev=d_lev, chans=chans, refs=refs, adj=d_adj.cpu().numpy().copy(),
             lev=d_lev.cpu().numpy().copy())
    _CACHE[key, ntrials] = c
    return c


def assert_equals_peel_sweep(c, got, what):
    out, lost = got["out"].cpu().numpy(), got["lost"].cpu().numpy().view(np.uint32)
    K = len(c["es"])
    assert out.shape == (K,) + c["refs"][0][0].shape and lost.shape == (K,) + c["refs"][0][1].shape
    for k in range(K):
        ref_out, ref_lost = c["refs"][k]
        for col in (0, 1, 2, 7):
            bad = np.flatnonzero(out[k][:, col] != ref_out[:, col])
            assert bad.size == 0, (what, "point", k, "column", col, "trial", int(bad[0]), out[k][bad[0]], ref_out[bad[0]])
        assert (out[k][:, [3, 4]] == 0).all() and (out[k][:, 6] >= 0).all()
        assert (lost[k] == ref_lost).all(), (what, "point", k, "lost bits")
    return out


# ---- levels ------------------------------------------------------------------------------------------------------------
LEVEL_SHAPES = {
    "4-8-L12-M64-doped3": (4, 8, 12, 64, "olmos", (3,)),
    "3-6-L12-M50": (3, 6, 12, 50, "olmos", ()),                          # n = 600: a partial last word
    "4-8-L12-M64-tb": (4, 8, 12, 64, "tail_biting", ()),
    "4-8-L12-M64-proto": (4, 8, 12, 64, "protograph", ()),
}


def sampler_words(E, p, ens, doped, e, trial0, ntrials):
    _, d_ch = E.sample_philox(p, SEED, trial0, ntrials, e, doped, adj16=(ens == "olmos"), ensemble=ens)
    return d_ch.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("key", list(LEVEL_SHAPES))
def test_levels_pack_to_the_samplers_channel_words(E, key):
    l, r, L, M, ens, doped = LEVEL_SHAPES[key]
    p = E.make_params(l, r, L, M)
    lev = E.channel_levels(p, SEED, 11, T, ES, doped).cpu().numpy()
    synchronize()
    assert lev.shape == (T, p.n) and lev.dtype == np.uint8 and lev.max() == len(ES) and lev.min() == 0
    for k, e in enumerate(ES):
        want = sampler_words(E, p, ens, doped, e, 11, T)
        assert (E.pack_bits(lev > k) == want).all(), (key, k)
    for d in doped:
        assert not lev[:, d * M:(d + 1) * M].any()
    # a batch split in two calls with trial0 advanced
    a, b = E.channel_levels(p, SEED, 11, 100, ES, doped), E.channel_levels(p, SEED, 111, T - 100, ES, doped)
    assert (np.concatenate([a.cpu().numpy(), b.cpu().numpy()]) == lev).all()


@pytest.mark.parametrize("es", [[0.47], list(np.linspace(0.6, 0.2, 64))], ids=["K1", "K64"])
def test_levels_with_one_point_and_with_sixty_four(E, es):
    p = E.make_params(3, 6, 12, 50)
    lev = E.channel_levels(p, SEED, 3, 64, es).cpu().numpy()
    synchronize()
    assert lev.max() <= len(es)
    for k, e in enumerate(es):
        assert (E.pack_bits(lev > k) == sampler_words(E, p, "olmos", (), e, 3, 64)).all(), k


# ---- the decoder against peel_sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_the_decoder_equals_peel_sweep_at_every_point(E, key):
    c = case(E, key)
    for k, e in enumerate(c["es"]):                                       # the levels ARE the channels the references decoded
        assert (E.pack_bits(c["lev"] > k) == c["chans"][k]).all()
    got = E.peel_sweep_eps(c["p"], c["d_adj"], c["d_lev"], len(c["es"]), c["g"].total_size, c["g"].lost_lo, c["g"].lost_hi,
                           want_lost=True)
    synchronize()
    assert_equals_peel_sweep(c, got, key)
    import torch
    assert c["d_adj"].dtype == (torch.int16 if SHAPES[key][5] == "olmos" else torch.int32)
    if key == "3-6-L10-M40-open":
        assert c["g"].total_size < c["p"].nk and c["g"].lost_hi < c["g"].total_size
    # without the lost bits the rows are the same
    bare = E.peel_sweep_eps(c["p"], c["d_adj"], c["d_lev"], len(c["es"]), c["g"].total_size, c["g"].lost_lo, c["g"].lost_hi)
    assert bare["lost"] is None and (bare["out"] == got["out"]).all()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_lev"].cpu().numpy() == c["lev"]).all()


@pytest.mark.parametrize("key", CONDITION)
def test_the_inputs_exercise_every_branch(E, key):
    """From peel_sweep's outputs alone: at least 10 % of the trials fail at es[0], at least 10 % decode at es[-1], and at least
    one trial has a residual that shrinks but stays non-empty between two neighbouring points."""
    c = case(E, key)
    lost = np.stack([r[0][:, 0] for r in c["refs"]])                      # [K, T]
    print(key, "failing trials per point:", (lost > 0).sum(axis=1).tolist(), "of", T)
    assert (lost[0] > 0).sum() >= T // 10 + 1 and (lost[-1] == 0).sum() >= T // 10 + 1
    assert ((lost[1:] < lost[:-1]) & (lost[1:] > 0)).any()


def test_the_workspace_form(E):
    """The smallest (4,8), L = 50 shape with int32 rows whose CN words leave the LDS (found by the query on the CPU)."""
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    es, nt = [0.48, 0.46, 0.44], 4
    assert E.peel_sweep_eps_workspace_bytes(p, nt, False) == nt * 4 * p.nk > 0
    refs, chans = [], []
    for e in es:
        d_adj, d_ch = E.sample_philox(p, SEED, 0, nt, e)
        ref = E.peel_sweep(p, d_adj, d_ch, p.nk, 0, 0, p.nk, want_lost=True)
        refs.append((ref["out"].cpu().numpy(), ref["lost"].cpu().numpy().view(np.uint32)))
    d_lev = E.channel_levels(p, SEED, 0, nt, es)
    got = E.peel_sweep_eps(p, d_adj, d_lev, 3, p.nk, 0, p.nk, want_lost=True)
    synchronize()
    out = assert_equals_peel_sweep(dict(es=es, refs=refs), got, "workspace")
    assert (out[0][:, 0] > 0).any()                                       # something failed at 0.48


def test_the_overflow_rescan_in_a_later_stage(E, monkeypatch):
    """Queues of two entries overflow in almost every round, also in the stages after the first, and the results are unchanged.
    Without a sweep_start nothing is barred from firing, so the re-scan after an overflow finds exactly the CNs the lost queue
    held: the rounds in [5] cannot grow, and the re-scans show in [6] (0 everywhere with the queues this shape gets)."""
    c = case(E, "4-8-L12-M32")
    args = (c["p"], c["d_adj"], c["d_lev"], len(c["es"]), c["g"].total_size, c["g"].lost_lo, c["g"].lost_hi)
    monkeypatch.delenv(QCAP, raising=False)
    free = E.peel_sweep_eps(*args, want_lost=True)
    monkeypatch.setenv(QCAP, "2")
    capped = E.peel_sweep_eps(*args, want_lost=True)
    synchronize()
    monkeypatch.undo()
    a = assert_equals_peel_sweep(c, free, "no cap")
    b = assert_equals_peel_sweep(c, capped, "queues of 2 entries")
    print("re-scans by stage:", b[:, :, 6].sum(axis=1).tolist(), "rounds by stage:", b[:, :, 5].sum(axis=1).tolist(),
          "without the cap:", a[:, :, 5].sum(axis=1).tolist())
    assert (a[:, :, 6] == 0).all() and (b[:, :, 5] >= a[:, :, 5]).all()
    assert (b[0, :, 6] > 0).any() and (b[1:, :, 6] > 0).any()             # a stage >= 1 overflowed and scanned again
    assert (b[:, :, 6] <= np.maximum(b[:, :, 5] - 1, 0)).all()            # a re-scan is one of the stage's rounds, never the first


# ---- the simulator and the command line -----------------------------------------------------------------------------------
CURVE_ES = [0.44, 0.50, 0.46, 0.44, 0.48, 0.42]                          # unsorted, with a duplicate
CURVE = (4, 8, 12, 64, True, False, True, False, 600, 100)


def test_the_curve_equals_the_loop_over_eps(E):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    kw = dict(seed=31, batch=256, device="cuda:0")
    got = PD.simulate_sc_ldpc_curve(CURVE_ES, *CURVE, [], **kw)
    want = [PD.simulate_sc_ldpc(e, *CURVE, [], rng="philox", sweep="first", **kw) for e in CURVE_ES]
    assert same_tuples(got, want), ([t[:8] for t in got], [t[:8] for t in want])
    stops = sorted(set(t[5] for t in want))
    assert len(stops) >= 3 and stops[-1] == 600 and stops[0] < 256        # points stop at different trials and drop out
    soft = {3: 0.5}
    got = PD.simulate_sc_ldpc_curve([0.46, 0.50], *CURVE, soft, **kw)
    want = [PD.simulate_sc_ldpc(e, *CURVE, soft, rng="philox", sweep="first", **kw) for e in (0.46, 0.50)]
    assert same_tuples(got, want)
    hard = PD.simulate_sc_ldpc_curve([0.50, 0.52], 4, 8, 13, 64, True, False, True, False, 300, 100, [3], **kw)
    assert same_tuples(hard, [PD.simulate_sc_ldpc(e, 4, 8, 13, 64, True, False, True, False, 300, 100, [3], rng="philox", **kw)
                              for e in (0.50, 0.52)])


ARGV = ["4", "8", "12", "64", str(CURVE_ES), "T", "U", "B", "NTB", "600", "100", "[]", "--rng", "philox", "--seed", "31", "--batch", "256"]


def test_ber_sim_eps_fused_writes_the_same_file(E, tmp_path):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    a, b = str(tmp_path / "loop.dat"), str(tmp_path / "fused.dat")
    PD.main_simulate_sc_ldpc([a] + ARGV)
    PD.main_simulate_sc_ldpc([b] + ARGV + ["--eps-fused", "on"])
    ta, tb = open(a, "rb").read(), open(b, "rb").read()
    assert ta == tb and len(ta.splitlines()) == 1 + len(CURVE_ES)


def test_ber_sim_eps_fused_two_ranks_write_the_single_rank_file(tmp_path):
    require_gpu()
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir(); d2.mkdir()
    _run(1, "fl_scaling_sc_ldpc_amd.peeling_decoding", ["ber_sim", str(d1 / "table.dat"), *ARGV])
    _run(2, "fl_scaling_sc_ldpc_amd.peeling_decoding", ["ber_sim", str(d2 / "table.dat"), *ARGV, "--eps-fused", "on"])
    _same_files(str(d1), str(d2), 1)
