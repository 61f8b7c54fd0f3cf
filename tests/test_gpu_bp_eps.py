"""Unlimited full BP over an eps grid from one code, on a real device (-m gpu): engine.full_bp_eps against engine.full_bp
(max_it = 0) point by point on the same code — and against engine.full_bp_fixpoint where dv = 4 — the condition that makes that
comparison mean something (trials fail, trials decode, residuals of size-2 stopping sets only, several blocks in error), the
workspace form, the overflow re-scan in a stage >= 1, a batch split in two, and run_grid_fused / bp_lim_iter --eps-fused against
Simulator(schedule="fixpoint").run_point(0, eps_k, …), single rank and two ranks.  Every reference is computed once per shape and
shared (tests/test_gpu_buffer_contracts_bp_eps.py imports it)."""
import os
import pickle

import numpy as np
import pytest

from conftest import require_gpu
from test_eps_host import ES, QCAP, WORKSPACE_M
from test_gpu_cli_ranks import _run, _same_files

pytestmark = pytest.mark.gpu
T = 256
SEED = 20261
COLS = [0, 1, 2, 3, 4, 6, 7]                                            # every column but the rounds

# key -> (dv, dc, L, N, is_term, 2-byte rows, doped, es)
SHAPES = {
    "4-8-L12-N16": (4, 8, 12, 16, True, True, (), ES),                  # dv = 4 instance, 2-byte rows
    "4-8-L12-N16-int32": (4, 8, 12, 16, True, False, (), ES),
    "3-6-L10-N20-open": (3, 6, 10, 20, False, True, (), ES),            # generic dv, cn_lim < nk
    "3-6-L10-N20": (3, 6, 10, 20, True, True, (), ES),
    "5-10-L10-N20": (5, 10, 10, 20, True, True, (), ES),
    "3-6-L11-N18": (3, 6, 11, 18, True, True, (), ES),                  # n = 198: level rows that are not 4-byte aligned
    "4-8-L12-N64-doped3": (4, 8, 12, 64, True, True, (3,), [0.54, 0.52, 0.50, 0.48, 0.46, 0.44]),
    "4-8-L12-N16-K1": (4, 8, 12, 16, True, True, (), [0.46]),
    "4-8-L12-N16-K64": (4, 8, 12, 16, True, True, (), list(np.linspace(0.6, 0.2, 64))),
}
# The terminated Olmos shapes of the six-point grid.  (The truncated (3,6) chain is compared above but cannot meet the
# condition: its tail CNs never fire, so every trial keeps VNs at every point and none decodes.)
CONDITION = ["4-8-L12-N16", "3-6-L10-N20", "5-10-L10-N20"]


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the full-BP eps tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


_CACHE = {}


def reference(E, p, es, ntrials, trial0, is_term, a16, doped):
    """Per point: the sampler at that eps and full_bp without a cap.  -> the code, the channels, [(counters, erased bits)]."""
    d_adj, chans, refs = None, [], []
    for e in es:
        d_adj, d_ch = E.sample_philox(p, SEED, trial0, ntrials, e, doped, adj16=a16)
        ref = E.full_bp(p, d_adj, d_ch, max_it=0, is_term=is_term, want_erased=True)
        fix = E.full_bp_fixpoint(p, d_adj, d_ch, is_term=is_term, want_erased=True) if p.dv == 4 else None
        synchronize()
        cnt, bits = ref["counters"].cpu().numpy(), ref["erased"].cpu().numpy().view(np.uint32)
        if fix is not None:                                              # the kernel this one is specified against agrees
            assert (fix["counters"].cpu().numpy()[:, COLS] == cnt[:, COLS]).all()
            assert (fix["erased"].cpu().numpy().view(np.uint32) == bits).all()
        chans.append(d_ch.cpu().numpy().view(np.uint32))
        refs.append((cnt, bits))
    return d_adj, chans, refs


def case(E, key, ntrials=T):
    """The code of a shape, its levels, and per point of its grid the channel words and full_bp's answer: computed once."""
    if (key, ntrials) in _CACHE:
        return _CACHE[key, ntrials]
    dv, dc, L, N, is_term, a16, doped, es = SHAPES[key]
    p = E.make_params(dv, dc, L, N)
    d_adj, chans, refs = reference(E, p, es, ntrials, 7, is_term, a16, doped)
    d_lev = E.channel_levels(p, SEED, 7, ntrials, es, doped)
    synchronize()
    c = dict(p=p, es=es, is_term=is_term, d_adj=d_adj, d_lev=d_lev, chans=chans, refs=refs, adj=d_adj.cpu().numpy().copy(),
             lev=d_lev.cpu().numpy().copy())
    _CACHE[key, ntrials] = c
    return c


def assert_equals_full_bp(c, got, what):
    cnt, bits = got["counters"].cpu().numpy(), got["erased"].cpu().numpy().view(np.uint32)
    K = len(c["es"])
    assert cnt.shape == (K,) + c["refs"][0][0].shape and bits.shape == (K,) + c["refs"][0][1].shape
    for k in range(K):
        ref_cnt, ref_bits = c["refs"][k]
        for col in COLS:
            bad = np.flatnonzero(cnt[k][:, col] != ref_cnt[:, col])
            assert bad.size == 0, (what, "point", k, "column", col, "trial", int(bad[0]), cnt[k][bad[0]], ref_cnt[bad[0]])
        assert (cnt[k][:, [4, 6]] == 0).all() and (cnt[k][:, 5] >= 0).all()
        assert (bits[k] == ref_bits).all(), (what, "point", k, "erased bits")
    return cnt


# ---- the decoder against full_bp ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_the_decoder_equals_full_bp_at_every_point(E, key):
    import torch
    c = case(E, key)
    p, K = c["p"], len(c["es"])
    for k in range(K):                                                   # the levels ARE the channels the references decoded
        assert (E.pack_bits(c["lev"] > k) == c["chans"][k]).all()
    got = E.full_bp_eps(p, c["d_adj"], c["d_lev"], K, is_term=c["is_term"], want_erased=True)
    synchronize()
    assert_equals_full_bp(c, got, key)
    assert c["d_adj"].dtype == (torch.int16 if SHAPES[key][5] else torch.int32)
    if key == "3-6-L10-N20-open":
        assert p.L * p.cns_pos < p.nk and (c["refs"][-1][0][:, 0] > 0).mean() > 0.9     # the tail holds VNs at every point
    # without the erased bits the rows are the same
    bare = E.full_bp_eps(p, c["d_adj"], c["d_lev"], K, is_term=c["is_term"])
    synchronize()
    assert bare["erased"] is None and (bare["counters"][:, :, COLS] == got["counters"][:, :, COLS]).all()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_lev"].cpu().numpy() == c["lev"]).all()


@pytest.mark.parametrize("key", CONDITION)
def test_the_inputs_exercise_every_branch(E, key):
    """From full_bp's rows alone: at the first point and at the last some trial fails and some trial decodes; at least three
    (trial, point) pairs keep a residual made of size-2 stopping sets only (num_erasures > 0, num_erasures_exp == 0); at least
    one pair has two or more blocks in error, where only the first position with a positive expurgated count contributes."""
    c = case(E, key)
    cnt = np.stack([r[0] for r in c["refs"]])                             # [K, T, 8]
    ne, be, ee = cnt[:, :, 0], cnt[:, :, 1], cnt[:, :, 2]
    size2_only, several = int(((ne > 0) & (ee == 0)).sum()), int((be >= 2).sum())
    print(key, "failing trials per point:", (ne > 0).sum(axis=1).tolist(), "of", T, "| residuals of size-2 sets only:", size2_only,
          "| pairs with >= 2 blocks in error:", several)
    for k in (0, -1):
        assert (ne[k] > 0).any() and (ne[k] == 0).any()
    assert size2_only >= 3 and several >= 1


def test_the_workspace_form(E):
    """(4,8), L = 50 with int32 rows at peel_sweep_eps's smallest N in the workspace (this kernel's CN words are there too)."""
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    es, nt = [0.48, 0.46, 0.44], 4
    assert E.full_bp_eps_workspace_bytes(p, nt, False) == nt * 4 * p.nk > 0
    d_adj, chans, refs = reference(E, p, es, nt, 0, True, False, ())
    d_lev = E.channel_levels(p, SEED, 0, nt, es)
    got = E.full_bp_eps(p, d_adj, d_lev, 3, want_erased=True)
    synchronize()
    cnt = assert_equals_full_bp(dict(es=es, refs=refs), got, "workspace")
    assert (cnt[0][:, 0] > 0).any()                                       # something failed at 0.48


def host_rounds(adj, U, cn_lim, ncn):
    """The kernel's rounds of one stage on the host (they are deterministic as sets: a round releases the lone VN of every
    frontier CN, and queues every CN < cn_lim whose count passes from two or more to one or none): the residual and the largest
    number of CNs one round queues."""
    U = U.copy()
    cnt = np.bincount(adj[U].ravel(), minlength=ncn)
    frontier = np.flatnonzero(cnt[:cn_lim] == 1)
    most = 0
    while frontier.size:
        lone = np.flatnonzero(U & np.isin(adj, frontier[cnt[frontier] == 1]).any(axis=1))
        U[lone] = False
        after = cnt - np.bincount(adj[lone].ravel(), minlength=ncn)
        frontier = np.flatnonzero((cnt[:cn_lim] >= 2) & (after[:cn_lim] <= 1))
        most = max(most, frontier.size)
        cnt = after
    return U, most


def test_the_overflow_rescan_in_a_later_stage(E, monkeypatch):
    """Queues of one entry overflow wherever a round queues two CNs, also in the stages after the first, and the rows and bits are
    unchanged; only the rounds may differ.  That a stage >= 1 does overflow is read off the reference on the host."""
    key = "4-8-L12-N16"
    c = case(E, key)
    p, K = c["p"], len(c["es"])
    adj = E.adj16_to_global(p, c["adj"])
    late = 0
    for t in range(T):
        for k in range(1, K):
            R_prev = E.unpack_bits(c["refs"][k - 1][1][t], p.n).astype(bool)
            U = R_prev & (c["lev"][t] > k)
            if not U.any():
                break
            R, most = host_rounds(adj[t], U, p.nk, p.nk)
            assert (R == E.unpack_bits(c["refs"][k][1][t], p.n).astype(bool)).all()
            late += most >= 2
    print("stages >= 1 in which a round queues two or more CNs:", late)
    assert late >= 3
    args = (p, c["d_adj"], c["d_lev"], K)
    monkeypatch.delenv(QCAP, raising=False)
    free = E.full_bp_eps(*args, want_erased=True)
    monkeypatch.setenv(QCAP, "1")
    capped = E.full_bp_eps(*args, want_erased=True)
    synchronize()
    monkeypatch.undo()
    a = assert_equals_full_bp(c, free, "no cap")
    b = assert_equals_full_bp(c, capped, "queues of one entry")
    print("rounds by stage:", b[:, :, 5].sum(axis=1).tolist(), "without the cap:", a[:, :, 5].sum(axis=1).tolist())


def test_a_batch_split_in_two_and_counters_views(E):
    import torch
    c = case(E, "5-10-L10-N20")
    p, K = c["p"], len(c["es"])
    T1 = T // 3 + 1
    buf = torch.full((K * T * 8 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    one = E.full_bp_eps(p, c["d_adj"], c["d_lev"], K, want_erased=True, counters=buf[:K * T * 8].view(K, T, 8))
    first = E.full_bp_eps(p, c["d_adj"][:T1], c["d_lev"][:T1], K, want_erased=True)
    second = E.full_bp_eps(p, c["d_adj"][T1:], c["d_lev"][T1:], K, want_erased=True)
    synchronize()
    assert one["counters"].data_ptr() == buf.data_ptr() and (buf[K * T * 8:] == 0x5A5A5A5A).all()
    assert_equals_full_bp(c, one, "one call into a view")
    two = {"counters": torch.cat([first["counters"], second["counters"]], dim=1),
           "erased": torch.cat([first["erased"], second["erased"]], dim=1)}
    assert_equals_full_bp(c, two, "two calls")
    with pytest.raises(AssertionError):
        E.full_bp_eps(p, c["d_adj"], c["d_lev"], K, counters=buf[:K * T * 8].view(T, K, 8))


# ---- the driver and the command line ----------------------------------------------------------------------------------------
GRID_ES = [0.44, 0.50, 0.46, 0.40, 0.48, 0.44, 0.42]                     # unsorted, with a duplicate
MIN_FE, MAX_FRAMES = 100, 300


def same_runs(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def counted(run):
    """A point's run counters without "iterations": the sum of column 5, which every fixpoint kernel fills with rounds of its
    own (the header says so) and no file holds."""
    assert "iterations" in run and len(run) == 9
    return {k: v for k, v in run.items() if k != "iterations"}


def test_the_grid_equals_run_point_of_point_zero(E):
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    p = E.make_params(4, 8, 12, 16)
    sim = BP.Simulator(p, schedule="fixpoint", batch=64, seed=31, index=2, runs=True, device="cuda:0")
    want = [sim.run_point(0, e, MIN_FE, MAX_FRAMES) for e in GRID_ES]
    got = BP.run_grid_fused(p, GRID_ES, MIN_FE, MAX_FRAMES, seed=31, index=2, batch=64, device="cuda:0", runs=True)
    synchronize()
    stops = [pt.f for pt in want]
    print("stop frames by point:", stops, "frame errors:", [pt.run["frame_err"] for pt in want])
    assert len(set(stops)) >= 3 and stops[1] < 200 and stops[3] == MAX_FRAMES and want[3].run["frame_err"] < MIN_FE
    assert [pt.eps for pt in got] == GRID_ES
    for a, b in zip(got, want):
        assert counted(a.run) == counted(b.run) and a.row() == b.row() and not a.bad, (a.eps, a.run, b.run)
        assert same_runs(a.runs, b.runs), a.eps
    bare = BP.run_grid_fused(p, GRID_ES, MIN_FE, MAX_FRAMES, seed=31, index=2, batch=64, device="cuda:0")
    assert [pt.run for pt in bare] == [pt.run for pt in got] and all(pt.runs is None for pt in bare)


CLI = ["0", "0", "0", "1000000", "--schedule", "fixpoint", "--N", "16", "--L", "12", "--num-points", "6", "--eps-delta", "0.02",
       "--max-frames", "300", "--min-frame-err", "100", "--batch", "64", "--seed", "4242", "--quiet"]


def test_the_command_line_writes_the_point_zero_rows(E, tmp_path):
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    dirs = {m: str(tmp_path / m) for m in ("on", "off", "auto", "none")}
    assert BP.bp_lim_iter(CLI + ["--eps-fused", "on", "--runs", "--outdir", dirs["on"]]) == 0
    assert BP.bp_lim_iter(CLI + ["--eps-fused", "off", "--runs", "--outdir", dirs["off"]]) == 0
    assert BP.bp_lim_iter(CLI + ["--eps-fused", "auto", "--runs", "--outdir", dirs["auto"]]) == 0
    assert BP.bp_lim_iter(CLI + ["--runs", "--outdir", dirs["none"]]) == 0
    synchronize()
    _same_files(dirs["off"], dirs["none"], 2)                            # off and auto write the unfused files byte for byte
    _same_files(dirs["auto"], dirs["none"], 2)
    name = [n for n in sorted(os.listdir(dirs["on"])) if n.endswith(".dat")]
    assert sorted(os.listdir(dirs["on"])) == sorted(os.listdir(dirs["none"])) and len(name) == 1
    fused = open(os.path.join(dirs["on"], name[0])).read().splitlines(True)
    loop = open(os.path.join(dirs["none"], name[0])).read().splitlines(True)
    assert len(fused) == len(loop) == 7 and fused[:2] == loop[:2]        # the header and point 0
    assert fused[2:] != loop[2:]                                         # ... the other points saw other codes
    p = E.make_params(4, 8, 12, 16)
    sim = BP.Simulator(p, schedule="fixpoint", max_it=1000000, batch=64, seed=4242, index=0, runs=True, device="cuda:0")
    pkl = pickle.load(open(os.path.join(dirs["on"], name[0] + ".runs.pkl"), "rb"))
    assert len(pkl) == 6
    for k in range(6):
        e = 0.48 - k * 0.02
        pt = sim.run_point(0, e, 100, 300)
        assert fused[1 + k] == pt.row(), k
        assert pkl[k]["eps"] == pt.eps and pkl[k]["frames"] == pt.f and same_runs({n: pkl[k][n] for n in pt.runs}, pt.runs)


def test_two_ranks_write_the_single_rank_fused_file(tmp_path):
    require_gpu()
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir(); d2.mkdir()
    args = ["bp_lim_iter", *CLI, "--eps-fused", "on", "--runs"]
    _run(1, "fl_scaling_sc_ldpc_amd.bp_decoding", [*args, "--outdir", str(d1)])
    _run(2, "fl_scaling_sc_ldpc_amd.bp_decoding", [*args, "--outdir", str(d2)])
    _same_files(str(d1), str(d2), 2)
