"""Exact per-VN and per-position erasure thresholds on a real device (-m gpu): engine.vn_threshold against the incremental
reference tests/test_vn_thresh_host.host_vn_thresholds over the downloaded rows and keys, against its sibling
engine.frame_threshold and the grid walker engine.full_bp_eps, under the debug caps (lists and queues of a few entries), with
tied keys, in the workspace form, and run_vn_thresholds / bp_curves against run_grid_fused and run_thresholds on the same frames,
single rank and two ranks.  Every equality is exact.  Every reference is computed once per shape and shared
(tests/test_gpu_buffer_contracts_vn_thresh.py imports it)."""
import os
import pickle

import numpy as np
import pytest

from conftest import require_gpu
from test_eps_host import QCAP, WORKSPACE_M
from test_gpu_bp_eps import host_rounds
from test_gpu_cli_ranks import _run, _same_files
from test_vn_thresh_host import CCAP, NONE, host_vn_thresholds

pytestmark = pytest.mark.gpu
T = 256
SEED, TRIAL0 = 20261, 7
COLS = [0, 1, 2, 3, 4, 7]                                               # every column but the two diagnostics
# key -> (dv, dc, L, N, is_term, 2-byte rows, doped)
SHAPES = {
    "4-8-L12-N16": (4, 8, 12, 16, True, True, ()),                      # dv = 4 instance, 2-byte rows
    "4-8-L12-N16-int32": (4, 8, 12, 16, True, False, ()),
    "3-6-L10-N20": (3, 6, 10, 20, True, True, ()),                      # generic dv
    "3-6-L10-N20-open": (3, 6, 10, 20, False, False, ()),               # cn_lim < nk, 4-byte rows
    "5-10-L8-N16": (5, 10, 8, 16, True, True, ()),
    "3-6-L11-N18": (3, 6, 11, 18, True, True, ()),                      # n = 198: scalar key loads, a partial last word
    "4-8-L12-N64-doped3": (4, 8, 12, 64, True, True, (3,)),
}
WINDOW = (0.30, 0.55)


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the VN-threshold tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def global_adj(E, p, adj):
    return E.adj16_to_global(p, adj) if adj.dtype == np.int16 else adj


def grid_of(t_lo, t_hi, K):
    return sorted(set(int(t) for t in np.linspace(t_lo, t_hi, K)))


def host_reference(p, adj, keys, t_lo, t_hi, is_term, grid):
    """host_vn_thresholds frame by frame: rows int64 [T, 6] (COLS), pos [T, L], counts [T, K], tau [T, n], and the releases."""
    cn_lim = p.nk if is_term else p.L * p.cns_pos
    refs = [host_vn_thresholds(adj[t], keys[t], t_lo, t_hi, cn_lim, p.nk, p.vns_pos, grid) for t in range(adj.shape[0])]
    return dict(rows=np.array([r["row"] for r in refs], dtype=np.int64), pos=np.array([r["pos"] for r in refs]),
                counts=np.array([r["counts"] for r in refs]).reshape(len(refs), len(grid)), tau=np.array([r["tau"] for r in refs]),
                releases=[r["releases"] for r in refs])


_CACHE = {}


def case(E, key):
    """The codes of a shape, their keys, and the reference of every frame on the 256-point grid: computed once."""
    if key in _CACHE:
        return _CACHE[key]
    dv, dc, L, N, is_term, a16, doped = SHAPES[key]
    p = E.make_params(dv, dc, L, N)
    t_lo, t_hi = E.erasure_threshold(WINDOW[0]), E.erasure_threshold(WINDOW[1])
    d_adj, _ch = E.sample_philox(p, SEED, TRIAL0, T, WINDOW[1], doped, adj16=a16)
    d_keys = E.channel_keys(p, SEED, TRIAL0, T, doped)
    synchronize()
    adj, keys = d_adj.cpu().numpy().copy(), d_keys.cpu().numpy().view(np.uint32).copy()
    grid = grid_of(t_lo, t_hi, 256)
    assert len(grid) == 256
    c = dict(p=p, is_term=is_term, doped=doped, t_lo=t_lo, t_hi=t_hi, d_adj=d_adj, d_keys=d_keys, adj=adj, keys=keys, grid=grid,
             gadj=global_adj(E, p, adj))
    c["ref"] = host_reference(p, c["gadj"], keys, t_lo, t_hi, is_term, grid)
    _CACHE[key] = c
    return c


def unsigned(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def assert_equals_reference(ref, got, what, counts=None):
    """Rows [0-4, 7], pos_thresh, counts and tau of a device result against the reference's."""
    r = got["rows"].cpu().numpy().astype(np.int64)
    assert r.shape == (ref["rows"].shape[0], 8)
    for i, col in enumerate(COLS):
        bad = np.flatnonzero(r[:, col] != ref["rows"][:, i])
        assert bad.size == 0, (what, "column", col, "frame", int(bad[0]), r[bad[0]].tolist(), ref["rows"][bad[0]].tolist())
    assert (r[:, 5] >= 0).all() and (r[:, 6] >= 0).all()
    pos = unsigned(got["pos_thresh"])
    assert pos.shape == ref["pos"].shape and (pos == ref["pos"]).all(), (what, "pos_thresh", np.argwhere(pos != ref["pos"])[:3].tolist())
    want_counts = ref["counts"] if counts is None else counts
    if want_counts.shape[1]:
        cnt = got["counts"].cpu().numpy().astype(np.int64)
        assert cnt.shape == want_counts.shape and (cnt == want_counts).all(), (what, "counts")
    else:
        assert got["counts"] is None
    if got["tau"] is not None:
        tau = unsigned(got["tau"])
        assert tau.shape == ref["tau"].shape and (tau == ref["tau"]).all(), (what, "tau", np.argwhere(tau != ref["tau"])[:3].tolist())
    return r


# ---- against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SHAPES))
def test_the_walk_equals_the_reference(E, key):
    import torch
    c = case(E, key)
    p, ref = c["p"], c["ref"]
    args = (p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"])
    got = E.vn_threshold(*args, grid=c["grid"], is_term=c["is_term"], want_tau=True)
    synchronize()
    r = assert_equals_reference(ref, got, key + " K = 256")
    status = r[:, 1]
    print(key, "status 0 / 1 / 2:", [int((status == s).sum()) for s in (0, 1, 2)], "| steps mean %.1f max %d" % (r[:, 4].mean(), r[:, 4].max()),
          "| scans mean %.1f" % r[:, 5].mean(), "| largest release of a step:", max(max(x, default=0) for x in ref["releases"]))
    assert c["d_adj"].dtype == (torch.int16 if SHAPES[key][5] else torch.int32)
    assert r[:, 4].max() >= 10
    if key in ("4-8-L12-N16", "4-8-L12-N16-int32", "3-6-L10-N20"):      # the terminated windows hold thresholds, above and below
        assert (status == 0).sum() >= 100
    # 64 points: every fourth of the 256 and the last
    sub = list(range(0, 256, 4))[:63] + [255]
    got64 = E.vn_threshold(*args, grid=[c["grid"][k] for k in sub], is_term=c["is_term"])
    synchronize()
    assert got64["tau"] is None
    assert_equals_reference(ref, got64, key + " K = 64", counts=ref["counts"][:, sub])
    bare = E.vn_threshold(*args, is_term=c["is_term"])
    synchronize()
    assert_equals_reference(ref, bare, key + " K = 0", counts=ref["counts"][:, :0])
    if key == "3-6-L11-N18":
        assert p.n == 198 and p.n % 32                                   # the last word is partial
    if c["doped"]:
        q = c["doped"][0]
        assert (ref["pos"][:, q] == NONE).all() and (ref["tau"][:, q * p.vns_pos:(q + 1) * p.vns_pos] == NONE).all()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_keys"].cpu().numpy().view(np.uint32) == c["keys"]).all()


# ---- against the sibling kernel and the grid walker -------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["4-8-L12-N16", "3-6-L10-N20-open", "5-10-L8-N16", "4-8-L12-N64-doped3"])
def test_the_walk_against_frame_threshold_and_full_bp_eps(E, key):
    c = case(E, key)
    p = c["p"]
    t_lo, t_hi = c["t_lo"], c["t_hi"]
    es = [float(e) for e in np.linspace(WINDOW[1], WINDOW[0], 16)]      # descending, both ends of the window
    ths = [E.erasure_threshold(e) for e in es]
    assert ths[0] == t_hi and ths[-1] == t_lo and len(set(ths)) == 16
    got = E.vn_threshold(p, c["d_adj"], c["d_keys"], t_lo, t_hi, grid=ths[::-1], is_term=c["is_term"], want_tau=True)
    ft = E.frame_threshold(p, c["d_adj"], c["d_keys"], t_lo, t_hi, is_term=c["is_term"], want_bits=True)
    d_lev = E.channel_levels(p, SEED, TRIAL0, T, es, c["doped"])
    walk = E.full_bp_eps(p, c["d_adj"], d_lev, 16, is_term=c["is_term"], want_erased=True)
    synchronize()
    r, f = got["rows"].cpu().numpy().astype(np.int64), ft["rows"].cpu().numpy().astype(np.int64)
    tau, pos = unsigned(got["tau"]), unsigned(got["pos_thresh"])
    assert (r[:, :2] == f[:, :2]).all() and (r[:, 3] == f[:, 2]).all() and (r[:, 7] == f[:, 7]).all()
    bits = ft["bits"].cpu().numpy().view(np.uint32)
    inside = r[:, 1] == 0
    assert inside.sum() + (r[:, 1] == 2).sum() >= 100 and (E.pack_bits(tau[inside] == r[inside, 0][:, None]) == bits[inside]).all()
    low = r[:, 1] == 2
    assert (E.pack_bits(tau[low] == t_lo) == bits[low]).all()
    cnt, erased = walk["counters"].cpu().numpy(), walk["erased"].cpu().numpy().view(np.uint32)
    counts = got["counts"].cpu().numpy()
    for k, th in enumerate(ths):
        assert (counts[:, 15 - k] == cnt[k, :, 0]).all(), ("num_erasures", k)
        assert ((pos <= th).sum(axis=1) == cnt[k, :, 1]).all(), ("num_blocks_err", k)
        assert (E.pack_bits(tau <= th) == erased[k]).all(), ("erased", k)
    assert cnt[0, :, 0].sum() > cnt[15, :, 0].sum()


# ---- debug caps and ties --------------------------------------------------------------------------------------------------------
def first_chunk_overflows(c, cap):
    """Frames whose first candidate scan must overflow a list of `cap` entries: the first chunk is [t_hi - width, t_hi) with
    width = t_hi * max(1, cap / 2) / |S(t_hi)| clamped to [1, t_hi - t_lo] (the rule of csrc/vn_threshold.hip), and a width of 1
    needs no list."""
    out = []
    for t in range(T):
        members = c["ref"]["tau"][t] != NONE
        if not members.any():
            continue
        width = min(max(c["t_hi"] * max(1, cap // 2) // int(members.sum()), 1), c["t_hi"] - c["t_lo"])
        if width > 1 and (c["keys"][t][members].astype(np.int64) >= c["t_hi"] - width).sum() > cap:
            out.append(t)
    return out


@pytest.mark.parametrize("key", ["4-8-L12-N16", "3-6-L10-N20-open"])
def test_small_lists_and_queues_change_no_answer(E, key, monkeypatch):
    c = case(E, key)
    p, ref = c["p"], c["ref"]
    args = (p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"])
    monkeypatch.delenv(QCAP, raising=False)
    monkeypatch.delenv(CCAP, raising=False)
    free = assert_equals_reference(ref, E.vn_threshold(*args, grid=c["grid"], is_term=c["is_term"], want_tau=True), "no cap")
    synchronize()
    assert (free[:, 6] == 0).all()
    for cap in (1, 3, 64):
        monkeypatch.setenv(CCAP, str(cap))
        got = E.vn_threshold(*args, grid=c["grid"], is_term=c["is_term"], want_tau=True)
        synchronize()
        r = assert_equals_reference(ref, got, "list of %d" % cap)
        must = first_chunk_overflows(c, cap)
        print(key, "list cap", cap, "| frames whose first scan must overflow:", len(must), "| re-scans:", int(r[:, 6].sum()),
              "| scans mean %.1f" % r[:, 5].mean())
        assert (r[must, 6] > 0).all()
        # a chunk is sized for max(1, cap / 2) candidates, so the first one holds more than cap with probability 0.26 (cap 1)
        # and 0.019 (cap 3, Poisson of mean 1) per frame: of 256 frames some must.  A list of 64 is sized for 32 of the at most
        # 200 VNs and overflows nowhere here: that capacity runs the sort over long lists, not the overflow.
        if cap == 1:
            assert len(must) >= 3
        if cap == 3:
            assert len(must) >= 1 and r[:, 6].sum() >= len(must)
        if cap == 64:
            assert must == [] and (r[:, 6] == 0).all()
    monkeypatch.delenv(CCAP)
    # queues of one entry: a frame whose decode at t_hi has a round that queues two CNs must re-scan
    cn_lim = p.nk if c["is_term"] else p.L * p.cns_pos
    must = [t for t in range(0, T, 4) if host_rounds(c["gadj"][t], c["keys"][t].astype(np.int64) < c["t_hi"], cn_lim, p.nk)[1] >= 2]
    monkeypatch.setenv(QCAP, "1")
    got = E.vn_threshold(*args, grid=c["grid"], is_term=c["is_term"], want_tau=True)
    synchronize()
    monkeypatch.undo()
    r = assert_equals_reference(ref, got, "queues of one entry")
    print(key, "queues of one entry | frames that must re-scan (of 64 looked at):", len(must), "| re-scans:", int(r[:, 6].sum()))
    assert len(must) >= 3 and (r[must, 6] > 0).all()


@pytest.mark.parametrize("cap", [None, 1, 3])
def test_tied_keys(E, cap, monkeypatch):
    """Integer keys in [0, 40) with the window [12, 24] (every step is a tie, on the truncated chain), all keys equal inside the
    window, and a window one threshold wide — 64 frames each, with and without a small list."""
    import torch
    c = case(E, "3-6-L10-N20-open")
    p, nt = c["p"], 64
    if cap is not None:
        monkeypatch.setenv(CCAP, str(cap))

    def run(keys, lo, hi, grid, what):
        d_keys = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).to("cuda:0")
        got = E.vn_threshold(p, c["d_adj"][:nt], d_keys, lo, hi, grid=grid, is_term=False, want_tau=True)
        synchronize()
        ref = host_reference(p, c["gadj"][:nt], keys, lo, hi, False, grid)
        return assert_equals_reference(ref, got, what), ref
    rng = np.random.RandomState(11)
    r, ref = run(rng.randint(0, 40, size=(nt, p.n)).astype(np.uint32), 12, 24, list(range(12, 25)), "keys in [0, 40)")
    assert (r[:, 4] >= 1).sum() >= 32 and max(max(x, default=0) for x in ref["releases"]) > 8
    mid = (c["t_lo"] + c["t_hi"]) // 2
    r, ref = run(np.full((nt, p.n), mid, dtype=np.uint32), c["t_lo"], c["t_hi"], [mid, mid + 1], "all keys equal")
    assert (r[:, 7] == p.n).all() and set(r[:, 1].tolist()) == {0} and (r[:, 0] == mid + 1).all() and (r[:, 4] == 1).all()
    assert (ref["counts"][:, 0] == 0).all() and (ref["counts"][:, 1] == r[:, 2]).all()
    inside = c["ref"]["tau"][:nt][(c["ref"]["tau"][:nt] > c["t_lo"]) & (c["ref"]["tau"][:nt] != NONE)]
    first = int(np.sort(inside)[inside.size // 2])                       # a threshold some VN has: the median one
    r, ref = run(c["keys"][:nt], first - 1, first, [first - 1, first], "t_hi - t_lo = 1")
    assert (r[:, 1] == 2).any() and (r[:, 4] <= 1).all()


# ---- the workspace form ---------------------------------------------------------------------------------------------------------
def test_the_workspace_form(E):
    """(4,8), L = 50 with int32 rows where the CN words go to the workspace; four frames, window [0.46, 0.48]."""
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    nt = 4
    t_lo, t_hi = E.erasure_threshold(0.46), E.erasure_threshold(0.48)
    assert E.vn_threshold_workspace_bytes(p, nt, False) == nt * 4 * p.nk > 0
    d_adj, _ch = E.sample_philox(p, SEED, 0, nt, 0.48)
    d_keys = E.channel_keys(p, SEED, 0, nt)
    synchronize()
    grid = grid_of(t_lo, t_hi, 64)
    got = E.vn_threshold(p, d_adj, d_keys, t_lo, t_hi, grid=grid, want_tau=True)
    synchronize()
    ref = host_reference(p, d_adj.cpu().numpy(), d_keys.cpu().numpy().view(np.uint32), t_lo, t_hi, True, grid)
    r = assert_equals_reference(ref, got, "workspace")
    print("workspace rows:", r.tolist())
    assert (r[:, 1] != 1).any() and r[:, 4].max() >= 100                 # something failed at 0.48, over a long walk


# ---- the driver and the command line --------------------------------------------------------------------------------------------
def test_the_thresholds_give_the_grids_curves(E):
    """One integer per VN decides every ε of the window: ber_at, block_err_at and fer_at are users_err, block_err and frame_err of
    run_grid_fused on the same 512 frames, point for point."""
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    p = E.make_params(4, 8, 12, 32)
    es = [float(e) for e in np.linspace(0.50, 0.40, 16)]
    res = BP.run_vn_thresholds(p, 0.40, 0.50, 512, seed=31, es=es, index=2, batch=200, device="cuda:0", want_tau=True)
    pts = BP.run_grid_fused(p, es, 0, 512, seed=31, index=2, batch=128, device="cuda:0")
    frames = BP.run_thresholds(p, 0.40, 0.50, 512, seed=31, index=2, batch=256, device="cuda:0")
    synchronize()
    want = {k: [pt.run[k] for pt in pts] for k in ("users_err", "block_err", "frame_err")}
    print("users_err by point:", want["users_err"], "| block_err:", want["block_err"], "| frame_err:", want["frame_err"])
    assert all(pt.f == 512 for pt in pts) and want["frame_err"][0] > want["frame_err"][-1] > 0
    assert res.ber_at(es).tolist() == want["users_err"] and res.block_err_at(es).tolist() == want["block_err"]
    assert res.fer_at(es).tolist() == want["frame_err"] == frames.fer_at(es).tolist()
    fine = np.linspace(0.40, 0.50, 200)
    assert (res.fer_at(fine) == frames.fer_at(fine)).all() and (np.diff(res.ber_at(fine)) >= 0).all()
    assert (res.bler_at(es).sum(axis=1) == want["block_err"]).all() and res.bler_at(es).shape == (16, p.L)
    assert (res.rows[:, :2] == frames.rows[:, :2]).all() and (res.rows[:, 3] == frames.rows[:, 2]).all()
    star = res.pos_eps_star()
    assert star.shape == (512, p.L) and np.isfinite(star).sum() >= 500 and np.nanmin(star) > 0.40 and np.nanmax(star) <= 0.5000001
    # the batch size changes nothing, and without tau the grid's points are still there
    again = BP.run_vn_thresholds(p, 0.40, 0.50, 512, seed=31, es=es, index=2, batch=512, device="cuda:0")
    assert again.tau is None and (again.rows[:, COLS] == res.rows[:, COLS]).all() and (again.pos_thresh == res.pos_thresh).all()
    assert (again.counts == res.counts).all() and again.ber_at(es).tolist() == want["users_err"]


CLI = ["0", "0", "0", "300", "--N", "16", "--L", "12", "--batch", "128", "--eps-lo", "0.40", "--eps-hi", "0.50", "--points", "9"]


def test_the_command_line_writes_what_run_vn_thresholds_returns(E, tmp_path, capsys):
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    assert BP.bp_curves(CLI + ["--seed", "4242", "--outdir", str(tmp_path)]) == 0
    synchronize()
    text = capsys.readouterr().out
    p = E.make_params(4, 8, 12, 16)
    name = BP.result_filename("bp_lim_iter", p, 0, 1000000, 0, 0) + ".curves.pkl"
    assert os.listdir(str(tmp_path)) == [name]
    pkl = pickle.load(open(os.path.join(str(tmp_path), name), "rb"))
    assert sorted(pkl) == sorted(["eps_lo", "eps_hi", "t_lo", "t_hi", "seed", "index", "es", "rows", "pos_thresh", "counts"])
    es = pkl["es"]
    assert (pkl["eps_lo"], pkl["eps_hi"], pkl["seed"], pkl["index"]) == (0.40, 0.50, 4242, 0) and len(es) == 9
    res = BP.run_vn_thresholds(p, 0.40, 0.50, 300, seed=4242, es=es, index=0, batch=77, device="cuda:0")
    synchronize()
    assert (pkl["rows"][:, COLS] == res.rows[:, COLS]).all() and (pkl["pos_thresh"] == res.pos_thresh).all()
    assert (pkl["counts"] == res.counts).all() and pkl["counts"].shape == (300, 9)
    lines = text.splitlines()
    assert lines[0] + "\n" == BP.RISULTATI_HEADER and len(lines) == 10
    for line, e, u, f, b in zip(lines[1:], es, res.ber_at(es), res.fer_at(es), res.block_err_at(es)):
        w = line.split()
        assert float(w[0]) == pytest.approx(e, abs=1e-6) and [int(x) for x in w[7:13]] == [p.n, p.L, 300, u, f, b]
    assert BP.bp_curves(CLI + ["--seed", "4242", "--quiet", "--outdir", str(tmp_path)]) == 0
    assert capsys.readouterr().out == ""


def test_two_ranks_write_the_single_rank_file(tmp_path):
    require_gpu()
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir(); d2.mkdir()
    args = ["bp_curves", *CLI, "--seed", "4242", "--quiet"]
    _run(1, "fl_scaling_sc_ldpc_amd.bp_decoding", [*args, "--outdir", str(d1)])
    _run(2, "fl_scaling_sc_ldpc_amd.bp_decoding", [*args, "--outdir", str(d2)])
    _same_files(str(d1), str(d2), 1)
