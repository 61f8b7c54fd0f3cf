"""Exact per-frame erasure thresholds on a real device (-m gpu): engine.channel_keys against the sampler's channel words,
engine.frame_threshold against a numpy bisection over the downloaded rows and keys (tests/test_thresh_host.host_bisect) and
against engine.full_bp (max_it = 0) with every frame at its own threshold, the condition that makes those comparisons mean
something, arbitrary keys, the overflow re-scan in a stage after the first, the workspace form, a batch split in two, and
run_thresholds / bp_thresholds against run_grid_fused on the same frames, single rank and two ranks.  Every reference is
computed once per shape and shared (tests/test_gpu_buffer_contracts_thresh.py imports it)."""
import os
import pickle

import numpy as np
import pytest

from conftest import require_gpu
from test_eps_host import ES, QCAP, WORKSPACE_M
from test_gpu_bp_eps import SEED, SHAPES, host_rounds
from test_gpu_cli_ranks import _run, _same_files
from test_thresh_host import host_bisect, host_fixpoint

pytestmark = pytest.mark.gpu
T = 256
TRIAL0 = 7
KEYS = ["4-8-L12-N16", "4-8-L12-N16-int32", "3-6-L10-N20", "3-6-L10-N20-open", "5-10-L10-N20", "3-6-L11-N18", "4-8-L12-N64-doped3"]
CONDITION = ["4-8-L12-N16", "3-6-L10-N20", "5-10-L10-N20"]              # the terminated Olmos shapes at [0.40, 0.50]
COLS = [0, 1, 2, 3, 4, 7]                                               # every column but the two diagnostics


def window(key):
    return (0.20, 0.40) if key.endswith("-open") else (0.40, 0.50)


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the frame-threshold tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def global_adj(E, p, adj):
    return E.adj16_to_global(p, adj) if adj.dtype == np.int16 else adj


def host_rows(p, adj, keys, t_lo, t_hi, is_term):
    """host_bisect frame by frame: rows int64 [T, 6] (COLS) and the critical residuals as words."""
    cn_lim = p.nk if is_term else p.L * p.cns_pos
    rows, bits = [], []
    for t in range(adj.shape[0]):
        row, R = host_bisect(adj[t], keys[t], t_lo, t_hi, cn_lim, p.nk, p.vns_pos)
        rows.append(row)
        bits.append(R)
    from fl_scaling_sc_ldpc_amd import engine
    return np.array(rows, dtype=np.int64), engine.pack_bits(np.array(bits, dtype=np.uint8))


_CACHE = {}


def case(E, key):
    """The code of a shape, its keys, and the host bisection of every frame: computed once."""
    if key in _CACHE:
        return _CACHE[key]
    dv, dc, L, N, is_term, a16, doped, _ = SHAPES[key]
    p = E.make_params(dv, dc, L, N)
    e_lo, e_hi = window(key)
    t_lo, t_hi = E.erasure_threshold(e_lo), E.erasure_threshold(e_hi)
    d_adj, _ch = E.sample_philox(p, SEED, TRIAL0, T, e_hi, doped, adj16=a16)
    d_keys = E.channel_keys(p, SEED, TRIAL0, T, doped)
    synchronize()
    adj, keys = d_adj.cpu().numpy().copy(), d_keys.cpu().numpy().view(np.uint32).copy()
    rows, bits = host_rows(p, global_adj(E, p, adj), keys, t_lo, t_hi, is_term)
    c = dict(p=p, is_term=is_term, doped=doped, t_lo=t_lo, t_hi=t_hi, d_adj=d_adj, d_keys=d_keys, adj=adj, keys=keys, rows=rows,
             bits=bits)
    _CACHE[key] = c
    return c


def assert_equals_host(c, got, what, rows=None, bits=None):
    want_rows = c["rows"] if rows is None else rows
    want_bits = c["bits"] if bits is None else bits
    r = got["rows"].cpu().numpy().astype(np.int64)
    assert r.shape == (want_rows.shape[0], 8)
    for i, col in enumerate(COLS):
        bad = np.flatnonzero(r[:, col] != want_rows[:, i])
        assert bad.size == 0, (what, "column", col, "frame", int(bad[0]), r[bad[0]].tolist(), want_rows[bad[0]].tolist())
    assert (r[:, 5] >= 1).all() and (r[:, 5] <= 33).all() and (r[:, 6] >= 0).all(), (what, r[:, 5].min(), r[:, 5].max())
    if got["bits"] is not None:
        b = got["bits"].cpu().numpy().view(np.uint32)
        assert b.shape == want_bits.shape and (b == want_bits).all(), (what, "bits")
    return r


# ---- the keys ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["4-8-L12-N16", "3-6-L11-N18"])
@pytest.mark.parametrize("doped", [(), (3,)], ids=["plain", "doped3"])
def test_the_keys_are_the_samplers_channel_at_every_eps(E, key, doped):
    """n = 192 (16-byte stores) and n = 198 (scalar stores, a partial last word): pack(keys < erasure_threshold(e)) is the
    channel sample_philox writes at e, with and without a doped position; doped VNs hold 0xFFFFFFFF."""
    import torch
    dv, dc, L, N = SHAPES[key][:4]
    p = E.make_params(dv, dc, L, N)
    assert (p.n % 4 == 0) == (key == "4-8-L12-N16")
    d_keys = E.channel_keys(p, SEED, TRIAL0, T, doped)
    # the same keys through the scalar stores: a row base that is not 16-byte aligned
    buf = torch.full((T * p.n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    shifted = E.channel_keys(p, SEED, TRIAL0, T, doped, out=buf[1:1 + T * p.n].view(T, p.n))
    synchronize()
    keys = d_keys.cpu().numpy().view(np.uint32)
    assert (shifted.cpu().numpy().view(np.uint32) == keys).all()
    assert buf[0].item() == 0x5A5A5A5A and (buf[1 + T * p.n:] == 0x5A5A5A5A).all()
    is_doped = np.zeros(p.n, dtype=bool)
    for d in doped:
        is_doped[d * p.vns_pos:(d + 1) * p.vns_pos] = True
    assert (keys[:, is_doped] == 0xFFFFFFFF).all() and (keys[:, ~is_doped] < (1 << 31)).all()
    for e in ES:
        _adj, d_ch = E.sample_philox(p, SEED, TRIAL0, T, e, doped, adj16=True)
        synchronize()
        assert (E.pack_bits(keys < E.erasure_threshold(e)) == d_ch.cpu().numpy().view(np.uint32)).all(), e
    # a batch keyed later is the tail of this one
    tail = E.channel_keys(p, SEED, TRIAL0 + 100, T - 100, doped)
    synchronize()
    assert (tail.cpu().numpy().view(np.uint32) == keys[100:]).all()


# ---- the decoder against the host bisection -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_the_decoder_equals_the_host_bisection(E, key):
    import torch
    c = case(E, key)
    p = c["p"]
    got = E.frame_threshold(p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"], is_term=c["is_term"], want_bits=True)
    synchronize()
    r = assert_equals_host(c, got, key)
    status = r[:, 1]
    print(key, "status 0 / 1 / 2:", [int((status == s).sum()) for s in (0, 1, 2)], "| stages mean %.1f max %d" % (r[:, 5].mean(), r[:, 5].max()),
          "| sizes of the critical residuals:", sorted(set(r[status == 0, 2].tolist()))[:6], "…")
    assert c["d_adj"].dtype == (torch.int16 if SHAPES[key][5] else torch.int32)
    if key == "3-6-L11-N18":
        assert p.n == 198 and p.n % 32                                   # the last word is partial
    bare = E.frame_threshold(p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"], is_term=c["is_term"])
    synchronize()
    assert bare["bits"] is None and (bare["rows"][:, COLS] == got["rows"][:, COLS]).all()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_keys"].cpu().numpy().view(np.uint32) == c["keys"]).all()


@pytest.mark.parametrize("key", KEYS)
def test_the_decoder_against_full_bp_at_each_frames_own_threshold(E, key):
    """full_bp without a cap, the kernel everything here is specified against: on {key < T*} it leaves exactly the critical
    residual, on {key < T* - 1} nothing; a status-1 frame decodes at t_hi; a status-2 frame keeps d_bits at t_lo."""
    import torch
    c = case(E, key)
    p = c["p"]
    got = E.frame_threshold(p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"], is_term=c["is_term"], want_bits=True)
    synchronize()
    r, bits = got["rows"].cpu().numpy().astype(np.int64), got["bits"].cpu().numpy().view(np.uint32)
    status = r[:, 1]
    at = np.where(status == 0, r[:, 0], np.where(status == 1, c["t_hi"], c["t_lo"]))
    below = np.where(status == 0, r[:, 0] - 1, 0)
    keys = c["keys"].astype(np.int64)

    def full_bp_at(thr):
        ch = E.pack_bits(keys < thr[:, None])
        d_ch = torch.from_numpy(ch.view(np.int32)).to("cuda:0")
        out = E.full_bp(p, c["d_adj"], d_ch, max_it=0, is_term=c["is_term"], want_erased=True)
        synchronize()
        return out["counters"].cpu().numpy(), out["erased"].cpu().numpy().view(np.uint32)
    cnt, erased = full_bp_at(at)
    assert (erased == bits).all()
    assert ((cnt[:, 0] == 0) == (status == 1)).all() and (cnt[:, 0] == r[:, 2]).all()
    assert (cnt[:, 7] == (keys < at[:, None]).sum(axis=1)).all()
    cnt_below, _ = full_bp_at(below)
    assert (cnt_below[status == 0, 0] == 0).all()


@pytest.mark.parametrize("key", CONDITION)
def test_the_inputs_exercise_every_branch(E, key):
    """Read off the host bisection alone: frames that decode at the top of the window, frames that fail at its bottom, and at
    least 100 thresholds inside; over the three shapes together, a critical residual of exactly two VNs."""
    c = case(E, key)
    status, size = c["rows"][:, 1], c["rows"][:, 2]
    counts = [int((status == s).sum()) for s in (0, 1, 2)]
    print(key, "status 0 / 1 / 2:", counts, "| smallest critical residual:", int(size[status == 0].min()))
    assert counts[1] >= 2 and counts[2] >= 2 and counts[0] >= 100
    if key == CONDITION[-1]:
        smallest = min(int(case(E, k)["rows"][case(E, k)["rows"][:, 1] == 0, 2].min()) for k in CONDITION)
        assert smallest == 2


# ---- arbitrary keys ----------------------------------------------------------------------------------------------------------
def test_arbitrary_keys(E):
    """Any uint32 keys are valid input, and so is any window: all keys equal inside the window, all at or above t_hi, all below
    t_lo, t_lo = 0, and a window one threshold wide.  64 frames each, against the host bisection."""
    import torch
    c = case(E, "4-8-L12-N16")
    p, nt = c["p"], 64
    adj = global_adj(E, p, c["adj"][:nt])
    t_lo, t_hi = c["t_lo"], c["t_hi"]

    def run(keys, lo, hi, what):
        d_keys = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).to("cuda:0")
        got = E.frame_threshold(p, c["d_adj"][:nt], d_keys, lo, hi, want_bits=True)
        synchronize()
        rows, bits = host_rows(p, adj, keys, lo, hi, True)
        return assert_equals_host(c, got, what, rows, bits)
    mid = (t_lo + t_hi) // 2
    r = run(np.full((nt, p.n), mid, dtype=np.uint32), t_lo, t_hi, "all keys equal")
    assert (r[:, 7] == p.n).all() and set(r[:, 1].tolist()) <= {0, 1}
    assert ((r[:, 1] == 0) <= (r[:, 0] == mid + 1)).all()                # whoever fails, fails where the keys are
    r = run(np.full((nt, p.n), t_hi, dtype=np.uint32) + (np.arange(p.n, dtype=np.uint32) % 3) * 0x40000000, t_lo, t_hi, "all keys >= t_hi")
    assert (r[:, 1] == 1).all() and (r[:, 7] == 0).all() and (r[:, 0] == -1).all() and (r[:, 5] == 1).all()
    low = c["keys"][:nt] % np.uint32(t_lo)
    r = run(low, t_lo, t_hi, "all keys < t_lo")
    full = [host_fixpoint(adj[t], np.ones(p.n, dtype=bool), p.nk, p.nk) for t in range(nt)]
    assert (r[:, 7] == p.n).all() and (r[:, 2] == [int(f.sum()) for f in full]).all()    # the full decode's residual
    assert ((r[:, 1] == 2) == (r[:, 2] > 0)).all() and ((r[:, 1] == 1) == (r[:, 2] == 0)).all()
    r = run(c["keys"][:nt], 0, t_hi, "t_lo = 0")
    assert (r[:, 1] != 2).all() and (r[:, 1] == 0).sum() >= 10
    inside = c["rows"][:nt][c["rows"][:nt, 1] == 0, 0]
    first = int(np.sort(inside)[inside.size // 2])                       # a threshold that is some frame's T*: the median one
    r = run(c["keys"][:nt], first - 1, first, "t_hi - t_lo = 1")
    assert (r[:, 1] == 0).sum() >= 1 and (r[r[:, 1] == 0, 0] == first).all() and (r[:, 1] == 1).any() and (r[:, 1] == 2).any()


def test_skipped_stages_with_many_waves_forming_u(E):
    """Keys in a narrow band just below t_hi: the bisection's first twenty or so mids lie below every key of R, so stage after
    stage is skipped (U empty before any peeling) back to back, at a shape where six waves form U (nw = 384) — the stretch in
    which the per-stage scalars are cleared with no barrier of a build or a peel in between.  16 frames, against the host."""
    import torch
    p = E.make_params(4, 8, 12, 1024)
    nt = 16
    assert p.nw == 384
    t_lo, t_hi = E.erasure_threshold(0.40), E.erasure_threshold(0.50)
    d_adj, _ch = E.sample_philox(p, SEED, TRIAL0, nt, 0.5, adj16=True)
    rng = np.random.RandomState(5)
    keys = (t_hi - 1 - rng.randint(0, 1000, size=(nt, p.n))).astype(np.uint32)
    d_keys = torch.from_numpy(keys.view(np.int32)).to("cuda:0")
    got = E.frame_threshold(p, d_adj, d_keys, t_lo, t_hi, want_bits=True)
    synchronize()
    rows, bits = host_rows(p, global_adj(E, p, d_adj.cpu().numpy()), keys, t_lo, t_hi, True)
    r = assert_equals_host(None, got, "a band of keys below t_hi", rows, bits)
    print("status:", r[:, 1].tolist(), "stages:", r[:, 5].tolist())
    assert (r[:, 7] == p.n).all() and (r[:, 1] == 0).all() and (r[:, 0] > t_hi - 1001).all() and (r[:, 5] >= 20).all()


# ---- the overflow re-scan -------------------------------------------------------------------------------------------------------
def test_the_overflow_rescan_in_a_later_stage(E, monkeypatch):
    """Queues of one entry overflow wherever a round queues two CNs, also in the stages after the first, and the rows and bits are
    unchanged; only the diagnostics may differ.  That a stage after the first does overflow is read off the host rounds: stage 1
    peels R ∩ {key < t_lo}, R the host's residual at t_hi."""
    key = "4-8-L12-N16"
    c = case(E, key)
    p = c["p"]
    adj = global_adj(E, p, c["adj"])
    late = 0
    for t in range(T):
        keys = c["keys"][t].astype(np.int64)
        R = host_fixpoint(adj[t], keys < c["t_hi"], p.nk, p.nk)
        U = R & (keys < c["t_lo"])
        if U.any():
            _, most = host_rounds(adj[t], U, p.nk, p.nk)
            late += most >= 2
    print("frames whose stage 1 has a round that queues two or more CNs:", late)
    assert late >= 3
    args = (p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"])
    monkeypatch.delenv(QCAP, raising=False)
    free = E.frame_threshold(*args, want_bits=True)
    monkeypatch.setenv(QCAP, "1")
    capped = E.frame_threshold(*args, want_bits=True)
    synchronize()
    monkeypatch.undo()
    a = assert_equals_host(c, free, "no cap")
    b = assert_equals_host(c, capped, "queues of one entry")
    print("re-scans:", int(b[:, 6].sum()), "without the cap:", int(a[:, 6].sum()))
    assert (a[:, 6] == 0).all() and (b[:, 6] > 0).any() and (b[:, 6] > 0).sum() >= late


# ---- the workspace form -----------------------------------------------------------------------------------------------------
def workspace_case(E):
    """(4,8), L = 50 with int32 rows where the CN words go to the workspace; four frames, window [0.44, 0.48]."""
    if "workspace" in _CACHE:
        return _CACHE["workspace"]
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    nt = 4
    t_lo, t_hi = E.erasure_threshold(0.44), E.erasure_threshold(0.48)
    d_adj, _ch = E.sample_philox(p, SEED, 0, nt, 0.48)
    d_keys = E.channel_keys(p, SEED, 0, nt)
    synchronize()
    adj, keys = d_adj.cpu().numpy().copy(), d_keys.cpu().numpy().view(np.uint32).copy()
    rows, bits = host_rows(p, adj, keys, t_lo, t_hi, True)
    c = dict(p=p, is_term=True, doped=(), t_lo=t_lo, t_hi=t_hi, d_adj=d_adj, d_keys=d_keys, adj=adj, keys=keys, rows=rows, bits=bits)
    _CACHE["workspace"] = c
    return c


def test_the_workspace_form(E):
    c = workspace_case(E)
    p = c["p"]
    assert E.frame_threshold_workspace_bytes(p, 4, False) == 4 * 4 * p.nk > 0
    got = E.frame_threshold(p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"], want_bits=True)
    synchronize()
    r = assert_equals_host(c, got, "workspace")
    print("workspace rows:", r.tolist())
    assert (r[:, 1] != 1).any()                                          # something failed at 0.48


# ---- batches and views ----------------------------------------------------------------------------------------------------------
def test_a_batch_split_in_two_and_rows_views(E):
    import torch
    c = case(E, "5-10-L10-N20")
    p = c["p"]
    T1 = T // 3 + 1
    args = (c["t_lo"], c["t_hi"])
    buf = torch.full((T * 8 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    one = E.frame_threshold(p, c["d_adj"], c["d_keys"], *args, want_bits=True, rows=buf[:T * 8].view(T, 8))
    first = E.frame_threshold(p, c["d_adj"][:T1], c["d_keys"][:T1], *args, want_bits=True)
    second = E.frame_threshold(p, c["d_adj"][T1:], c["d_keys"][T1:], *args, want_bits=True)
    synchronize()
    assert one["rows"].data_ptr() == buf.data_ptr() and (buf[T * 8:] == 0x5A5A5A5A).all()
    assert_equals_host(c, one, "one call into a view")
    two = {"rows": torch.cat([first["rows"], second["rows"]]), "bits": torch.cat([first["bits"], second["bits"]])}
    assert_equals_host(c, two, "two calls")
    assert (two["rows"][:, COLS] == one["rows"][:, COLS]).all()
    with pytest.raises(AssertionError):
        E.frame_threshold(p, c["d_adj"], c["d_keys"], *args, rows=buf[:T * 8].view(8, T))


# ---- the driver and the command line ----------------------------------------------------------------------------------------
def test_the_thresholds_give_the_grids_frame_errors(E):
    """One integer per frame decides every ε of the window: fer_at(es) is frame_err of run_grid_fused on the same 512 frames."""
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    p = E.make_params(4, 8, 12, 16)
    es = [float(e) for e in np.linspace(0.50, 0.40, 16)]
    assert es[0] == 0.50 and es[-1] == 0.40
    res = BP.run_thresholds(p, 0.40, 0.50, 512, seed=31, index=2, batch=200, device="cuda:0", want_bits=True)
    pts = BP.run_grid_fused(p, es, 0, 512, seed=31, index=2, batch=128, device="cuda:0")
    synchronize()
    want = [pt.run["frame_err"] for pt in pts]
    got = res.fer_at(es).tolist()
    print("frame errors by point:", want)
    assert all(pt.f == 512 for pt in pts) and got == want and want[0] > want[-1] > 0 and len(set(want)) >= 8
    assert res.rows.shape == (512, 8) and res.bits.shape == (512, p.nw)
    star = res.eps_star()
    inside = res.rows[:, 1] == 0
    assert inside.sum() >= 200 and np.isnan(star[~inside]).all() and ((star[inside] > 0.40) & (star[inside] <= 0.5000001)).all()
    # a finer grid than any the grid decoders take: 200 points, no two of one threshold, from the same rows
    fine = res.fer_at(np.linspace(0.40, 0.50, 200))
    assert (np.diff(fine) >= 0).all() and fine[0] == want[-1] and fine[-1] == want[0]
    # the batch size changes nothing
    again = BP.run_thresholds(p, 0.40, 0.50, 512, seed=31, index=2, batch=512, device="cuda:0")
    assert (again.rows[:, COLS] == res.rows[:, COLS]).all() and again.bits is None


CLI = ["0", "0", "0", "300", "--N", "16", "--L", "12", "--batch", "128"]


def test_the_command_line_writes_the_rows_of_run_thresholds(E, tmp_path, capsys):
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    assert BP.bp_thresholds(CLI + ["--seed", "4242", "--outdir", str(tmp_path)]) == 0
    synchronize()
    text = capsys.readouterr().out
    p = E.make_params(4, 8, 12, 16)
    name = BP.result_filename("bp_lim_iter", p, 0, 1000000, 0, 0) + ".thresholds.pkl"
    assert os.listdir(str(tmp_path)) == [name]
    pkl = pickle.load(open(os.path.join(str(tmp_path), name), "rb"))
    g = BP.DEFAULTS["bp_lim_iter"]["grid"]
    e_lo, e_hi = g.eps(g.num_points - 1), g.eps(0)
    assert sorted(pkl) == sorted(["eps_lo", "eps_hi", "t_lo", "t_hi", "seed", "index", "rows"])
    assert (pkl["eps_lo"], pkl["eps_hi"], pkl["seed"], pkl["index"]) == (e_lo, e_hi, 4242, 0)
    assert (pkl["t_lo"], pkl["t_hi"]) == (E.erasure_threshold(e_lo), E.erasure_threshold(e_hi))
    res = BP.run_thresholds(p, e_lo, e_hi, 300, seed=4242, index=0, batch=77, device="cuda:0")
    synchronize()
    assert pkl["rows"].dtype == np.int64 and pkl["rows"].shape == (300, 8) and (pkl["rows"][:, COLS] == res.rows[:, COLS]).all()
    assert "frames 300" in text and "eps*: mean" in text
    assert BP.bp_thresholds(CLI + ["--seed", "4242", "--quiet", "--outdir", str(tmp_path)]) == 0
    assert capsys.readouterr().out == ""


def test_two_ranks_write_the_single_rank_file(tmp_path):
    require_gpu()
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir(); d2.mkdir()
    args = ["bp_thresholds", *CLI, "--seed", "4242", "--quiet"]
    _run(1, "fl_scaling_sc_ldpc_amd.bp_decoding", [*args, "--outdir", str(d1)])
    _run(2, "fl_scaling_sc_ldpc_amd.bp_decoding", [*args, "--outdir", str(d2)])
    _same_files(str(d1), str(d2), 1)
