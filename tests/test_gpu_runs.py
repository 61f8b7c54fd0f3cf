"""Error-propagation statistics on the GPU (-m gpu): scldpc_chain_runs_device and scldpc_stream_runs_device (err_runs.hip)
against the numpy references of tests/test_runs_host.py, on synthetic inputs and behind the decoders.  Every comparison is exact
integer equality.  The conditions the inputs were chosen for are asserted on the reference alone, before any comparison; the
code under test never is a reference."""
import os
import pickle

import numpy as np
import pytest

from conftest import require_gpu
from test_runs_host import (SYNTH_CHAIN, check_synthetic_chain, np_chain_runs, np_stream_runs, synthetic_chain_bits,
                            synthetic_stream_rows)

pytestmark = pytest.mark.gpu
NAMES = ("pos", "run_hist", "fail_hist")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def params(E, L, V):
    return E.CodeParams(1, 1, L, V, V)                                   # any V: dv * vns_pos == dc * cns_pos


def upload_bits(E, bits, nw=None):
    import torch
    words = E.pack_bits(np.asarray(bits, dtype=np.uint8))
    assert nw is None or words.shape[1] == nw
    return torch.from_numpy(words.view(np.int32)).cuda()


def run_chain(E, p, d_bits, acc=None, **kw):
    import torch
    res = E.chain_runs(p, d_bits, acc=acc, want_trial=True, want_fail_bits=True, **kw)
    torch.cuda.synchronize()
    return res


def same_chain(what, res, want):
    acc, trial, fail_bits = want
    for name in NAMES:
        g = res[name].cpu().numpy()
        assert g.dtype == np.int64 and g.shape == acc[name].shape and (g == acc[name]).all(), (what, name, np.argwhere(g != acc[name])[:4].tolist())
    if trial is not None:
        g = res["trial"].cpu().numpy()
        assert (g == trial).all(), (what, "trial", np.argwhere(g != trial)[:4].tolist())
        g = res["fail_bits"].cpu().numpy().view(np.uint32)
        assert g.shape == fail_bits.shape and (g == fail_bits).all(), (what, "fail_bits")


_chain_refs = {}


def chain_case(key):
    """bits and the reference's answer for one synthetic shape, computed once and left unchanged."""
    if key not in _chain_refs:
        L, V, T, q, rho = key
        bits = synthetic_chain_bits(L, V, T, q, rho)
        _chain_refs[key] = (bits, np_chain_runs(bits, L, V))
    return _chain_refs[key]


# ---- 1. chain, synthetic bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SYNTH_CHAIN), ids=lambda k: "L%d-V%d" % k[:2])
def test_chain_synthetic_bits(E, key):
    L, V, T, q, rho = key
    bits, want = chain_case(key)
    check_synthetic_chain(want[0], want[1], SYNTH_CHAIN[key])             # the inputs are what the shapes were chosen for
    p = params(E, L, V)
    same_chain(key, run_chain(E, p, upload_bits(E, bits, p.nw)), want)


def test_chain_of_one_position_and_the_constant_rows(E):
    rs = np.random.RandomState(7)
    for V in (2, 64, 100):
        bits = (rs.rand(9, V) < 0.02).astype(np.uint8)
        bits[0] = 0
        bits[1] = 1
        want = np_chain_runs(bits, 1, V)
        assert want[0]["run_hist"].tolist()[1] == [want[0]["fail_hist"][1]] * 2 and want[0]["fail_hist"][0] >= 1
        same_chain(("L=1", V), run_chain(E, params(E, 1, V), upload_bits(E, bits)), want)
    for L, V in ((12, 20), (70, 34), (64, 32), (128, 2)):
        bits = np.zeros((3, L * V), np.uint8)
        bits[1] = 1
        want = np_chain_runs(bits, L, V)
        assert want[1].tolist() == [[0, L, 0, 0], [L, 0, 1, L], [0, L, 0, 0]]
        assert want[0]["run_hist"][L].tolist() == [1, 1] and want[0]["run_hist"][0, 0] == 2      # one run of L that reaches the end
        same_chain(("constant", L, V), run_chain(E, params(E, L, V), upload_bits(E, bits)), want)


def test_chain_ignores_garbage_beyond_n(E):
    import torch
    key = (12, 20, 64, .35, .2)                                          # n = 240: 16 padding bits in the last word
    bits, want = chain_case(key)
    p = params(E, 12, 20)
    d = upload_bits(E, bits, p.nw)
    d[:, -1] |= torch.tensor(np.array([0xFFFF0000], np.uint32).view(np.int32)[0], device="cuda")
    same_chain("garbage beyond n", run_chain(E, p, d), want)


def test_chain_more_trials_than_workgroups_accumulation_and_splits(E):
    L, V = 12, 20
    p = params(E, L, V)
    rs = np.random.RandomState(99)
    g = rs.rand(3000, L) < .35
    big = ((rs.rand(3000, L, V) < .2) & g[:, :, None]).reshape(3000, L * V)
    want = np_chain_runs(big, L, V)
    assert want[0]["run_hist"][1:, 0].sum() > 3000 and want[0]["run_hist"][0, 0] > 0
    d_big = upload_bits(E, big, p.nw)
    res = run_chain(E, p, d_big)
    same_chain("3000 trials", res, want)
    again = run_chain(E, p, d_big, acc={k: res[k] for k in NAMES})       # a second call doubles the sums
    same_chain("twice", again, ({k: 2 * v for k, v in want[0].items()}, want[1], want[2]))
    bits, want64 = chain_case((L, V, 64, .35, .2))
    d = upload_bits(E, bits, p.nw)
    for cut in (1, 17):
        a = run_chain(E, p, d[:cut].contiguous())
        b = run_chain(E, p, d[cut:].contiguous(), acc={k: a[k] for k in NAMES})
        same_chain(("split", cut), b, (want64[0], None, None))
        assert (np.concatenate([a["trial"].cpu().numpy(), b["trial"].cpu().numpy()]) == want64[1]).all()
        assert (np.concatenate([a["fail_bits"].cpu().numpy(), b["fail_bits"].cpu().numpy()]).view(np.uint32) == want64[2]).all()


# ---- 2. chain, behind the decoders ------------------------------------------------------------------------------------------
_graphs = {}


def decoder_inputs(E, oracle, eps):
    """(4,8), L = 12, N = 100, seed 11, trials 0 .. 31 from the CPU twin of the sampler, uploaded."""
    import torch
    from test_gpu_ss import to_adj16
    if eps not in _graphs:
        p = E.make_params(4, 8, 12, 100)
        po = oracle.Params(4, 8, 12, p.cns_pos, p.vns_pos)
        pairs = [oracle.sample_philox(po, 11, t, eps) for t in range(32)]
        adj = np.stack([a for a, _ in pairs])
        ch = np.stack([np.asarray(c).view(np.uint32) for _, c in pairs])
        _graphs[eps] = (p, adj, to_adj16(p, adj), ch)
    p, adj, adj16, ch = _graphs[eps]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return p, up(adj), up(adj16), up(ch.view(np.int32))


FORMS = ("square", "square-ring", "classical", "classical-ring", "full")


def decode(E, form, p, d_adj, d_adj16, d_ch):
    if form == "square":
        return E.sw_bp(p, d_adj, d_ch, 4, 4, 4, want_erased=True, ring=False)
    if form == "square-ring":
        return E.sw_bp(p, d_adj16, d_ch, 4, 4, 4, want_erased=True, ring=True)
    if form == "classical":
        return E.sw_bp(p, d_adj, d_ch, 4, 4, want_erased=True, classical=True, ring=False)
    if form == "classical-ring":
        return E.sw_bp(p, d_adj16, d_ch, 4, 4, want_erased=True, classical=True, ring=True)
    return E.full_bp(p, d_adj, d_ch, max_it=4, want_erased=True)


@pytest.mark.parametrize("eps", [0.36, 0.40])
@pytest.mark.parametrize("form", FORMS)
def test_chain_behind_the_decoders(E, oracle, form, eps):
    import torch
    p, d_adj, d_adj16, d_ch = decoder_inputs(E, oracle, eps)
    out = decode(E, form, p, d_adj, d_adj16, d_ch)
    res = run_chain(E, p, out["erased"])
    torch.cuda.synchronize()
    bits = E.unpack_bits(out["erased"].cpu().numpy(), p.n)
    want = np_chain_runs(bits, p.L, p.vns_pos)
    acc, trial, _ = want
    if form.startswith("square") and eps == 0.36:                        # conditions on the inputs (what the oracle's decoder gives there)
        assert acc["run_hist"][0, 0] >= 5 and (trial[:, 2] >= 2).sum() >= 5 and np.count_nonzero(acc["run_hist"][1:, 0]) >= 5
        assert trial[:, 3].max() >= 5
    if form.startswith("square") and eps == 0.40:
        assert acc["run_hist"][:, 1].sum() >= 5 and acc["run_hist"][12, 1] >= 5
    same_chain((form, eps), res, want)
    cnt = out["counters"].cpu().numpy()
    got = {k: res[k].cpu().numpy() for k in NAMES}
    assert got["pos"][:, 1].sum() == cnt[:, 0].sum() and got["pos"][:, 0].sum() == cnt[:, 1].sum()
    assert got["run_hist"][0, 0] == (cnt[:, 0] == 0).sum()


# ---- 3. stream, synthetic rows ----------------------------------------------------------------------------------------------
def state_of(sr):
    import torch
    torch.cuda.synchronize()
    return [sr.hist.cpu().numpy().tolist(), sr.sums.cpu().numpy().tolist(), sr.phase.cpu().numpy().tolist(), sr.carry.cpu().numpy().tolist()]


_stream_ref = {}


def stream_case(nbins):
    if nbins not in _stream_ref:
        rows = synthetic_stream_rows()
        _stream_ref[nbins] = (rows, np_stream_runs(8, 4, (8, 9), nbins).feed(rows))
    return _stream_ref[nbins]


def test_stream_synthetic_rows_in_four_splits(E):
    import torch
    rows, ref = stream_case(32)
    assert ref.sums.tolist() == [3976, 462, 14279, 167, 462, 160, 462, 3133]
    assert ref.hist[0][:9].tolist() == [0, 58, 37, 25, 15, 10, 14, 3, 5]
    assert ref.hist[1][10] > 0 and ref.hist[1][13] > 0 and ref.hist[0][10] == 0 == ref.hist[0][13] and not ref.open_hist()[0].any()
    p = E.make_params(4, 8, 20, 64)
    d_rows = torch.from_numpy(rows).cuda()
    for chunk in (64, 7, 500, 1):
        sr = E.StreamRuns(p, 8, doped=(8, 9), nbins=32)
        for k in range(0, 500, chunk):
            sr.update(d_rows[:, k:k + chunk].contiguous())
        assert state_of(sr) == ref.state(), chunk
        assert (sr.open_hist().cpu().numpy() == ref.open_hist()).all()
    assert (d_rows.cpu().numpy() == rows).all()


def test_stream_marked_unusable_is_skipped_and_two_bins_clamp(E):
    import torch
    rows, _ = stream_case(32)
    p = E.make_params(4, 8, 20, 64)
    bad = rows.copy()
    bad[3] = -0x0BADBEEF                                                 # what the streaming kernels leave unwritten
    bad[5, :, :2] = np.array([0x7FFFFFFF, 0x7FFFFFFF], np.int32)
    counters = np.zeros((8, 10), np.int64)
    counters[3, 9] = counters[5, 9] = -1
    ref = np_stream_runs(8, 4, (8, 9), 2)
    ref.carry[3] = (41, 2, 5, 0, 17, 0, 0, 0)                            # the carry such a stream keeps
    keep = ref.carry[3].copy()
    sr = E.StreamRuns(p, 8, doped=(8, 9), nbins=2)
    sr.carry.copy_(torch.from_numpy(ref.carry))
    d_cnt = torch.from_numpy(counters).cuda()
    for k in range(0, 500, 100):
        ref.feed(bad[:, k:k + 100], skip=(3, 5))
        sr.update(torch.from_numpy(bad[:, k:k + 100].copy()).cuda(), d_cnt)
    assert (ref.carry[3] == keep).all() and not ref.carry[5].any() and not ref.hist[:, 0][:3].any() and ref.hist[:, 1].all()
    assert state_of(sr) == ref.state()
    # garbage rows in a stream that is NOT marked: clamped, never an index (the sums are the reference's on the same garbage)
    wild = rows[:2].copy()
    wild[1, 100:110, 0] = np.array([0x7FFFFFFF, -0x80000000, -1, 2, 0x7FFFFFF0, 5, 5, 5, 3, 1 << 30], np.int32)
    wild[1, 100:110, 1] = np.array([0x7FFFFFFF, 7, 7, -5, 1, 0, 9, 0, 1, 1], np.int32)
    ref = np_stream_runs(2, 4, (8, 9), 32).feed(wild)
    sr = E.StreamRuns(p, 2, doped=(8, 9), nbins=32).update(torch.from_numpy(wild).cuda())
    assert state_of(sr) == ref.state()


# ---- 4. stream, behind the decoder ------------------------------------------------------------------------------------------
def test_stream_behind_the_decoder(E):
    import torch
    p = E.make_params(4, 8, 20, 10)
    st = E.Streams(p, 8, seed=17, eps=0.40, W=6, doped=(9,), stream0=5)
    sr = E.StreamRuns(p, 8, doped=(9,), nbins=64)
    ref = np_stream_runs(8, 4, (9,), 64)
    for npos in (100, 64, 136):
        cnt, tr = st.run(npos, trace=True)
        sr.update(tr, cnt)
        torch.cuda.synchronize()
        ref.feed(tr.cpu().numpy())
    cnt = cnt.cpu().numpy()
    runs, events = ref.hist[0], ref.hist[1]
    assert runs.sum() >= 100 and events.sum() >= 50
    assert np.flatnonzero(events).max() > np.flatnonzero(runs).max()    # an event longer than any run
    assert ref.sums[1] == cnt[:, 1].sum() and ref.sums[2] == cnt[:, 0].sum()
    assert state_of(sr) == ref.state()
    oh = sr.open_hist().cpu().numpy()
    assert (oh == ref.open_hist()).all() and oh.sum() == np.count_nonzero(ref.carry[:, 1]) + np.count_nonzero(ref.carry[:, 2])


def test_streaming_cli_with_runs(E, tmp_path):
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    argv = ["2", "6", "1", "9", "--L", "20", "--N", "10", "--eps-ini", "0.42", "--num-points", "1", "--max-blocks-err", "200",
            "--max-blocks", "4000", "--streams", "4", "--chunk", "25", "--seed", "3", "--quiet"]
    dirs = [tmp_path / n for n in ("plain", "runs1", "runs2")]
    B.streaming(argv + ["--outdir", str(dirs[0])])
    for d in dirs[1:]:
        B.streaming(argv + ["--outdir", str(d), "--runs", "--nbins", "48"])
    name = "SC_LDPC_4_8_L20_M5_DOP1_BP_Stream_SW6_Random_BLER_2.dat"
    assert sorted(os.listdir(str(dirs[0]))) == [name] and sorted(os.listdir(str(dirs[1]))) == [name, name + ".runs.pkl"]
    dat = (dirs[0] / name).read_bytes()
    assert dat == (dirs[1] / name).read_bytes() == (dirs[2] / name).read_bytes()
    got = [pickle.load(open(str(d / (name + ".runs.pkl")), "rb")) for d in dirs[1:]]
    # a traced replay of the same streams and chunks, through the reference
    p = E.make_params(4, 8, 20, 10)
    st = E.Streams(p, 4, 3, 0.42, 6, (9,), stream0=0)
    ref = np_stream_runs(4, 4, (9,), 48)
    tot = None
    while tot is None or (tot[3] < 200 and tot[7] < 4000):
        cnt, tr = st.run(25, trace=True)
        ref.feed(tr.cpu().numpy())
        tot = cnt[:, :8].sum(dim=0).cpu().numpy()
    assert ref.sums[1] > 0
    for (pt,) in got:
        assert sorted(pt) == ["doped", "eps", "hist", "nbins", "open_hist", "period", "phase", "streams", "sums"]
        assert (pt["eps"], pt["nbins"], pt["doped"], pt["period"], pt["streams"]) == (0.42, 48, (9,), 10, 4)
        for k, want in (("hist", ref.hist), ("sums", ref.sums), ("phase", ref.phase), ("open_hist", ref.open_hist())):
            assert pt[k].dtype == np.int64 and pt[k].shape == want.shape and (pt[k] == want).all(), k


# ---- 5. the simulator: the ordered stop cuts the statistics where it cuts the counters ------------------------------------------
@pytest.mark.parametrize("decoder,W", [("sw", 4), ("swc", 4), ("full", 0)])
def test_simulator_runs_cover_exactly_the_frames_of_the_point(E, decoder, W):
    import torch
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    p = E.make_params(4, 8, 12, 100)
    kw = dict(decoder=decoder, W=W, max_it=4, init_it=4, rng="philox", seed=11)
    point = B.Simulator(p, batch=4, runs=True, **kw).run_point(3, 0.40, 7, 64)
    f = point.f
    assert 4 < f < 64 and f % 4 != 0 and point.run["frame_err"] == 7    # the stop rule cut inside the second batch or a later one
    replay = B.Simulator(p, batch=64, runs=True, **kw)                   # the same frames in one batch, through the reference
    replay.fill_batch(3, 0.40, 0, f)
    res = replay.decode_batch(f)
    torch.cuda.synchronize()
    want, trial, _ = np_chain_runs(E.unpack_bits(res["erased"].cpu().numpy(), p.n), p.L, p.vns_pos)
    assert (trial[:, 0] > 0).sum() == 7 and trial[f - 1, 0] > 0         # the last frame fed is the tripping one
    for name in NAMES:
        assert point.runs[name].dtype == np.int64 and (point.runs[name] == want[name]).all(), name
    assert point.runs["fail_hist"].sum() == f and point.runs["run_hist"][0, 0] == f - 7
    assert point.runs["pos"][:, 1].sum() == point.run["users_err"] and point.runs["pos"][:, 0].sum() == point.run["block_err"]
    assert B.Simulator(p, batch=4, **kw).run_point(3, 0.40, 7, 64).runs is None
