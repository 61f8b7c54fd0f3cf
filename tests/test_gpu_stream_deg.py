"""Streaming mode for the VN degrees 3 and 5 on the GPU (-m gpu): stream_gen_kernel<*, 3 | 5> and stream_dec_kernel<3 | 5>
through the C-ABI against the CPU twin (the streaming oracle with Philox keys and the node-level decoder), position by
position, across launches and buffer wrap-arounds, as tests/test_gpu_stream.py does for dv = 4.  The shapes: sockets per
position S = V * dv with S mod 4 = 2 (N = 10), 0, 1 (3,9 at N = 99: odd S, the unpaired copies) and 3 (5,15 at N = 99);
dc = 2 dv and dc = 3 dv; several rows and several Philox calls per thread (N = 1000, 5000); L = 20 at dv = 5, a buffer so
short that the reference has re-used the CN rows of a position by the time it expurgates it.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

SEED, SID0 = 17, 5


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _twin_rows(dv, dc, L, N, eps, W, doped, npos, ns):
    """The oracle's rows [ns][npos][10] of streams SID0 .. SID0 + ns - 1: computed once per case, read by every test of it."""
    from fl_scaling_sc_ldpc_amd import engine
    from oracle import oracle
    oracle.build(with_reference=False)
    p = engine.make_params(dv, dc, L, N)
    po = oracle.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    out = np.empty((ns, npos, 10), dtype=np.int64)
    for s in range(ns):
        tw = oracle.Stream(po, SEED, eps, W, doped, rng_mode=1, decoder=1, sid=SID0 + s)
        for k in range(npos):
            o = tw.step()
            out[s, k] = [o[f] for f in oracle.Stream.FIELDS]
    out.setflags(write=False)
    return out


def _run_against_twin(E, dv, dc, L, N, eps, W, doped, chunks, ns):
    p = E.make_params(dv, dc, L, N)
    want = _twin_rows(dv, dc, L, N, eps, W, tuple(doped), sum(chunks), ns)
    st = E.Streams(p, ns, seed=SEED, eps=eps, W=W, doped=doped, stream0=SID0)
    done = 0
    for npos in chunks:                                   # the state carries over from launch to launch
        cnt, tr = st.run(npos, trace=True)
        tr = tr.cpu().numpy().astype(np.int64); cnt = cnt.cpu().numpy()
        bad = np.argwhere(tr != want[:, done:done + npos])
        assert bad.size == 0, ((dv, dc, L, N), done, bad[:3].tolist(), tr[tuple(bad[0][:2])].tolist(),
                               want[bad[0][0], done + bad[0][1]].tolist())
        done += npos
        assert (cnt[:, :8] == want[:, done - 1, 2:]).all() and (cnt[:, 8] == done).all() and (cnt[:, 9] == done + L // 2).all()
    return want


# dv, dc, L, N, eps, W, doped, chunks, streams, (positions in error, positions counted[, erasures after expurgation]) of
# stream SID0; the third figure where the buffer is so short that the expurgation finds no pair (the oracle's count)
CASES = [
    (3, 6, 20, 10, 0.42, 6, (), (40, 35, 60), 3, (80, 133)),
    (3, 6, 20, 10, 0.45, 7, (5, 6), (50, 45, 55), 3, (26, 106)),
    (5, 10, 20, 10, 0.45, 6, (), (40, 35, 60), 3, (131, 131, 574)),
    (5, 10, 20, 10, 0.47, 5, (7, 8, 9, 10), (50, 45, 55), 3, (51, 94, 197)),
    (3, 6, 30, 100, 0.46, 12, (10, 11), (70, 30), 3, (9, 82)),
    (5, 10, 30, 100, 0.48, 11, (9, 10, 11, 12), (70, 30), 3, (8, 68)),
    (5, 10, 30, 100, 0.46, 10, (), (55, 45), 3, (95, 96)),
    (3, 9, 30, 99, 0.28, 10, (7, 8), (45, 40), 3, (0, 65)),
    (5, 15, 30, 99, 0.30, 8, (), (45, 40), 3, (80, 81)),
    (3, 6, 50, 1000, 0.46, 20, (), (30, 30), 2, (0, 58)),
    (5, 10, 50, 1000, 0.48, 20, (10, 11, 12, 13), (60,), 2, (0, 40)),
    (3, 6, 50, 5000, 0.46, 20, (24,), (12,), 2, (0, 10)),
    (5, 10, 50, 5000, 0.48, 20, (), (12,), 2, (0, 8)),
]


@pytest.mark.parametrize("dv,dc,L,N,eps,W,doped,chunks,ns,figures", CASES,
                         ids=["%d_%d_L%d_N%d_W%d_dop%d" % (c[0], c[1], c[2], c[3], c[5], len(c[6])) for c in CASES])
def test_streams_equal_cpu_twin(E, dv, dc, L, N, eps, W, doped, chunks, ns, figures):
    want = _run_against_twin(E, dv, dc, L, N, eps, W, doped, chunks, ns)
    # the reference this compares with is the one the case was chosen on: block errors / blocks counted of stream SID0
    last = dict(zip(("pos", "nep", "ne", "be", "ee", "bee", "gb", "gbl", "gbe", "gble"), want[0, -1].tolist()))
    assert (last["be"], last["gbl"]) == figures[:2]
    if len(figures) == 3:
        assert last["ee"] == figures[2]


# ceil(L/2) - 3dv + 2 = -1, -2, -1, -1: the reference has re-used the rows of one or two of the dv CN positions of the VN
# position it expurgates (always edge 0's first), at dv = 5, 4 and 3; (4,8) at L = 20 (tests/test_gpu_stream.py) is the first
# buffer long enough.  dv, dc, L, N, eps, W, doped, chunks, (be, gbl, ee) of stream SID0 after 135 positions
SHORT = [(5, 10, 24, 10, 0.45, 6, (), (40, 35, 60), (131, 131, 574)),
         (5, 10, 22, 10, 0.45, 6, (7, 8, 9, 10), (50, 45, 40), (44, 84, 159)),
         (4, 8, 18, 10, 0.45, 5, (), (40, 35, 60), (130, 132, 523)),
         (3, 6, 12, 10, 0.42, 4, (), (40, 35, 60), (86, 133, 300))]


@pytest.mark.parametrize("dv,dc,L,N,eps,W,doped,chunks,figures", SHORT, ids=["%d_%d_L%d" % c[:3] for c in SHORT])
def test_buffers_whose_cn_rows_are_reused_before_the_expurgation_equal_cpu_twin(E, dv, dc, L, N, eps, W, doped, chunks, figures):
    """2dv - 1 <= ceil(L/2) < 3dv - 2: the reference expurgates a position after it has re-used the slot of its edge-0 CN
    position, finds no VN pair there and counts every erased VN; the decoder must count the same, launch sizes regardless."""
    want = _run_against_twin(E, dv, dc, L, N, eps, W, doped, chunks, 3)
    assert (int(want[0, -1, 3]), int(want[0, -1, 7]), int(want[0, -1, 4])) == figures


LAYOUT_CASES = [c for c in CASES if c[3] == 99 or (c[3] == 100 and c[6])]


@pytest.mark.parametrize("env", ["SCLDPC_DEBUG_STREAM_WIDE", "SCLDPC_DEBUG_STREAM_LEGACY"])
@pytest.mark.parametrize("dv,dc,L,N,eps,W,doped,chunks,ns,figures", LAYOUT_CASES,
                         ids=["%d_%d_N%d" % (c[0], c[1], c[3]) for c in LAYOUT_CASES])
def test_the_other_generation_paths_give_the_same_stream(E, monkeypatch, env, dv, dc, L, N, eps, W, doped, chunks, ns, figures):
    """The 16-bit-counter fallback ranking with its CN rows built in a pass of their own (SCLDPC_DEBUG_STREAM_WIDE) and the
    generator's other LDS layout (SCLDPC_DEBUG_STREAM_LEGACY), at S mod 4 = 0, 1 and 3 and odd dc: the same twin."""
    assert len(LAYOUT_CASES) == 4
    monkeypatch.setenv(env, "1")
    _run_against_twin(E, dv, dc, L, N, eps, W, doped, chunks, ns)


@pytest.mark.parametrize("dv,dc,L,N,eps,W,doped,npos,errs", [(3, 6, 20, 10, 0.45, 7, (5, 6), 150, (22, 106)),
                                                             (5, 10, 30, 100, 0.48, 11, (9, 10, 11, 12), 100, None)])
def test_same_input_mode_equals_the_literal_oracle_on_the_glibc_stream(E, oracle, dv, dc, L, N, eps, W, doped, npos, errs):
    """The kernels fed with main_streaming's own draws (scldpc_stream_glibc_inputs_host) against the oracle's glibc stream
    with the literal message decoder, row by row; two launches, and a second slot fed from another seed."""
    import torch
    p = E.make_params(dv, dc, L, N)
    po = oracle.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    G = L // 2 + npos
    ins = [E.stream_glibc_inputs(p, SEED + k, eps, doped, G) for k in range(2)]
    st = E.InputStreams(p, np.stack([ins[0][0], ins[1][0]]), np.stack([ins[0][1], ins[1][1]]), W, doped)
    first = npos // 3
    _, tr1 = st.run(first, trace=True)
    cnt, tr2 = st.run(npos - first, trace=True)
    torch.cuda.synchronize()
    for slot in range(2):
        tw = oracle.Stream(po, SEED + slot, eps, W, doped, rng_mode=0, decoder=0)
        want = np.array([[o[f] for f in oracle.Stream.FIELDS] for o in (tw.step() for _ in range(npos))])
        rows = np.concatenate([tr1[slot].cpu().numpy(), tr2[slot].cpu().numpy()])
        assert (rows == want).all(), (slot, np.argwhere(rows != want)[:3].tolist())
        c = cnt[slot].cpu().numpy()
        assert c[:8].tolist() == want[-1, 2:].tolist() and c[8] == npos and c[9] == G
        if slot == 0 and errs:
            assert (want[-1, 3], want[-1, 7]) == errs


def test_streaming_cli_at_3_6_sums_the_same_streams(E, tmp_path):
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    B.streaming(["2", "6", "2", "5", "6", "--dv", "3", "--dc", "6", "--L", "20", "--N", "10", "--eps-ini", "0.45",
                 "--num-points", "1", "--max-blocks-err", "50", "--max-blocks", "4000", "--streams", "4", "--chunk", "25",
                 "--seed", "3", "--outdir", str(tmp_path), "--quiet"])
    rows = open(tmp_path / "SC_LDPC_3_6_L20_M5_DOP2_BP_Stream_SW6_Random_BLER_2.dat").read().strip().split("\n")
    assert rows[0] == B.STREAM_HEADER.strip() and len(rows) == 2
    f = rows[1].split()
    assert len(f) == 13 and f[0] == "0.450000"
    ne, gb, be, gbl, ee, gbe, bee, gble = (int(x) for x in f[5:])
    assert bee >= 50 or gble >= 4000
    st = E.Streams(E.make_params(3, 6, 20, 10), 4, 3, 0.45, 6, (5, 6), stream0=0)     # same streams, same chunks
    tot = None
    while tot is None or (tot[3] < 50 and tot[7] < 4000):
        tot = st.run(25)[0][:, :8].sum(dim=0).cpu().numpy()
    assert [ne, be, ee, bee, gb, gbl, gbe, gble] == tot.tolist()


def test_streaming_cli_at_5_10_writes_its_file(E, tmp_path):
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    B.streaming(["0", "11", "4", "9", "10", "11", "12", "--dv", "5", "--dc", "10", "--L", "30", "--N", "100", "--eps-ini",
                 "0.48", "--num-points", "1", "--max-blocks-err", "10", "--max-blocks", "300", "--streams", "3", "--chunk",
                 "20", "--seed", "4", "--outdir", str(tmp_path), "--quiet"])
    rows = open(tmp_path / "SC_LDPC_5_10_L30_M50_DOP4_BP_Stream_SW11_Random_BLER_0.dat").read().strip().split("\n")
    assert rows[0] == B.STREAM_HEADER.strip() and len(rows) == 2 and rows[1].split()[0] == "0.480000"


def test_streaming_cli_glibc_run_at_3_6_equals_the_oracle_stopped_by_the_same_rule(E, oracle, tmp_path):
    """`sw … --rng glibc`: one stream from srandom(seed), stopped at the first position at which num_blocks_err_exp or
    num_blocks_generated_exp reaches its bound (BPF:2033) — the oracle's glibc stream with the literal decoder, stepped
    until the same rule trips."""
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    B.streaming(["1", "7", "2", "5", "6", "--dv", "3", "--dc", "6", "--L", "20", "--N", "10", "--eps-ini", "0.45",
                 "--num-points", "1", "--max-blocks-err", "12", "--max-blocks", "400", "--rng", "glibc", "--seed", "29",
                 "--chunk", "16", "--outdir", str(tmp_path), "--quiet"])
    rows = open(tmp_path / "SC_LDPC_3_6_L20_M5_DOP2_BP_Stream_SW7_Random_BLER_1.dat").read().strip().split("\n")
    assert len(rows) == 2
    tw = oracle.Stream(oracle.Params(3, 6, 20, 5, 10), 29, 0.45, 7, (5, 6), rng_mode=0, decoder=0)
    while True:
        o = tw.step()
        if o["bee"] >= 12 or o["gble"] >= 400:
            break
    f = rows[1].split()
    assert f[0] == "0.450000"
    assert [int(x) for x in f[5:]] == [o[k] for k in ("ne", "gb", "be", "gbl", "ee", "gbe", "bee", "gble")]


def test_refusals_name_the_limit(E):
    from fl_scaling_sc_ldpc_amd import _lib
    for dv, dc in ((2, 4), (6, 12)):
        p = _lib.CodeParams(dv, dc, 30, 5 * dv, 5 * dc)                 # dv * vns_pos = dc * cns_pos
        assert not E.stream_supported(p, 4)
        with pytest.raises(E.ScldpcError, match="dv = 3, 4 or 5"):
            E.Streams(p, 1, 1, 0.4, 4)
    with pytest.raises(E.ScldpcError, match="L/2"):                      # W + dv - 1 = 11 > 10
        E.Streams(E.make_params(5, 10, 20, 10), 1, 1, 0.4, 7)
    assert E.stream_supported(E.make_params(5, 10, 20, 10), 6)
