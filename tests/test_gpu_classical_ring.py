"""The classical ring window decoder (-m gpu): sw_ring.hip's classical instances for (3,6), (4,8) and (5,10), through
scldpc_swc_bp_ring_device — against the CPU oracle at small sizes, against the real reference's fixtures, against the
whole-chain kernel at size (the queue-overflow repair among it), and through the Simulator and `bp_lim_iter --window classical`.
Inputs are sample_philox(adj16=True) followed by cn_sockets.  Everything is integer work: bit-exact, no tolerance anywhere."""
import functools
import os

import numpy as np
import pytest

from conftest import golden_names, load_golden, require_gpu

pytestmark = pytest.mark.gpu

# (9, 24): V = 24, C = 12, ragged; the two small (3,6) shapes carry every expurgation case
SMALL = [(3, 6, 14, 60), (3, 6, 9, 24), (3, 6, 16, 200), (4, 8, 12, 40), (4, 8, 16, 200), (5, 10, 12, 40), (5, 10, 16, 200)]
PAIRS = [(3, 6), (4, 8), (5, 10)]
EPS = (0.05, 0.3, 0.40, 0.44, 0.47, 0.52, 0.95)
WINDOWS = ((3, 2), (5, 4), (8, 20), (1, 3), (20, 5))                    # (W, max_it); W = 20 is wider than every chain
T_ORACLE = 12
NAMES = ("num_erasures", "num_blocks_err", "num_erasures_exp", "num_blocks_err_exp", "num_erasures_p1", "iterations", "status")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@pytest.fixture(scope="module")
def B():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import bp_decoding
    return bp_decoding


def _tables(E, p, seed, trial0, T, eps):
    a, ch = E.sample_philox(p, seed, trial0, T, eps, adj16=True)
    return a, E.cn_sockets(p, a), ch


def _same(torch, ref, out, what):
    """All eight counters (iterations among them) and the erased bitmap."""
    assert torch.equal(ref["counters"], out["counters"]), (what, ref["counters"][:4], out["counters"][:4])
    assert torch.equal(ref["erased"], out["erased"]), what


@functools.lru_cache(maxsize=None)
def _against_oracle(shape):
    """Decodes the shape's cases through the classical ring and compares the seven counters, the channel erasures and the
    erased bitmap with the oracle's literal classical window; returns what the cases exercised: trials that failed, that
    decoded, with ee != ne, with p1 > 0, whose result the cap changed against max_it = 1000, and whose result differs from the
    square window with the same W and cap."""
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    dv, dc, L, N = shape
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    mix = np.zeros(6, dtype=np.int64)
    for eps in EPS:
        a, cs, ch = _tables(E, p, 99, 0, T_ORACLE, eps)
        A = E.adj16_to_global(p, a.cpu().numpy())
        bits = E.unpack_bits(ch.cpu().numpy(), p.n)
        graphs = [O.Graph.from_vn_adj(po, A[t]) for t in range(T_ORACLE)]
        for W, max_it in WINDOWS:
            assert E.swc_ring_supported(p, W)
            out = E.sw_bp(p, a, ch, W, max_it, want_erased=True, classical=True, ring=True, d_cn_sock=cs)
            torch.cuda.synchronize()
            c = out["counters"].cpu().numpy()
            er = E.unpack_bits(out["erased"].cpu().numpy(), p.n)
            for t in range(T_ORACLE):
                what = (shape, eps, W, max_it, t)
                res, erased = O.decode_sw(graphs[t], bits[t], W, max_it, literal=True, square=False)
                assert c[t].tolist() == [res[k] for k in NAMES] + [int(bits[t].sum())], (what, c[t], res)
                assert res["status"] == 0 and (er[t] == erased).all(), what
                free, _ = O.decode_sw(graphs[t], bits[t], W, 1000, literal=True, square=False)
                sq, er_sq = O.decode_sw(graphs[t], bits[t], W, max_it, literal=True, square=True)
                mix += [res["num_erasures"] > 0, res["num_erasures"] == 0, res["num_erasures_exp"] != res["num_erasures"],
                        res["num_erasures_p1"] > 0, any(res[k] != free[k] for k in NAMES[:5]),
                        any(res[k] != sq[k] for k in NAMES[:5]) or bool((erased != er_sq).any())]
    return tuple(int(x) for x in mix)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "dv%d-dc%d-L%d-N%d" % s)
def test_classical_ring_equals_the_cpu_oracle(E, shape):
    _against_oracle(shape)


def test_the_oracle_cases_are_not_vacuous(E):
    """Of 2940 cases: 1946 failed, 994 decoded, 37 with ee != ne, 777 with p1 > 0, 841 changed by the cap, 2080 unlike the
    square window (the oracle on its CPU twin of the sampler gives the same totals)."""
    tot = np.sum([_against_oracle(shape) for shape in SMALL], axis=0)
    print("case mix:", tot.tolist())
    assert (tot > 0).all(), tot
    assert tot.tolist() == [1946, 994, 37, 777, 841, 2080], tot


@pytest.mark.parametrize("name", golden_names(variants=("bpfsw",)))
def test_classical_ring_matches_reference_golden(E, name):
    """decodeBP_SW of BPF:627-897 against the real reference's outputs, the reference's tables converted to 2 bytes."""
    import torch
    g = load_golden(name)
    m = g.meta
    p = E.make_params(m["dv"], m["dc"], m["L"], m["VNsPos"])
    adj, ch = E.sample_glibc_trials(p, g["seed"], m["eps"])
    a, ch = E.to_device(E.global_to_adj16(p, adj), ch)
    out = E.sw_bp(p, a, ch, m["W"], m["max_it"], want_erased=True, classical=True, ring=True, d_cn_sock=E.cn_sockets(p, a))
    torch.cuda.synchronize()
    c = out["counters"].cpu().numpy()
    for col, key in ((0, "ne"), (1, "be"), (2, "ee"), (3, "bee"), (4, "p1"), (7, "nch")):
        assert (c[:, col] == g[key]).all(), (name, key)
    assert (c[:, 6] == 0).all()
    if g.has("erased"):
        assert (E.unpack_bits(out["erased"].cpu().numpy(), p.n) == g["erased"]).all()


@pytest.mark.parametrize("dv,dc", PAIRS)
def test_classical_ring_equals_the_whole_chain_kernel_at_n_2000(E, dv, dc):
    import torch
    p = E.make_params(dv, dc, 20, 2000)
    for eps in (0.2, 0.46, 0.49):
        a, cs, ch = _tables(E, p, 7, 3, 8, eps)
        for W, max_it in ((10, 20), (20, 6)):
            ref = E.sw_bp(p, a, ch, W, max_it, want_erased=True, classical=True, ring=False)
            out = E.sw_bp(p, a, ch, W, max_it, want_erased=True, classical=True, ring=True, d_cn_sock=cs)
            torch.cuda.synchronize()
            _same(torch, ref, out, (dv, dc, eps, W, max_it))


def _queue_room(p, W):
    """Words per queue that ring_args (sw_ring.hip) finds beside the classical window's state when it aims at eight workgroups
    per CU, before the floor of 512 entries: the carve restated (every block rounded up to four words)."""
    up = lambda words: (words + 3) & ~3                                  # noqa: E731
    Cw, wpp = (p.cns_pos + 7) // 8, (p.vns_pos + 31) // 32
    state = (up((W + 3 * p.dv - 2) * Cw) + up((W + 2 * p.dv - 1) * wpp) + up((W * Cw + 3) // 4) + up(2 * p.L) + up(12))
    return (160 * 1024 // 8 // 4 - 64 - state) // 2


@pytest.mark.parametrize("dv,dc", PAIRS)
def test_classical_ring_repairs_a_queue_overflow_at_n_6000(E, dv, dc):
    """L = 12, N = 6000, W = 10: the window's state leaves the queues at their floor of 512 entries, and at eps = 0.3 a round
    releases thousands of VNs (1800 erased per position), so rounds overflow and the snapshot scan repairs them."""
    import torch
    p = E.make_params(dv, dc, 12, 6000)
    assert _queue_room(p, 10) < 512 and E.swc_ring_supported(p, 10)
    a, cs, ch = _tables(E, p, 31, 0, 4, 0.3)
    ref = E.sw_bp(p, a, ch, 10, 20, want_erased=True, classical=True, ring=False)
    out = E.sw_bp(p, a, ch, 10, 20, want_erased=True, classical=True, ring=True, d_cn_sock=cs)
    torch.cuda.synchronize()
    _same(torch, ref, out, (dv, dc))
    assert int(ref["counters"][:, 7].min().item()) > 512 * 12            # channel erasures: far beyond a queue per position


def test_classical_without_ring_keeps_the_chain_kernel_and_a_refusal_names_the_limit(E):
    import torch
    p = E.make_params(3, 6, 20, 200)
    a, cs, ch = _tables(E, p, 5, 0, 4, 0.45)
    ref = E.sw_bp(p, a, ch, 6, 5, want_erased=True, classical=True, ring=False)
    _same(torch, ref, E.sw_bp(p, a, ch, 6, 5, want_erased=True, classical=True), "ring=None")
    _same(torch, ref, E.sw_bp(p, a, ch, 6, 5, want_erased=True, classical=True, ring=True), "table on the fly")
    with pytest.raises(E.ScldpcError, match="LDS: the window's CN counts, S bits and queues exceed 160 KiB"):
        E.sw_bp(p, a, ch, 10 ** 6, 5, classical=True, ring=True)


RING = "sampler (first generation) + cn_sockets pass + sw_ring classical window (window state in LDS, dv = %d, dc = %d)"
CHAIN = "sampler (first generation) + sw_bp classical window (whole chain)"


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_run_point_counts_the_same_on_the_ring_path(B, E, dv, dc):
    import torch
    p = E.make_params(dv, dc, 20, 200)
    runs = []
    for ring in (True, False):
        sim = B.Simulator(p, decoder="swc", W=6, max_it=5, batch=32, seed=8, device="cuda:0", ring=ring)
        assert sim.path.decoder == ("swc_ring" if ring else "swc_chain")
        assert sim.kernel_choice() == (RING % (dv, dc) if ring else CHAIN)
        runs.append(dict(sim.run_point(0, 0.46, 40, 96).run))
    torch.cuda.synchronize()
    assert runs[0] == runs[1] and 0 < runs[0]["frames"] <= 96 and runs[0]["frame_err"] > 0


def test_cli_writes_the_same_file_on_the_ring_path(B, tmp_path, capfd):
    texts = {}
    for mode in ("on", "off", "auto"):
        d = tmp_path / mode
        capfd.readouterr()
        B.bp_lim_iter(["0", "6", "0", "5", "--window", "classical", "--dv", "3", "--dc", "6", "--L", "20", "--N", "200",
                       "--eps-ini", "0.47", "--num-points", "2", "--max-frames", "64", "--min-frame-err", "64", "--batch", "32",
                       "--seed", "5", "--ring", mode, "--outdir", str(d)])
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "kernels:" in ln]
        assert len(lines) == 1, lines
        named = RING % (3, 6) in lines[0]
        assert named == (mode == "on" or (mode == "auto" and B.CLASSICAL_RING_BY_DEFAULT)), (mode, lines[0])
        if not named:
            assert CHAIN in lines[0]
        files = sorted(os.listdir(d))
        assert files == ["SC_LDPC_3_6_L20_M100_BP_SW6_5it_Random_BLER_0.dat"]
        texts[mode] = open(d / files[0], "rb").read()
    assert texts["on"] == texts["off"] == texts["auto"] and len(texts["on"]) > 100
