"""The ring window decoder for the pairs (3,6) and (5,10) (-m gpu): sw_ring.hip's instances for a compile-time degree pair,
through scldpc_sw_bp_ring_device_deg — against the CPU oracle at small sizes, against the whole-chain kernel at size (the
queue-overflow repair among it), (4,8) through the new entry point against the old one, and the drivers.
Inputs are sample_philox(adj16=True) followed by cn_sockets.  Everything is integer work: bit-exact, no tolerance anywhere."""
import functools
import os

import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

SMALL = [(3, 6, 14, 60), (3, 6, 9, 24), (3, 6, 16, 200), (5, 10, 12, 40), (5, 10, 16, 200)]     # (9, 24): V = 24, C = 12, ragged
EPS = (0.05, 0.3, 0.40, 0.44, 0.47, 0.52, 0.95)
WINDOWS = ((3, 2, 0), (5, 4, 9), (8, 20, 60), (1, 3, 0), (20, 5, 0))    # (W, max_it, init_it); W = 20 is wider than every chain
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
    """All eight counters and the erased bitmap."""
    assert torch.equal(ref["counters"], out["counters"]), (what, ref["counters"][:4], out["counters"][:4])
    assert torch.equal(ref["erased"], out["erased"]), what


@functools.lru_cache(maxsize=None)
def _against_oracle(shape):
    """Decodes the shape's cases through the new entry point and compares every output with the CPU oracle (literal form for
    trial 0, peel form for the rest); returns what the cases exercised: trials that failed, that decoded, with ee != ne, with
    p1 > 0, and whose result the iteration cap changed against max_it = 1000."""
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    dv, dc, L, N = shape
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    failed = decoded = expurgated = phase1 = capped = 0
    for eps in EPS:
        a, cs, ch = _tables(E, p, 99, 0, T_ORACLE, eps)
        A = E.adj16_to_global(p, a.cpu().numpy())
        bits = E.unpack_bits(ch.cpu().numpy(), p.n)
        graphs = [O.Graph.from_vn_adj(po, A[t]) for t in range(T_ORACLE)]
        for W, max_it, init_it in WINDOWS:
            assert E.sw_ring_deg_supported(p, W) and not E.sw_ring_supported(p, W)
            out = E.sw_bp(p, a, ch, W, max_it, init_it, want_erased=True, ring=True, d_cn_sock=cs, deg=True)
            torch.cuda.synchronize()
            c = out["counters"].cpu().numpy()
            er = E.unpack_bits(out["erased"].cpu().numpy(), p.n)
            for t in range(T_ORACLE):
                what = (shape, eps, W, max_it, init_it, t)
                res, erased = O.decode_sw(graphs[t], bits[t], W, max_it, init_it, literal=(t == 0))
                assert c[t].tolist() == [res[k] for k in NAMES] + [int(bits[t].sum())], (what, c[t], res)
                assert res["status"] == 0 and (er[t] == erased).all(), what
                free, _ = O.decode_sw(graphs[t], bits[t], W, 1000, 1000, literal=False)
                failed += res["num_erasures"] > 0
                decoded += res["num_erasures"] == 0
                expurgated += res["num_erasures_exp"] != res["num_erasures"]
                phase1 += res["num_erasures_p1"] > 0
                capped += any(res[k] != free[k] for k in NAMES[:5])
    return failed, decoded, expurgated, phase1, capped


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "dv%d-dc%d-L%d-N%d" % s)
def test_ring_deg_decoder_equals_the_cpu_oracle(E, shape):
    _against_oracle(shape)


def test_the_oracle_cases_exercise_failures_expurgation_phase_1_and_a_binding_cap(E):
    tot = np.sum([_against_oracle(shape) for shape in SMALL], axis=0)
    assert (tot > 0).all(), tot                      # failed, decoded, ee != ne, p1 > 0, changed by the cap


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_ring_deg_decoder_equals_the_whole_chain_kernel_at_n_2000(E, dv, dc):
    import torch
    p = E.make_params(dv, dc, 20, 2000)
    for eps in (0.2, 0.46, 0.49):
        a, cs, ch = _tables(E, p, 7, 3, 8, eps)
        for W, max_it, init_it in ((10, 20, 0), (20, 6, 60)):
            ref = E.sw_bp(p, a, ch, W, max_it, init_it, want_erased=True, ring=False)
            out = E.sw_bp(p, a, ch, W, max_it, init_it, want_erased=True, ring=True, d_cn_sock=cs, deg=True)
            torch.cuda.synchronize()
            _same(torch, ref, out, (dv, dc, eps, W, max_it, init_it))


def _queue_room(p, W):
    """Words per queue that ring_args (sw_ring.hip) finds beside the window's state when it aims at eight workgroups per CU,
    before the floor of 512 entries: the carve restated (every block rounded up to four words)."""
    up = lambda words: (words + 3) & ~3                                  # noqa: E731
    Cw, wpp = (p.cns_pos + 7) // 8, (p.vns_pos + 31) // 32
    state = (up((W + 2 * p.dv - 1) * Cw) + up((W + p.dv) * wpp) + up((W * Cw + 3) // 4) + up(2 * p.L) + up(12))
    return (160 * 1024 // 8 // 4 - 64 - state) // 2


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_ring_deg_decoder_repairs_a_queue_overflow_at_n_6000(E, dv, dc):
    """L = 12, N = 6000, W = 10: the window's state leaves the queues at their floor of 512 entries, and at eps = 0.3 a round
    releases thousands of VNs (1800 erased per position), so rounds overflow and the snapshot scan repairs them with the
    DV-wide append."""
    import torch
    p = E.make_params(dv, dc, 12, 6000)
    assert _queue_room(p, 10) < 512 and E.sw_ring_deg_supported(p, 10)
    a, cs, ch = _tables(E, p, 31, 0, 4, 0.3)
    ref = E.sw_bp(p, a, ch, 10, 20, 0, want_erased=True, ring=False)
    out = E.sw_bp(p, a, ch, 10, 20, 0, want_erased=True, ring=True, d_cn_sock=cs, deg=True)
    torch.cuda.synchronize()
    _same(torch, ref, out, (dv, dc))
    assert int(ref["counters"][:, 7].min().item()) > 512 * 12            # channel erasures: far beyond a queue per position


@pytest.mark.parametrize("L,N,W,max_it,init_it", [(30, 200, 6, 4, 12), (100, 2000, 10, 20, 0)])
def test_4_8_through_the_deg_entry_point_is_the_ring_result(E, L, N, W, max_it, init_it):
    import torch
    p = E.make_params(4, 8, L, N)
    assert E.sw_ring_supported(p, W) and E.sw_ring_deg_supported(p, W)
    for eps in (0.3, 0.47):
        a, cs, ch = _tables(E, p, 91, 17, 8, eps)
        ref = E.sw_bp(p, a, ch, W, max_it, init_it, want_erased=True, ring=True, d_cn_sock=cs)
        out = E.sw_bp(p, a, ch, W, max_it, init_it, want_erased=True, ring=True, d_cn_sock=cs, deg=True)
        torch.cuda.synchronize()
        _same(torch, ref, out, (L, N, eps))                              # every counter, iterations included


def test_sw_bp_without_deg_keeps_the_chain_kernel_for_other_pairs(E):
    import torch
    p = E.make_params(3, 6, 20, 200)
    a, cs, ch = _tables(E, p, 5, 0, 4, 0.45)
    with pytest.raises(E.ScldpcError, match=r"\(4,8\) chain only"):
        E.sw_bp(p, a, ch, 6, 5, ring=True)
    ref = E.sw_bp(p, a, ch, 6, 5, want_erased=True, ring=False)
    _same(torch, ref, E.sw_bp(p, a, ch, 6, 5, want_erased=True), "ring=None")                   # today's choice: the chain kernel
    _same(torch, ref, E.sw_bp(p, a, ch, 6, 5, want_erased=True, deg=True), "deg, table on the fly")
    with pytest.raises(E.ScldpcError, match=r"\(3,6\), \(4,8\) and \(5,10\) chains only"):
        E.sw_bp(p, a, ch, 10 ** 6, 5, ring=True, deg=True)              # a window whose state exceeds the LDS


RING = "sampler (first generation) + cn_sockets pass + sw_ring (window state in LDS, dv = %d, dc = %d)"


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_run_point_counts_the_same_on_the_ring_path(B, E, dv, dc):
    import torch
    p = E.make_params(dv, dc, 20, 200)
    runs = []
    for ring in (True, False):
        sim = B.Simulator(p, decoder="sw", W=6, max_it=5, init_it=10, batch=32, seed=8, device="cuda:0", ring=ring)
        assert sim.ring_deg == ring and sim.path.decoder == ("sw_ring" if ring else "sw_chain")
        if ring:
            assert sim.kernel_choice() == RING % (dv, dc)
        runs.append(dict(sim.run_point(0, 0.46, 40, 96).run))
    torch.cuda.synchronize()
    assert runs[0] == runs[1] and 0 < runs[0]["frames"] <= 96 and runs[0]["frame_err"] > 0


def test_cli_writes_the_same_file_on_the_ring_path(B, tmp_path, capfd):
    texts = {}
    for mode in ("on", "off", "auto"):
        d = tmp_path / mode
        capfd.readouterr()
        B.sw_lim_iter(["0", "6", "0", "5", "10", "--dv", "3", "--dc", "6", "--L", "20", "--N", "200", "--eps-ini", "0.47",
                       "--num-points", "2", "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5",
                       "--ring", mode, "--outdir", str(d)])
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "kernels:" in ln]
        assert len(lines) == 1, lines
        named = RING % (3, 6) in lines[0]
        assert named == (mode == "on" or (mode == "auto" and B.RING_DEG_BY_DEFAULT)), (mode, lines[0])
        if not named:
            assert "sampler (first generation) + sw_bp (whole chain)" in lines[0]
        files = sorted(os.listdir(d))
        assert files == ["SC_LDPC_3_6_L20_M100_BP_SW6_5it_10init_Random_BLER_0.dat"]
        texts[mode] = open(d / files[0], "rb").read()
    assert texts["on"] == texts["off"] == texts["auto"] and len(texts["on"]) > 100
