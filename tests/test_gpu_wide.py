"""The wide form of the 4-bit level decoder (-m gpu): full_bp_small.hip with 32-bit queue entries and one 1024-thread
workgroup per CU — trials of more than 65536 CNs (bp_traj's default N = 5000, L = 50) — against the 16-bit form where both
apply, the first-generation kernel where only it applies, the reference's own graphs and the published-curve inputs.
Everything is bit-exact (integer counters, rows, bitmaps): no tolerance anywhere."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden, require_gpu
from small_queue_cases import front_overflows, natural_qcap

pytestmark = pytest.mark.gpu

PUB = os.path.join(GOLDEN_DIR, "published")
WIDE_LINE = "full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries"


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


def _same(torch, ref, out, what):
    """All eight counters, every row up to the iteration count (and nothing but zeros beyond, where both hold zeros), the
    erased bitmap."""
    assert torch.equal(ref["counters"], out["counters"]), (what, ref["counters"][:4], out["counters"][:4])
    if ref["erased"] is not None:
        assert torch.equal(ref["erased"], out["erased"]), what
    if ref["rows"] is not None:
        its = ref["counters"][:, 5].long()
        cap = ref["rows"].shape[1]
        live = (torch.arange(cap, device=its.device)[None, :] < its[:, None])[:, :, None]
        assert torch.equal(ref["rows"] * live, out["rows"] * live), what


@pytest.mark.parametrize("L,N,eps", [(50, 1000, 0.48), (100, 1000, 0.47), (10, 10, 0.5), (16, 200, 0.48)])
def test_wide_equals_narrow_where_both_apply(E, L, N, eps):
    """full_bp_wide against full_bp_cn16(sockets=True) on sample_philox_sock16's tables: with and without rows, terminated
    and truncated, unlimited and with a binding cap."""
    import torch
    p = E.make_params(4, 8, L, N)
    assert E.full_bp_wide_supported(p) and E.full_bp_sock16_supported(p)
    a, cs, ch = E.sample_philox_sock16(p, 91, 17, 96, eps)
    bound = 0
    for is_term in (True, False):
        for cap in (0, 3, 40):
            for rows_cap in (0, 600):
                ref = E.full_bp_cn16(p, a, cs, ch, max_it=cap, is_term=is_term, want_erased=True, sockets=True, rows_cap=rows_cap)
                out = E.full_bp_wide(p, a, cs, ch, max_it=cap, is_term=is_term, want_erased=True, rows_cap=rows_cap)
                torch.cuda.synchronize()
                _same(torch, ref, out, (L, N, is_term, cap, rows_cap))
                bound += int((ref["counters"][:, 5] == cap).sum().item()) if cap else 0
    assert bound > 0                                                     # a cap did bind


@pytest.mark.parametrize("L,N,eps,is_term", [(50, 5000, 0.47, True), (50, 5000, 0.46, True), (100, 2000, 0.47, True),
                                             (50, 2474, 0.48, True), (20, 5000, 0.47, False), (50, 6000, 0.46, True)])
def test_wide_equals_the_first_generation_where_only_it_applies(E, L, N, eps, is_term):
    """sample_philox(adj16) -> cn_sockets -> full_bp_wide against full_bp on the same tables: all eight counters (the
    iteration count included), rows, erased bitmap; caps 0, 1, 40, 500."""
    import torch
    p = E.make_params(4, 8, L, N)
    assert E.full_bp_wide_supported(p) and not E.full_bp_sock16_supported(p) and not E.cn16_supported(p)
    T = 48
    a, ch = E.sample_philox(p, 2024, 5, T, eps, adj16=True)
    cs = E.cn_sockets(p, a)
    for cap in (0, 1, 40, 500):
        for rows_cap in (0, 700):
            ref = E.full_bp(p, a, ch, max_it=cap, is_term=is_term, rows_cap=rows_cap, want_erased=True)
            out = E.full_bp_wide(p, a, cs, ch, max_it=cap, is_term=is_term, rows_cap=rows_cap, want_erased=True)
            torch.cuda.synchronize()
            _same(torch, ref, out, (L, N, eps, cap, rows_cap))


def test_wide_decoder_takes_frontiers_of_many_queue_fulls_from_the_snapshot(E):
    """Low eps: nearly every erased VN is resolved in iteration 0, so the first frontier is many queue-fulls (6092 entries at
    this size against tens of thousands of degree-1 CNs) and the pushes of a round overflow the queue (scan rounds back to
    back) — counters and residual still equal the flooding kernel's."""
    import torch
    p = E.make_params(4, 8, 50, 5000)
    for eps in (0.2, 0.35, 0.6, 0.97):
        a, ch = E.sample_philox(p, 79, 0, 32, eps, adj16=True)
        cs = E.cn_sockets(p, a)
        if eps < 0.5:                                        # the inputs do fill the queue: more degree-1 CNs than its entries
            assert front_overflows(p, a.cpu().numpy(), ch.cpu().numpy(), natural_qcap(p, "traj", True)), eps
        ref = E.full_bp(p, a, ch, want_erased=True, rows_cap=64)
        out = E.full_bp_wide(p, a, cs, ch, want_erased=True, rows_cap=64)
        torch.cuda.synchronize()
        _same(torch, ref, out, eps)


@pytest.mark.parametrize("name", ["c3_bpt_M2500_L50_e460_trunc", "c3_bpt_M2500_L50_e470_term"])
def test_wide_decoder_on_the_references_own_graphs(E, name):
    """glibc replay of the fixture's seeds -> global_to_adj16 -> cn_sockets -> full_bp_wide with rows: ne, be, ee, bee, nch,
    the iteration count and every trajectory row equal what the real reference wrote at its shipped size."""
    import torch
    g = load_golden(name)
    m = g.meta
    p = E.make_params(m["dv"], m["dc"], m["L"], m["VNsPos"])
    assert p.nk == 132500 and E.full_bp_wide_supported(p)
    T = g.T
    adj, ch = E.sample_glibc_trials(p, g["seed"][:T], m["eps"])
    d_a, d_ch = E.to_device(E.global_to_adj16(p, adj), ch)
    d_cs = E.cn_sockets(p, d_a)
    out = E.full_bp_wide(p, d_a, d_cs, d_ch, max_it=g.max_it, is_term=bool(m["is_term"]), rows_cap=2048, want_erased=True)
    torch.cuda.synchronize()
    c, rows = out["counters"].cpu().numpy(), out["rows"].cpu().numpy()
    for col, key in ((0, "ne"), (1, "be"), (2, "ee"), (3, "bee"), (7, "nch")):
        assert (c[:, col] == g[key][:T]).all(), (name, key, c[:, col], g[key][:T])
    assert (c[:, 6] == 0).all() and (c[:, 4] == 0).all()
    assert (E.unpack_bits(out["erased"].cpu().numpy(), p.n).sum(axis=1) == g["ne"][:T]).all()
    assert [int(x) for x in c[:, 5]] == [len(g.rows_of(t)) for t in range(T)], name
    for t in range(T):
        ref = g.rows_of(t)
        assert len(ref) <= 2048 and (rows[t, :len(ref)] == ref).all(), (name, t)


def test_wide_decoder_on_the_published_curve_inputs(E):
    """Exactly the inputs of test_bp_trajectories_reproduce_the_published_files_statistics[L50_M2500…] (seed 4711, 8192
    frames in batches of 2048, eps and cap from the fixture's meta, truncated): counters and rows of full_bp_wide equal
    full_bp's on every frame, so the statistics checked there carry over unchanged."""
    import torch
    m = json.loads(str(np.load(os.path.join(PUB, "bp_trajectories_L50_M2500_e4600_trunc_500it.npz"))["meta"]))
    p = E.make_params(m["dv"], m["dc"], m["L"], m["vns_pos"])
    cap, frames, batch = m["max_it"], 8192, 2048
    assert (p.L, p.vns_pos, cap, bool(m["is_term"])) == (50, 5000, 500, False)
    for b0 in range(0, frames, batch):
        adj, ch = E.sample_philox(p, 4711, b0, batch, m["eps"], adj16=True)
        cs = E.cn_sockets(p, adj)
        ref = E.full_bp(p, adj, ch, max_it=cap, is_term=False, rows_cap=cap)
        out = E.full_bp_wide(p, adj, cs, ch, max_it=cap, is_term=False, rows_cap=cap)
        torch.cuda.synchronize()
        _same(torch, ref, out, b0)
        del adj, ch, cs, ref, out


def test_bp_traj_at_its_default_size_writes_the_same_file_on_the_wide_path(B, tmp_path, capfd):
    """`bp_traj 0 0 0 500 0` at the default size (N = 5000, L = 50): the kernels line names the wide path when it is selected
    (--wide on; --wide auto follows WIDE_BY_DEFAULT) and the written file is byte-identical to the first-generation path's,
    in the 4- and 3-column layouts."""
    texts = {}
    for cols in (4, 3):
        for mode in ("on", "off", "auto"):
            d = tmp_path / f"{mode}{cols}"
            capfd.readouterr()
            B.bp_traj(["0", "0", "0", "500", "0", "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "11",
                       "--cols", str(cols), "--wide", mode, "--outdir", str(d)])
            err = capfd.readouterr().err
            line = [ln for ln in err.split("\n") if "kernels:" in ln]
            assert len(line) == 1, err
            named = WIDE_LINE + ", trajectory rows)" in line[0]
            assert named == (mode == "on" or (mode == "auto" and B.WIDE_BY_DEFAULT)), (mode, line[0])
            if named:
                assert "sampler (first generation) + cn_sockets pass" in line[0]
            files = sorted(os.listdir(d))
            assert files == ["trajectories_0.4600_truncated_SC_LDPC_4_8_L50_M2500_BP_Full_500it_Random_BLER_0.dat"]
            texts[mode, cols] = open(d / files[0]).read()
        assert texts["on", cols] == texts["off", cols] == texts["auto", cols]
        assert len(texts["on", cols].split("\n\n")) - 1 == 64
    assert texts["on", 4] != texts["on", 3]


def test_bp_lim_iter_at_n_5000_writes_the_same_file_on_the_wide_path(B, tmp_path, capfd):
    outs = {}
    for mode in ("on", "off"):
        d = tmp_path / mode
        capfd.readouterr()
        B.bp_lim_iter(["2", "0", "0", "120", "--N", "5000", "--eps-ini", "0.47", "--num-points", "1", "--max-frames", "96",
                       "--min-frame-err", "96", "--batch", "48", "--seed", "3", "--wide", mode, "--outdir", str(d)])
        err = capfd.readouterr().err
        assert ((WIDE_LINE + ")") in err) == (mode == "on"), err
        files = sorted(os.listdir(d))
        assert len(files) == 1
        outs[mode] = open(d / files[0]).read()
    assert outs["on"] == outs["off"] and len(outs["on"].strip().split("\n")) == 2


def test_simulator_samples_the_socket_table_where_the_second_generation_sampler_takes_it(B, E):
    """L = 100, N = 2000 (BASELINE config 4's ensemble; 8000 sockets per position): sample_philox_sock16 feeds the wide
    decoder; a point's run counters equal the first-generation path's."""
    import torch
    p = E.make_params(4, 8, 100, 2000)
    runs = []
    for wide in (True, False):
        sim = B.Simulator(p, decoder="full", max_it=200, batch=64, seed=8, device="cuda:0", wide=wide)
        assert sim.wide == wide and sim.wide_sock == wide
        if wide:
            assert sim.kernel_choice().startswith("sampler_v3 (CN->socket table) + full_bp_small wide")
        res = sim.run_point(0, 0.475, 128, 128)
        runs.append(dict(res.run))
    torch.cuda.synchronize()
    assert runs[0] == runs[1] and runs[0]["frames"] == 128
