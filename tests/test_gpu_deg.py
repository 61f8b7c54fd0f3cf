"""The 4-bit level decoder for the pairs (3,6) and (5,10) (-m gpu): full_bp_small.hip's instances for a compile-time degree
pair, through the _deg entry points — against the CPU oracle at small sizes, against the first-generation kernel where the
oracle is too slow, the wide forms at N = 5000, (4,8) through the same entry points, the fixpoint form and the drivers.
Inputs are sample_philox(adj16=True) followed by cn_sockets.  Everything is integer work: bit-exact, no tolerance anywhere."""
import functools
import os

import numpy as np
import pytest

from conftest import require_gpu
from small_queue_cases import front_overflows, natural_qcap

pytestmark = pytest.mark.gpu

SMALL = [(3, 6, 14, 60), (3, 6, 9, 24), (3, 6, 16, 200), (5, 10, 12, 40), (5, 10, 16, 200)]     # (9, 24): n = 216, ragged
EPS = (0.05, 0.3, 0.44, 0.48, 0.52, 0.95)
MODES = ((True, 0), (False, 0), (True, 3))                              # (is_term, max_it)
T_ORACLE, ROWS_CAP = 24, 1024


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
    """All eight counters, every row up to the iteration count, the erased bitmap."""
    assert torch.equal(ref["counters"], out["counters"]), (what, ref["counters"][:4], out["counters"][:4])
    if ref["erased"] is not None:
        assert torch.equal(ref["erased"], out["erased"]), what
    if ref["rows"] is not None:
        its = ref["counters"][:, 5].long()
        cap = ref["rows"].shape[1]
        live = (torch.arange(cap, device=its.device)[None, :] < its[:, None])[:, :, None]
        assert torch.equal(ref["rows"] * live, out["rows"] * live), what


def _tables(E, p, seed, trial0, T, eps):
    a, ch = E.sample_philox(p, seed, trial0, T, eps, adj16=True)
    return a, E.cn_sockets(p, a), ch


@functools.lru_cache(maxsize=None)
def _against_oracle(shape):
    """Decodes the shape's cases with the narrow trajectory form and compares every output with the CPU oracle; returns what
    the cases exercised: (trials that failed, trials that decoded, trials with ee != ne, trials a cap of 3 stopped)."""
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    dv, dc, L, N = shape
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    assert E.full_bp_deg_supported(p)
    failed = decoded = expurgated = capped = 0
    for eps in EPS:
        a, cs, ch = _tables(E, p, 99, 0, T_ORACLE, eps)
        A = E.adj16_to_global(p, a.cpu().numpy())
        bits = E.unpack_bits(ch.cpu().numpy(), p.n)
        graphs = [O.Graph.from_vn_adj(po, A[t]) for t in range(T_ORACLE)]
        for is_term, max_it in MODES:
            out = E.full_bp_deg(p, a, cs, ch, max_it=max_it, is_term=is_term, rows_cap=ROWS_CAP, want_erased=True)
            lvl = E.full_bp_deg(p, a, cs, ch, max_it=max_it, is_term=is_term, want_erased=True)
            torch.cuda.synchronize()
            assert torch.equal(out["counters"], lvl["counters"]) and torch.equal(out["erased"], lvl["erased"])
            c, rows = out["counters"].cpu().numpy(), out["rows"].cpu().numpy()
            er = E.unpack_bits(out["erased"].cpu().numpy(), p.n)
            for t in range(T_ORACLE):
                what = (shape, eps, is_term, max_it, t)
                res, erased, orows = O.decode_bp(graphs[t], bits[t], max_it=max_it, is_term=int(is_term),
                                                 literal=(t == 0), rows_cap=ROWS_CAP)
                k = res["iterations"]
                assert k <= ROWS_CAP
                assert c[t].tolist() == [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"],
                                         res["num_blocks_err_exp"], 0, k, 0, int(bits[t].sum())], (what, c[t], res)
                assert res["status"] == 0 and (er[t] == erased).all(), what
                for col, name in enumerate(("deg1", "recovered", "first_pos")):
                    assert (rows[t, :k, col] == orows[name]).all(), (what, name)
                failed += res["num_erasures"] > 0
                decoded += res["num_erasures"] == 0
                expurgated += res["num_erasures_exp"] != res["num_erasures"]
                capped += max_it > 0 and k == max_it and res["num_erasures"] > 0
    return failed, decoded, expurgated, capped


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "dv%d-dc%d-L%d-N%d" % s)
def test_deg_decoder_equals_the_cpu_oracle(E, shape):
    _against_oracle(shape)


def test_the_oracle_cases_exercise_failures_expurgation_and_a_binding_cap(E):
    tot = np.sum([_against_oracle(shape) for shape in SMALL], axis=0)
    assert (tot > 0).all(), tot                      # failed, decoded, ee != ne, iterations == 3 with erasures left


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_deg_decoder_equals_the_first_generation_at_n_1000(E, dv, dc):
    """L = 50, N = 1000: all eight counters, rows and bitmap of full_bp on the same tables; at eps = 0.2 iteration 0's
    frontier is several queue-fulls (the snapshot path)."""
    import torch
    p = E.make_params(dv, dc, 50, 1000)
    assert E.full_bp_deg_supported(p)
    for eps in (0.2, 0.46, 0.49):
        a, cs, ch = _tables(E, p, 7, 3, 8, eps)
        if eps == 0.2:                                       # the inputs do fill the queue: more degree-1 CNs than its entries
            assert front_overflows(p, a.cpu().numpy(), ch.cpu().numpy(), max(natural_qcap(p, m, False) for m in ("level", "traj")))
        for cap in (0, 1, 40):
            for rows_cap in (0, 600):
                ref = E.full_bp(p, a, ch, max_it=cap, rows_cap=rows_cap, want_erased=True)
                out = E.full_bp_deg(p, a, cs, ch, max_it=cap, rows_cap=rows_cap, want_erased=True)
                torch.cuda.synchronize()
                _same(torch, ref, out, (dv, dc, eps, cap, rows_cap))
                if eps == 0.2 and rows_cap:
                    assert int(ref["rows"][:, 0, 0].min().item()) > 4096          # deg_1_iter of iteration 0


@pytest.mark.parametrize("dv,dc,eps", [(3, 6, 0.48), (5, 10, 0.49)])
def test_wide_deg_decoder_equals_the_first_generation_at_n_5000(E, dv, dc, eps):
    import torch
    p = E.make_params(dv, dc, 50, 5000)
    assert p.nk > 65536 and not E.full_bp_deg_supported(p) and E.full_bp_deg_supported(p, wide=True)
    for e in (eps, 0.2):
        a, cs, ch = _tables(E, p, 2024, 5, 16, e)
        cases = [(cap, rows_cap, True) for cap in (0, 40) for rows_cap in (0, 700)] + [(0, 700, False)]
        for cap, rows_cap, is_term in cases:
            ref = E.full_bp(p, a, ch, max_it=cap, is_term=is_term, rows_cap=rows_cap, want_erased=True)
            out = E.full_bp_deg(p, a, cs, ch, max_it=cap, is_term=is_term, rows_cap=rows_cap, want_erased=True, wide=True)
            torch.cuda.synchronize()
            _same(torch, ref, out, (dv, dc, e, cap, rows_cap, is_term))


@pytest.mark.parametrize("L,N", [(50, 1000), (16, 200)])
def test_4_8_through_the_deg_entry_points_is_the_sock16_and_wide_result(E, L, N):
    import torch
    p = E.make_params(4, 8, L, N)
    assert E.full_bp_deg_supported(p) and E.full_bp_deg_supported(p, wide=True)
    a, cs, ch = E.sample_philox_sock16(p, 91, 17, 32, 0.48)
    for is_term in (True, False):
        ref = E.full_bp_fixpoint_cn16(p, a, cs, ch, is_term=is_term, want_erased=True, sockets=True)
        out = E.full_bp_fixpoint_deg(p, a, cs, ch, is_term=is_term, want_erased=True)
        torch.cuda.synchronize()
        # column 5 of a fixpoint form counts the kernel's barrier rounds, which depend on how the waves interleave: two runs of
        # the same instance differ there
        cols = [0, 1, 2, 3, 4, 6, 7]
        assert torch.equal(ref["counters"][:, cols], out["counters"][:, cols]), ("fixpoint", L, N, is_term)
        assert torch.equal(ref["erased"], out["erased"]), ("fixpoint", L, N, is_term)
        for cap in (0, 3):
            for rows_cap in (0, 600):
                kw = dict(max_it=cap, is_term=is_term, want_erased=True, rows_cap=rows_cap)
                ref = E.full_bp_cn16(p, a, cs, ch, sockets=True, **kw)
                out = E.full_bp_deg(p, a, cs, ch, **kw)
                refw = E.full_bp_wide(p, a, cs, ch, **kw)
                outw = E.full_bp_deg(p, a, cs, ch, wide=True, **kw)
                torch.cuda.synchronize()
                _same(torch, ref, out, (L, N, is_term, cap, rows_cap))
                _same(torch, refw, outw, ("wide", L, N, is_term, cap, rows_cap))


@pytest.mark.parametrize("dv,dc,L,N", [(3, 6, 50, 1000), (5, 10, 50, 1000), (3, 6, 9, 24), (5, 10, 16, 200)])
def test_fixpoint_deg_equals_full_bp_fixpoint(E, dv, dc, L, N):
    import torch
    p = E.make_params(dv, dc, L, N)
    cols = [0, 1, 2, 3, 4, 7]                                            # column 5: barrier rounds of either kernel
    for eps in (0.3, 0.46, 0.49, 0.6):
        a, cs, ch = _tables(E, p, 13, 0, 16, eps)
        for is_term in (True, False):
            ref = E.full_bp_fixpoint(p, a, ch, is_term=is_term, want_erased=True)
            out = E.full_bp_fixpoint_deg(p, a, cs, ch, is_term=is_term, want_erased=True)
            torch.cuda.synchronize()
            assert torch.equal(ref["counters"][:, cols], out["counters"][:, cols]), (dv, dc, L, N, eps, is_term)
            assert torch.equal(ref["erased"], out["erased"]) and int(out["counters"][:, 6].abs().sum().item()) == 0


def _line(pair, wide=False, rows=False):
    return ("sampler (first generation) + cn_sockets pass + full_bp_small " + ("wide " if wide else "") +
            "level-synchronous (4-bit CN counts, dv = %d, dc = %d" % pair + (", 32-bit queue entries" if wide else "") +
            (", trajectory rows)" if rows else ")"))


@pytest.mark.parametrize("prog,dv,dc", [("bp_lim_iter", 3, 6), ("bp_traj", 5, 10)])
def test_cli_writes_the_same_files_on_the_deg_path(B, tmp_path, capfd, prog, dv, dc):
    texts = {}
    for mode in ("on", "off", "auto"):
        d = tmp_path / mode
        capfd.readouterr()
        argv = ["0", "0", "0", "200"] + (["1"] if prog == "bp_traj" else []) + [
            "--dv", str(dv), "--dc", str(dc), "--N", "200", "--L", "16", "--eps-ini", "0.47", "--num-points", "2",
            "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5", "--deg", mode, "--outdir", str(d)]
        getattr(B, prog)(argv)
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "kernels:" in ln]
        assert len(lines) == 1, lines
        named = _line((dv, dc), rows=prog == "bp_traj") in lines[0]
        assert named == (mode == "on" or (mode == "auto" and B.DEG_BY_DEFAULT)), (mode, lines[0])
        if not named:
            assert "sampler (first generation) + full_bp (16-bit CN words" in lines[0]
        files = sorted(os.listdir(d))
        assert len(files) == (2 if prog == "bp_traj" else 1)
        texts[mode] = [open(d / f).read() for f in files]
    assert texts["on"] == texts["off"] == texts["auto"] and all(len(t) > 100 for t in texts["on"])


def test_run_point_at_n_5000_counts_the_same_on_the_deg_path(B, E):
    import torch
    p = E.make_params(3, 6, 50, 5000)
    runs = []
    for deg in (True, False):
        sim = B.Simulator(p, decoder="full", max_it=200, batch=32, seed=8, device="cuda:0", deg=deg)
        assert sim.deg == deg and (sim.path.decoder == "degwide") == deg
        if deg:
            assert sim.kernel_choice() == _line((3, 6), wide=True)
        runs.append(dict(sim.run_point(0, 0.485, 64, 64).run))
    torch.cuda.synchronize()
    assert runs[0] == runs[1] and runs[0]["frames"] == 64
