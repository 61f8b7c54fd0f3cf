"""Every form of the first-generation flooding decoders (-m gpu) at the smallest shapes that still take it: CN-word policy
(16-bit packed, 32-bit in LDS, 32-bit in the workspace) x adjacency width (4-byte global ids, 2-byte position-local ids) x the
dv = 4 and the generic-dv code, for full_bp (level-synchronous and fixpoint), sw_bp (square and classical window, whole-chain
kernel), and peel_sweep — counters, trajectory rows and erased / lost bits against the CPU oracles, exactly.  Which policy a shape
takes is host arithmetic and asserted first (workspace bytes, LDS bytes); the workspace shapes with the 2-byte table run with
the CN words prebuilt through cn_build.hip and with the kernels' own build."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

W, SW_IT, SW_INIT = 3, 4, 7
# (dv, dc, L, N, eps, trials): what it takes — (scldpc_full_bp_lds_bytes, CN words in the workspace)
SHAPES = {
    (4, 8, 9, 24, 0.44, 3): (66048, False),         # packed, ragged n (216 VNs: the last channel word is partial)
    (3, 6, 14, 60, 0.44, 3): (66864, False),        # packed, generic dv
    (4, 8, 6, 1200, 0.50, 3): (88864, False),       # dv * vns_pos > 4096: 32-bit words in LDS
    (3, 6, 6, 1400, 0.50, 3): (89824, False),       # … generic dv
    (4, 8, 5, 9600, 0.30, 2): (76464, True),       # 32-bit words beyond the LDS: workspace (all three kernels from N = 9530 on)
    (3, 6, 6, 9600, 0.30, 2): (77664, True),       # … generic dv (from N = 9462 on)
}


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """Inputs (host replay of the reference's sampler) and every oracle result of a shape, computed once."""
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    from oracle import pd_oracle as P
    dv, dc, L, N, eps, T = shape
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    adj, ch = E.sample_glibc_trials(p, [1000 + 17 * t for t in range(T)], eps)
    bits = E.unpack_bits(ch, p.n)
    ref = []
    for t in range(T):
        g = O.Graph.from_vn_adj(po, adj[t])
        r = {}
        for is_term in (1, 0):
            for max_it in (0, 3):
                r["bp", is_term, max_it] = O.decode_bp(g, bits[t], max_it=max_it, is_term=is_term, literal=False, rows_cap=512)
        for classical in (False, True):
            # (the literal message-passing decoder is the only one with the classical window; the square one has a fast twin)
            r["sw", classical] = O.decode_sw(g, bits[t], W, SW_IT, 0 if classical else SW_INIT, literal=classical or p.n < 10000,
                                             square=not classical)
        tr, mask = adj[t].astype(np.int64), bits[t].astype(bool)
        for total, start, lo, hi in _sweep_ranges(p):
            alive = P.peel_closure(tr, mask, total, start)
            lost = alive & ((tr >= lo) & (tr < hi)).any(axis=1) & (tr < total).all(axis=1)
            sizes, comp, idx = P.components(tr, lost)
            big = sizes[comp] > 2 if len(idx) else np.zeros(0, dtype=bool)
            r["pd", total, start] = (int(lost.sum()), int(sizes[sizes > 2].sum()),
                                     int(len(np.unique((tr[idx, 0] // p.cns_pos)[big]))), lost)
        ref.append(r)
    return p, adj, ch, bits, ref


def _sweep_ranges(p):
    """(total_size, sweep_start, lost_lo, lost_hi): the terminated, bounded chain; and a truncated one swept from position 1 on
    (CNs of position 0 that hold one VN from the outset never fire) that reports positions 1 .. L-2."""
    return ((p.nk, 0, 0, p.nk), (p.L * p.cns_pos, p.cns_pos, p.cns_pos, (p.L - 1) * p.cns_pos))


@pytest.mark.parametrize("shape", list(SHAPES), ids=["%d_%d_L%d_N%d" % s[:4] for s in SHAPES])
def test_every_form_equals_the_cpu_oracles(E, monkeypatch, shape):
    import torch
    from fl_scaling_sc_ldpc_amd import _lib
    lds_bytes, in_workspace = SHAPES[shape]
    p, adj, ch, bits, ref = _reference(shape)
    T = shape[5]
    L = _lib.lib()
    assert L.scldpc_full_bp_lds_bytes(C.byref(p)) == lds_bytes
    for op, arg in ((1, 0), (1, 1), (2, W), (3, 0), (3, 1)):            # SCLDPC_WS_FULL_BP, _SW_BP, _PEEL_SWEEP
        assert L.scldpc_workspace_bytes(op, C.byref(p), T, arg, 0) == (T * p.nk * 4 if in_workspace else 0), (op, arg)
    ran_failed = ran_clean = 0
    for adj16 in (False, True):
        assert p.cns_pos <= 65536
        d_adj, d_ch = E.to_device(E.global_to_adj16(p, adj) if adj16 else adj, ch)
        for prebuild in (("1", "0") if in_workspace and adj16 else (None,)):
            if prebuild is not None:
                for name in ("FULLBP", "SW", "SWEEP"):
                    monkeypatch.setenv("SCLDPC_DEBUG_%s_PREBUILD" % name, prebuild)
            what = (shape, adj16, prebuild)
            for is_term in (1, 0):
                for max_it in (0, 3):
                    out = E.full_bp(p, d_adj, d_ch, max_it=max_it, is_term=bool(is_term), rows_cap=512, want_erased=True)
                    plain = E.full_bp(p, d_adj, d_ch, max_it=max_it, is_term=bool(is_term))     # the kernels without rows
                    c, rows = out["counters"].cpu().numpy(), out["rows"].cpu().numpy()
                    er = E.unpack_bits(out["erased"].cpu().numpy(), p.n)
                    assert (plain["counters"].cpu().numpy() == c).all(), what
                    for t in range(T):
                        res, erased, orows = ref[t]["bp", is_term, max_it]
                        assert c[t].tolist() == [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"],
                                                 res["num_blocks_err_exp"], 0, res["iterations"], 0, bits[t].sum()], (what, t)
                        assert (er[t] == erased).all(), (what, t)
                        got = rows[t, :res["iterations"]]
                        assert (got[:, 0] == orows["deg1"]).all() and (got[:, 1] == orows["recovered"]).all() \
                            and (got[:, 2] == orows["first_pos"]).all(), (what, is_term, max_it, t)
                        ran_failed += res["num_erasures"] > 0
                        ran_clean += res["num_erasures"] == 0
                fix = E.full_bp_fixpoint(p, d_adj, d_ch, is_term=bool(is_term), want_erased=True)
                c, er = fix["counters"].cpu().numpy(), E.unpack_bits(fix["erased"].cpu().numpy(), p.n)
                for t in range(T):
                    res, erased, _ = ref[t]["bp", is_term, 0]
                    assert c[t, [0, 1, 2, 3, 4, 6, 7]].tolist() == [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"],
                                                                    res["num_blocks_err_exp"], 0, 0, bits[t].sum()], (what, t)
                    assert (er[t] == erased).all(), (what, t)
            for classical in (False, True):
                out = E.sw_bp(p, d_adj, d_ch, W, SW_IT, 0 if classical else SW_INIT, want_erased=True, classical=classical, ring=False)
                c, er = out["counters"].cpu().numpy(), E.unpack_bits(out["erased"].cpu().numpy(), p.n)
                for t in range(T):
                    res, erased = ref[t]["sw", classical]
                    assert c[t].tolist() == [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"],
                                             res["num_blocks_err_exp"], res["num_erasures_p1"], res["iterations"], 0,
                                             bits[t].sum()], (what, classical, t)
                    assert (er[t] == erased).all(), (what, classical, t)
            for total, start, lo, hi in _sweep_ranges(p):
                out = E.peel_sweep(p, d_adj, d_ch, total, start, lo, hi, want_lost=True)
                o, lost = out["out"].cpu().numpy(), E.unpack_bits(out["lost"].cpu().numpy(), p.n)
                for t in range(T):
                    n_lost, n_exp, blocks, lost_ref = ref[t]["pd", total, start]
                    assert o[t, [0, 1, 2, 7]].tolist() == [n_lost, n_exp, blocks, bits[t].sum()], (what, total, t)
                    assert (lost[t].astype(bool) == lost_ref).all(), (what, total, t)
        torch.cuda.synchronize()
    assert ran_failed and ran_clean, "the shape's trials should both fail and succeed"
