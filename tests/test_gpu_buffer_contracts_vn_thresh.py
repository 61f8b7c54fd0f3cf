"""Buffer contract of the device entries of include/scldpc_vn_thresh.h (-m gpu), as tests/test_gpu_buffer_contracts_thresh.py
keeps it for include/scldpc_thresh.h: engine.vn_threshold runs with engine._uninit replaced by a poison.Arena — the rows, the
position thresholds, the counts, tau and the workspace filled with 0xFF, with 0x5A, or with what a run on other keys and
another window left behind, between two guard zones — with the CN words in LDS and in the workspace, and the entries are called
directly with their outputs between guard zones of their own:
  * the result equals the reference of tests/test_gpu_vn_thresh.py under each fill, exactly, every element defined;
  * no guard byte around the rows, the position thresholds, the counts, tau or the workspace changes;
  * the adjacency and the keys are only read;
  * d_tau = NULL and d_counts = NULL (no grid) leave the other outputs unchanged, and a batch split in two calls equals one call.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_eps_host import WORKSPACE_M
from test_gpu_vn_thresh import COLS, SEED, T, assert_equals_reference, case, grid_of, host_reference, synchronize, unsigned
from test_uncoupled_host import header_device_entries
from test_vn_thresh_host import HEADER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def test_the_file_covers_every_device_entry_of_the_header():
    outs = ["d_rows", "d_pos_thresh", "d_counts", "d_tau", "d_workspace"]
    assert header_device_entries(HEADER) == {"scldpc_vn_threshold_device": outs, "scldpc_vn_threshold_device_adj16": outs}


def workspace_case(E):
    """(4,8), L = 50 with int32 rows where the CN words go to the workspace; two frames, window [0.47, 0.48]."""
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    nt = 2
    t_lo, t_hi = E.erasure_threshold(0.47), E.erasure_threshold(0.48)
    d_adj, _ch = E.sample_philox(p, SEED, 0, nt, 0.48)
    d_keys = E.channel_keys(p, SEED, 0, nt)
    synchronize()
    adj, keys = d_adj.cpu().numpy().copy(), d_keys.cpu().numpy().view(np.uint32).copy()
    grid = grid_of(t_lo, t_hi, 64)
    return dict(p=p, is_term=True, doped=(), t_lo=t_lo, t_hi=t_hi, d_adj=d_adj, d_keys=d_keys, adj=adj, keys=keys, grid=grid,
                ref=host_reference(p, adj, keys, t_lo, t_hi, True, grid))


@pytest.mark.parametrize("key", ["4-8-L12-N16", "3-6-L10-N20-open", "3-6-L11-N18", "4-8-L12-N64-doped3", "workspace"])
def test_poisoned_buffers_and_red_zones(E, monkeypatch, key):
    c = workspace_case(E) if key == "workspace" else case(E, key)
    p, ref = c["p"], c["ref"]
    nt, K = c["d_adj"].shape[0], len(c["grid"])
    nbytes = E.vn_threshold_workspace_bytes(p, nt, c["d_adj"].element_size() == 2)
    assert (nbytes > 0) == (key == "workspace")
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":                                              # other keys and another window first
            keys0 = E.channel_keys(p, SEED + 1, 0, nt, c["doped"])
            E.vn_threshold(p, c["d_adj"], keys0, c["t_lo"] // 2, c["t_hi"] + 1000, grid=[g + 500 for g in c["grid"]],
                           is_term=c["is_term"], want_tau=True)
            synchronize()
            arena.check_guards()
            arena.recycle()
        got = E.vn_threshold(p, c["d_adj"], c["d_keys"], c["t_lo"], c["t_hi"], grid=c["grid"], is_term=c["is_term"], want_tau=True)
        synchronize()
        arena.check_guards()
        sizes = [r.nbytes for r in arena.records]
        want_sizes = [nt * 32, nt * p.L * 4, nt * K * 4, nt * p.n * 4] + ([nbytes] if nbytes else [])
        assert sizes == want_sizes, (sizes, want_sizes)                  # the rows, the positions, the counts, tau, the workspace
        poison.assert_defined_equal((key, mode, "rows"), got["rows"].cpu().numpy()[:, COLS].astype(np.int64), ref["rows"])
        poison.assert_defined_equal((key, mode, "pos"), unsigned(got["pos_thresh"]), ref["pos"])
        poison.assert_defined_equal((key, mode, "counts"), got["counts"].cpu().numpy().astype(np.int64), ref["counts"])
        poison.assert_defined_equal((key, mode, "tau"), unsigned(got["tau"]), ref["tau"])
        assert_equals_reference(ref, got, (key, mode))
        monkeypatch.undo()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_keys"].cpu().numpy().view(np.uint32) == c["keys"]).all()


@pytest.mark.parametrize("key", ["4-8-L12-N16", "4-8-L12-N16-int32"])
def test_outputs_between_red_zones_and_a_batch_split_in_two(E, key):
    """The entries called directly: outputs between guard zones, the inputs inside larger allocations; one call over T frames and
    two calls over T1 + T2 write the same outputs; without d_tau, and without a grid and d_counts, the others are the same."""
    import torch
    c = case(E, key)
    p, ref = c["p"], c["ref"]
    a16 = c["d_adj"].dtype == torch.int16
    lib = E.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arena = poison.Arena(0x5A)
    d_code = arena((T + 2,) + tuple(c["d_adj"].shape[1:]), dtype=c["d_adj"].dtype, device="cuda:0")
    d_code[1:T + 1] = c["d_adj"]
    d_keys = arena((T + 2, p.n), dtype=torch.int32, device="cuda:0")      # the decoder's inputs inside larger allocations
    d_keys[1:T + 1] = c["d_keys"]
    T1 = T // 3 + 1
    fn = lib.scldpc_vn_threshold_device_adj16 if a16 else lib.scldpc_vn_threshold_device
    grid = np.ascontiguousarray(c["grid"], dtype=np.uint32)

    def call(t0, n, want_tau=True, want_counts=True):
        K = grid.size if want_counts else 0
        out = {"rows": arena((n, 8), dtype=torch.int32, device="cuda:0"), "pos_thresh": arena((n, p.L), dtype=torch.int32, device="cuda:0"),
               "counts": arena((n, K), dtype=torch.int32, device="cuda:0") if K else None,
               "tau": arena((n, p.n), dtype=torch.int32, device="cuda:0") if want_tau else None}
        ptr = lambda t: t.data_ptr() if t is not None else None
        E.check(fn(C.byref(p), n, d_code[1 + t0].data_ptr(), d_keys[1 + t0].data_ptr(), c["t_lo"], c["t_hi"], 1, K,
                   grid.ctypes.data if K else None, ptr(out["rows"]), ptr(out["pos_thresh"]), ptr(out["counts"]), ptr(out["tau"]),
                   None, 0, stream))
        synchronize()
        return out
    one = call(0, T)
    first, second = call(0, T1), call(T1, T - T1)
    no_tau, no_counts = call(0, T, want_tau=False), call(0, T, want_counts=False)
    arena.check_guards()
    assert_equals_reference(ref, one, "one call")
    two = {k: torch.cat([first[k], second[k]]) for k in one}
    assert_equals_reference(ref, two, "two calls")
    assert no_tau["tau"] is None
    assert_equals_reference(ref, no_tau, "d_tau = NULL")
    assert_equals_reference(ref, no_counts, "no grid, d_counts = NULL", counts=ref["counts"][:, :0])
    for d_big, d_in in ((d_code, c["d_adj"]), (d_keys, c["d_keys"])):
        edge = torch.cat([d_big[:1], d_big[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all() and (d_big[1:T + 1] == d_in).all()   # the inputs are only read
