"""Buffer contract of the device entries of include/scldpc_eps.h (-m gpu), as tests/test_gpu_buffer_contracts_ss.py keeps it for
include/scldpc_ss.h: engine.channel_levels and engine.peel_sweep_eps run with engine._uninit replaced by a poison.Arena — the
levels, the rows, the lost bits and the workspace filled with 0xFF, with 0x5A, or with what a run on another grid left behind,
between two guard zones — with the CN words in LDS and in the workspace, and the entries are called directly with their outputs
between guard zones of their own:
  * the result equals engine.peel_sweep's (the sampler's channel words) under each fill, exactly, every element defined;
  * no guard byte around the levels, the rows, the lost bits or the workspace changes;
  * the adjacency and the levels are only read;
  * a batch split in two calls equals one call.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_eps_host import HEADER, WORKSPACE_M
from test_gpu_eps import SEED, SHAPES, T, assert_equals_peel_sweep, case, synchronize
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def test_the_file_covers_every_device_entry_of_the_header():
    assert header_device_entries(HEADER) == {
        "scldpc_channel_levels_device": ["d_levels"],
        "scldpc_peel_sweep_eps_device": ["d_out", "d_lost_bits", "d_workspace"],
        "scldpc_peel_sweep_eps_device_adj16": ["d_out", "d_lost_bits", "d_workspace"],
    }


def workspace_case(E):
    """(4,8), L = 50 with int32 rows at the smallest M whose CN words go to the workspace; four trials, three points."""
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    es, refs = [0.48, 0.46, 0.44], []
    for e in es:
        d_adj, d_ch = E.sample_philox(p, SEED, 0, 4, e)
        ref = E.peel_sweep(p, d_adj, d_ch, p.nk, 0, 0, p.nk, want_lost=True)
        refs.append((ref["out"].cpu().numpy(), ref["lost"].cpu().numpy().view(np.uint32)))
    d_lev = E.channel_levels(p, SEED, 0, 4, es)

    class G:
        total_size, lost_lo, lost_hi = p.nk, 0, p.nk
    return dict(p=p, g=G, es=es, d_adj=d_adj, d_lev=d_lev, refs=refs, adj=d_adj.cpu().numpy().copy(), lev=d_lev.cpu().numpy().copy())


@pytest.mark.parametrize("key", ["4-8-L12-M32", "5-10-L10-M40", "4-8-L12-M64-tb", "workspace"])
def test_poisoned_buffers_and_red_zones(E, monkeypatch, key):
    c = workspace_case(E) if key == "workspace" else case(E, key)
    p, g, K = c["p"], c["g"], len(c["es"])
    nt = c["d_adj"].shape[0]
    doped = () if key == "workspace" else SHAPES[key][6]
    other = [e + 0.03 for e in c["es"]]                                   # another grid and other draws first, in the stale mode
    nbytes = E.peel_sweep_eps_workspace_bytes(p, nt, c["d_adj"].element_size() == 2)
    assert (nbytes > 0) == (key == "workspace")
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            lev0 = E.channel_levels(p, SEED + 1, 0, nt, other, doped)
            E.peel_sweep_eps(p, c["d_adj"], lev0, K, g.total_size, g.lost_lo, g.lost_hi, want_lost=True)
            synchronize()
            arena.check_guards()
            arena.recycle()
        trial0 = 0 if key == "workspace" else 7
        lev = E.channel_levels(p, SEED, trial0, nt, c["es"], doped)
        got = E.peel_sweep_eps(p, c["d_adj"], lev, K, g.total_size, g.lost_lo, g.lost_hi, want_lost=True)
        synchronize()
        arena.check_guards()
        sizes = [r.nbytes for r in arena.records]
        want_sizes = [nt * p.n, K * nt * 32, K * nt * p.nw * 4] + ([nbytes] if nbytes else [])
        assert sizes == want_sizes, (sizes, want_sizes)                  # the levels, the rows, the lost bits, the workspace
        poison.assert_defined_equal((key, mode, "levels"), lev.cpu().numpy(), c["lev"])
        assert_equals_peel_sweep(c, got, (key, mode))
        monkeypatch.undo()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_lev"].cpu().numpy() == c["lev"]).all()   # inputs are only read


@pytest.mark.parametrize("key", ["4-8-L12-M32", "4-8-L12-M64-proto"])
def test_outputs_between_red_zones_and_a_batch_split_in_two(E, key):
    """The entries called directly: outputs between guard zones, the inputs inside larger allocations; one call over T trials and
    two calls over T1 + T2 write the same levels and, point by point, the same rows and lost bits."""
    import torch
    c = case(E, key)
    p, g, es, K = c["p"], c["g"], c["es"], len(c["es"])
    doped = SHAPES[key][6]
    a16 = c["d_adj"].dtype == torch.int16
    lib = E.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arena = poison.Arena(0x5A)
    d_rows = arena((T + 2,) + tuple(c["d_adj"].shape[1:]), dtype=c["d_adj"].dtype, device="cuda:0")
    d_rows[1:T + 1] = c["d_adj"]
    eps = np.ascontiguousarray(es, dtype=np.float64)
    darr = np.ascontiguousarray(doped, dtype=np.int32)

    def levels_call(buf, t0, n):
        E.check(lib.scldpc_channel_levels_device(C.byref(p), SEED, 7 + t0, n, K, eps.ctypes.data, darr.size,
                                                 darr.ctypes.data if darr.size else None, buf[t0].data_ptr(), stream))
    T1 = T // 3 + 1
    lev_one = arena((T, p.n), dtype=torch.uint8, device="cuda:0")
    lev_two = arena((T + 2, p.n), dtype=torch.uint8, device="cuda:0")     # the decoder's input inside a larger allocation
    levels_call(lev_one, 0, T)
    levels_call(lev_two[1:], 0, T1)
    levels_call(lev_two[1:], T1, T - T1)
    synchronize()
    arena.check_guards()
    poison.assert_defined_equal("levels, one call", lev_one.cpu().numpy(), c["lev"])
    poison.assert_defined_equal("levels, two calls", lev_two[1:T + 1].cpu().numpy(), c["lev"])
    assert (lev_two[[0, T + 1]].cpu().numpy() == 0x5A).all()

    fn = lib.scldpc_peel_sweep_eps_device_adj16 if a16 else lib.scldpc_peel_sweep_eps_device

    def sweep_call(t0, n, want_lost=True):
        out = arena((K, n, 8), dtype=torch.int32, device="cuda:0")
        lost = arena((K, n, p.nw), dtype=torch.int32, device="cuda:0") if want_lost else None
        E.check(fn(C.byref(p), n, d_rows[1 + t0].data_ptr(), lev_two[1 + t0].data_ptr(), K, g.total_size, g.lost_lo, g.lost_hi,
                   out.data_ptr(), lost.data_ptr() if lost is not None else None, None, 0, stream))
        synchronize()
        return out, lost
    one = sweep_call(0, T)
    first, second = sweep_call(0, T1), sweep_call(T1, T - T1)
    bare, none = sweep_call(0, T, want_lost=False)
    arena.check_guards()
    assert none is None and (bare == one[0]).all()
    assert_equals_peel_sweep(c, {"out": one[0], "lost": one[1]}, "one call")
    two = {"out": torch.cat([first[0], second[0]], dim=1), "lost": torch.cat([first[1], second[1]], dim=1)}
    assert_equals_peel_sweep(c, two, "two calls")
    for d_big, d_in in ((d_rows, c["d_adj"]),):
        edge = torch.cat([d_big[:1], d_big[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all() and (d_big[1:T + 1] == d_in).all()
    assert (lev_two[1:T + 1].cpu().numpy() == c["lev"]).all()            # the levels are only read
