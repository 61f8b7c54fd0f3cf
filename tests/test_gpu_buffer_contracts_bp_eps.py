"""Buffer contract of the device entries of include/scldpc_bp_eps.h (-m gpu), as tests/test_gpu_buffer_contracts_eps.py keeps it
for include/scldpc_eps.h: engine.full_bp_eps runs with engine._uninit replaced by a poison.Arena — the counters, the erased bits
and the workspace filled with 0xFF, with 0x5A, or with what a run on another grid left behind, between two guard zones — with the
CN words in LDS and in the workspace, and the entries are called directly with their outputs between guard zones of their own:
  * the result equals engine.full_bp's (the sampler's channel words, no iteration cap) under each fill, exactly, every element
    defined;
  * no guard byte around the counters, the erased bits or the workspace changes;
  * the adjacency and the levels are only read;
  * a batch split in two calls equals one call.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_bp_eps_host import HEADER
from test_eps_host import WORKSPACE_M
from test_gpu_bp_eps import SEED, SHAPES, T, assert_equals_full_bp, case, reference, synchronize
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def test_the_file_covers_every_device_entry_of_the_header():
    assert header_device_entries(HEADER) == {
        "scldpc_full_bp_eps_device": ["d_counters", "d_erased_bits", "d_workspace"],
        "scldpc_full_bp_eps_device_adj16": ["d_counters", "d_erased_bits", "d_workspace"],
    }


def workspace_case(E):
    """(4,8), L = 50 with int32 rows where the CN words go to the workspace; four trials, three points."""
    p = E.make_params(4, 8, 50, WORKSPACE_M)
    es = [0.48, 0.46, 0.44]
    d_adj, chans, refs = reference(E, p, es, 4, 0, True, False, ())
    d_lev = E.channel_levels(p, SEED, 0, 4, es)
    synchronize()
    return dict(p=p, es=es, is_term=True, d_adj=d_adj, d_lev=d_lev, refs=refs, adj=d_adj.cpu().numpy().copy(),
                lev=d_lev.cpu().numpy().copy())


@pytest.mark.parametrize("key", ["4-8-L12-N16", "3-6-L10-N20-open", "5-10-L10-N20", "workspace"])
def test_poisoned_buffers_and_red_zones(E, monkeypatch, key):
    c = workspace_case(E) if key == "workspace" else case(E, key)
    p, K = c["p"], len(c["es"])
    nt = c["d_adj"].shape[0]
    doped = () if key == "workspace" else SHAPES[key][6]
    other = [e + 0.03 for e in c["es"]]                                   # another grid and other draws first, in the stale mode
    nbytes = E.full_bp_eps_workspace_bytes(p, nt, c["d_adj"].element_size() == 2)
    assert (nbytes > 0) == (key == "workspace")
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            lev0 = E.channel_levels(p, SEED + 1, 0, nt, other, doped)
            E.full_bp_eps(p, c["d_adj"], lev0, K, is_term=c["is_term"], want_erased=True)
            synchronize()
            arena.check_guards()
            arena.recycle()
        trial0 = 0 if key == "workspace" else 7
        lev = E.channel_levels(p, SEED, trial0, nt, c["es"], doped)
        got = E.full_bp_eps(p, c["d_adj"], lev, K, is_term=c["is_term"], want_erased=True)
        synchronize()
        arena.check_guards()
        sizes = [r.nbytes for r in arena.records]
        want_sizes = [nt * p.n, K * nt * 32, K * nt * p.nw * 4] + ([nbytes] if nbytes else [])
        assert sizes == want_sizes, (sizes, want_sizes)                  # the levels, the counters, the erased bits, the workspace
        poison.assert_defined_equal((key, mode, "levels"), lev.cpu().numpy(), c["lev"])
        poison.assert_defined_equal((key, mode, "counters"), got["counters"].cpu().numpy()[:, :, [0, 1, 2, 3, 4, 6, 7]],
                                    np.stack([r[0] for r in c["refs"]])[:, :, [0, 1, 2, 3, 4, 6, 7]])
        assert_equals_full_bp(c, got, (key, mode))
        monkeypatch.undo()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_lev"].cpu().numpy() == c["lev"]).all()   # inputs are only read


@pytest.mark.parametrize("key", ["4-8-L12-N16", "4-8-L12-N16-int32"])
def test_outputs_between_red_zones_and_a_batch_split_in_two(E, key):
    """The entries called directly: outputs between guard zones, the inputs inside larger allocations; one call over T trials and
    two calls over T1 + T2 write, point by point, the same counters and erased bits."""
    import torch
    c = case(E, key)
    p, K = c["p"], len(c["es"])
    a16 = c["d_adj"].dtype == torch.int16
    lib = E.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arena = poison.Arena(0x5A)
    d_rows = arena((T + 2,) + tuple(c["d_adj"].shape[1:]), dtype=c["d_adj"].dtype, device="cuda:0")
    d_rows[1:T + 1] = c["d_adj"]
    d_lev = arena((T + 2, p.n), dtype=torch.uint8, device="cuda:0")       # the decoder's inputs inside larger allocations
    d_lev[1:T + 1] = c["d_lev"]
    T1 = T // 3 + 1
    fn = lib.scldpc_full_bp_eps_device_adj16 if a16 else lib.scldpc_full_bp_eps_device

    def call(t0, n, want_erased=True):
        cnt = arena((K, n, 8), dtype=torch.int32, device="cuda:0")
        bits = arena((K, n, p.nw), dtype=torch.int32, device="cuda:0") if want_erased else None
        E.check(fn(C.byref(p), n, d_rows[1 + t0].data_ptr(), d_lev[1 + t0].data_ptr(), K, 1, cnt.data_ptr(),
                   bits.data_ptr() if bits is not None else None, None, 0, stream))
        synchronize()
        return cnt, bits
    one = call(0, T)
    first, second = call(0, T1), call(T1, T - T1)
    bare, none = call(0, T, want_erased=False)
    arena.check_guards()
    assert none is None and (bare[:, :, [0, 1, 2, 3, 4, 6, 7]] == one[0][:, :, [0, 1, 2, 3, 4, 6, 7]]).all()
    assert_equals_full_bp(c, {"counters": one[0], "erased": one[1]}, "one call")
    two = {"counters": torch.cat([first[0], second[0]], dim=1), "erased": torch.cat([first[1], second[1]], dim=1)}
    assert_equals_full_bp(c, two, "two calls")
    for d_big, d_in in ((d_rows, c["d_adj"]), (d_lev, c["d_lev"])):
        edge = torch.cat([d_big[:1], d_big[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all() and (d_big[1:T + 1] == d_in).all()   # the inputs are only read
