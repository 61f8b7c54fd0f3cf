"""Buffer contract of the device entries of include/scldpc_thresh.h (-m gpu), as tests/test_gpu_buffer_contracts_bp_eps.py
keeps it for include/scldpc_bp_eps.h: engine.channel_keys and engine.frame_threshold run with engine._uninit replaced by a
poison.Arena — the keys, the rows, the bits and the workspace filled with 0xFF, with 0x5A, or with what a run on other draws and
another window left behind, between two guard zones — with the CN words in LDS and in the workspace, and the entries are called
directly with their outputs between guard zones of their own:
  * the keys and the result equal the references of tests/test_gpu_thresh.py under each fill, exactly, every element defined;
  * no guard byte around the keys, the rows, the bits or the workspace changes;
  * the adjacency and the keys are only read;
  * d_bits = NULL leaves the rows unchanged, and a batch split in two calls equals one call.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_gpu_bp_eps import SEED
from test_gpu_thresh import COLS, T, TRIAL0, assert_equals_host, case, synchronize, workspace_case
from test_thresh_host import HEADER
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def test_the_file_covers_every_device_entry_of_the_header():
    assert header_device_entries(HEADER) == {
        "scldpc_channel_keys_device": ["d_keys"],
        "scldpc_frame_threshold_device": ["d_rows", "d_bits", "d_workspace"],
        "scldpc_frame_threshold_device_adj16": ["d_rows", "d_bits", "d_workspace"],
    }


@pytest.mark.parametrize("key", ["4-8-L12-N16", "3-6-L10-N20-open", "3-6-L11-N18", "4-8-L12-N64-doped3", "workspace"])
def test_poisoned_buffers_and_red_zones(E, monkeypatch, key):
    c = workspace_case(E) if key == "workspace" else case(E, key)
    p = c["p"]
    nt = c["d_adj"].shape[0]
    trial0 = 0 if key == "workspace" else TRIAL0
    nbytes = E.frame_threshold_workspace_bytes(p, nt, c["d_adj"].element_size() == 2)
    assert (nbytes > 0) == (key == "workspace")
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":                                              # other draws and another window first
            keys0 = E.channel_keys(p, SEED + 1, 0, nt, c["doped"])
            E.frame_threshold(p, c["d_adj"], keys0, c["t_lo"] // 2, c["t_hi"] + 1000, is_term=c["is_term"], want_bits=True)
            synchronize()
            arena.check_guards()
            arena.recycle()
        d_keys = E.channel_keys(p, SEED, trial0, nt, c["doped"])
        got = E.frame_threshold(p, c["d_adj"], d_keys, c["t_lo"], c["t_hi"], is_term=c["is_term"], want_bits=True)
        synchronize()
        arena.check_guards()
        sizes = [r.nbytes for r in arena.records]
        want_sizes = [nt * p.n * 4, nt * 32, nt * p.nw * 4] + ([nbytes] if nbytes else [])
        assert sizes == want_sizes, (sizes, want_sizes)                  # the keys, the rows, the bits, the workspace
        poison.assert_defined_equal((key, mode, "keys"), d_keys.cpu().numpy().view(np.uint32), c["keys"])
        poison.assert_defined_equal((key, mode, "rows"), got["rows"].cpu().numpy()[:, COLS].astype(np.int64), c["rows"])
        poison.assert_defined_equal((key, mode, "bits"), got["bits"].cpu().numpy().view(np.uint32), c["bits"])
        assert_equals_host(c, got, (key, mode))
        monkeypatch.undo()
    assert (c["d_adj"].cpu().numpy() == c["adj"]).all() and (c["d_keys"].cpu().numpy().view(np.uint32) == c["keys"]).all()


@pytest.mark.parametrize("key", ["4-8-L12-N16", "4-8-L12-N16-int32"])
def test_outputs_between_red_zones_and_a_batch_split_in_two(E, key):
    """The entries called directly: outputs between guard zones, the inputs inside larger allocations; one call over T frames and
    two calls over T1 + T2 write the same rows and bits; without d_bits the rows are the same."""
    import torch
    c = case(E, key)
    p = c["p"]
    a16 = c["d_adj"].dtype == torch.int16
    lib = E.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arena = poison.Arena(0x5A)
    d_code = arena((T + 2,) + tuple(c["d_adj"].shape[1:]), dtype=c["d_adj"].dtype, device="cuda:0")
    d_code[1:T + 1] = c["d_adj"]
    d_keys = arena((T + 2, p.n), dtype=torch.int32, device="cuda:0")      # the decoder's inputs inside larger allocations
    d_keys[1:T + 1] = c["d_keys"]
    T1 = T // 3 + 1
    fn = lib.scldpc_frame_threshold_device_adj16 if a16 else lib.scldpc_frame_threshold_device

    def call(t0, n, want_bits=True):
        rows = arena((n, 8), dtype=torch.int32, device="cuda:0")
        bits = arena((n, p.nw), dtype=torch.int32, device="cuda:0") if want_bits else None
        E.check(fn(C.byref(p), n, d_code[1 + t0].data_ptr(), d_keys[1 + t0].data_ptr(), c["t_lo"], c["t_hi"], 1, rows.data_ptr(),
                   bits.data_ptr() if bits is not None else None, None, 0, stream))
        synchronize()
        return rows, bits
    one = call(0, T)
    first, second = call(0, T1), call(T1, T - T1)
    bare, none = call(0, T, want_bits=False)
    # the keys entry, its output between guard zones: the rows of the frames in the middle only
    out = arena((T + 2, p.n), dtype=torch.int32, device="cuda:0")
    E.check(lib.scldpc_channel_keys_device(C.byref(p), SEED, TRIAL0, T, 0, None, out[1].data_ptr(), stream))
    synchronize()
    arena.check_guards()
    assert (out[1:T + 1] == c["d_keys"]).all()
    assert (torch.cat([out[:1], out[T + 1:]]).cpu().numpy().view(np.uint8) == 0x5A).all()
    assert none is None and (bare[:, COLS] == one[0][:, COLS]).all()     # d_bits = NULL leaves the rows unchanged
    assert_equals_host(c, {"rows": one[0], "bits": one[1]}, "one call")
    two = {"rows": torch.cat([first[0], second[0]]), "bits": torch.cat([first[1], second[1]])}
    assert_equals_host(c, two, "two calls")
    for d_big, d_in in ((d_code, c["d_adj"]), (d_keys, c["d_keys"])):
        edge = torch.cat([d_big[:1], d_big[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all() and (d_big[1:T + 1] == d_in).all()   # the inputs are only read
