"""Buffer contract of the device entry of include/scldpc_cov.h (-m gpu), as tests/test_gpu_buffer_contracts_unc.py keeps it for
include/scldpc_uncoupled.h: engine.r1_gram runs with engine._uninit replaced by a poison.Arena — its workspace filled with 0xFF,
with 0x5A, or with what a run on other rows left behind, between two guard zones — and the entry is called directly with
`gram` between guard zones of its own:
  * the result equals numpy's int64 Gram under each fill (the workspace's content on entry is irrelevant, the status word
    included), exactly;
  * no guard byte around the workspace or around gram changes;
  * d_r1 and d_steps are only read;
  * a batch split in two calls equals one call.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_cov_host import HEADER
from test_gpu_cov import np_gram, rows, steps_of, NCOLS
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu

# key -> (T, K): ragged in both (padding rows and columns of the panel are written, not found), and whole tiles and chunks
SHAPES = {"T45-K70": (45, 70), "T64-K64": (64, 64), "T300-K5": (300, 5)}


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the buffer-contract tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def test_the_file_covers_every_device_entry_of_the_header():
    assert header_device_entries(HEADER) == {"scldpc_r1_gram_device": ["d_gram", "d_ws"]}


@pytest.mark.parametrize("key", list(SHAPES))
def test_poisoned_workspace_and_red_zones(E, monkeypatch, key):
    import torch
    T, K = SHAPES[key]
    r1, steps = rows(T), steps_of(K)
    other = rows(T, seed=9, hi=1 << 20)
    want = np_gram(r1, steps)
    d_r1, d_other = torch.from_numpy(r1).cuda(), torch.from_numpy(other).cuda()
    d_steps = torch.from_numpy(steps.astype(np.int32)).cuda()
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            E.r1_gram(d_other, d_steps)                                  # other rows first
            synchronize()
            arena.check_guards()
            arena.recycle()
        got = E.r1_gram(d_r1, d_steps)
        synchronize()
        arena.check_guards()
        assert len(arena.records) == 1                                   # the workspace came out of the arena, and nothing else
        assert arena.records[0].nbytes == E.lib().scldpc_r1_gram_workspace_bytes(T, K)
        poison.assert_defined_equal((key, mode), got.cpu().numpy(), want)
        monkeypatch.undo()
    assert (d_r1.cpu().numpy() == r1).all() and (d_steps.cpu().numpy() == steps).all()      # inputs are only read


@pytest.mark.parametrize("key", list(SHAPES))
def test_gram_between_red_zones_and_a_batch_split_in_two(E, key):
    """The entry called directly: gram and the workspace between guard zones, the rows inside a larger allocation; one call
    over T trials and two calls over T1 + T2 trials accumulate the same sums on top of what gram held."""
    import torch
    T, K = SHAPES[key]
    r1, steps = rows(T), steps_of(K)
    want = np_gram(r1, steps)
    arena = poison.Arena(0x5A)
    d_rows = arena((T + 2, NCOLS), dtype=torch.int32, device="cuda:0")
    d_rows[1:T + 1] = torch.from_numpy(r1).cuda()
    d_steps = arena((K,), dtype=torch.int32, device="cuda:0")
    d_steps.copy_(torch.from_numpy(steps.astype(np.int32)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = E.lib()

    def call(gram, t0, n):
        nbytes = lib.scldpc_r1_gram_workspace_bytes(n, K)
        ws = arena(nbytes, dtype=torch.uint8, device="cuda:0")
        E.check(lib.scldpc_r1_gram_device(n, NCOLS, d_rows[1 + t0].data_ptr(), K, d_steps.data_ptr(), gram.data_ptr(),
                                          ws.data_ptr(), nbytes, stream))
        synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0                 # the status word: nothing was clamped
    base = 1000 + np.arange(3 * K * K, dtype=np.int64).reshape(3, K, K)
    one = arena((3, K, K), dtype=torch.int64, device="cuda:0")
    two = arena((3, K, K), dtype=torch.int64, device="cuda:0")
    one.copy_(torch.from_numpy(base))
    two.copy_(torch.from_numpy(base))
    call(one, 0, T)
    T1 = T // 3 + 1
    call(two, 0, T1)
    call(two, T1, T - T1)
    arena.check_guards()
    poison.assert_defined_equal((key, "one call"), one.cpu().numpy(), base + want)
    poison.assert_defined_equal((key, "two calls"), two.cpu().numpy(), base + want)
    edge = torch.cat([d_rows[:1], d_rows[T + 1:]]).cpu().numpy().view(np.uint8)
    assert (edge == 0x5A).all() and (d_rows[1:T + 1].cpu().numpy() == r1).all() and (d_steps.cpu().numpy() == steps).all()
