"""Buffer contract of the device entry of include/scldpc_ss.h (-m gpu), as tests/test_gpu_buffer_contracts_cov.py keeps it for
include/scldpc_cov.h: engine.ss_spectrum runs with engine._uninit replaced by a poison.Arena — its workspace and its `trial`
rows filled with 0xFF, with 0x5A, or with what a run on other members left behind, between two guard zones — with the
union-find state in LDS and in the workspace, and the entry is called directly with d_hist, d_pos_hist and d_trial between guard
zones of their own:
  * the result equals the oracle's under each fill (the workspace's content on entry is irrelevant, the status word
    included), exactly;
  * no guard byte around the workspace, the rows or the histograms changes;
  * the adjacency and the member bits are only read;
  * a batch split in two calls equals one call.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_gpu_ss import NBINS, SHAPES, graphs, members_of, reference, to_adj16, upload
from test_ss_host import FORCE, HEADER
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu
KEYS = ["3-6-olmos", "4-8-olmos", "3-6-tb-L1"]


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
    assert header_device_entries(HEADER) == {"scldpc_ss_spectrum_device": ["d_hist", "d_pos_hist", "d_trial", "d_ws"]}


def inputs(E, oracle, key, adj16):
    dv, dc, L, M, rho, ens, T = SHAPES[key]
    p, trs = graphs(E, oracle, dv, dc, L, M, ens, T)
    mem = members_of(p.n, rho, T)
    want = reference((key, rho), trs, mem, p)
    rows = to_adj16(p, trs) if adj16 else trs
    d_adj, d_m = upload(E, rows, mem)
    return p, rows, mem, want, d_adj, d_m


@pytest.mark.parametrize("force", [False, True], ids=["lds", "workspace"])
@pytest.mark.parametrize("key", KEYS)
def test_poisoned_workspace_and_red_zones(E, oracle, monkeypatch, key, force):
    p, rows, mem, want, d_adj, d_m = inputs(E, oracle, key, adj16=(key == "4-8-olmos"))
    T = len(rows)
    _, d_other = upload(E, rows, members_of(p.n, 0.5, T + 1)[1:])         # other members first, in the stale mode
    for mode in poison.MODES:
        if force:
            monkeypatch.setenv(FORCE, "1")
        else:
            monkeypatch.delenv(FORCE, raising=False)
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            E.ss_spectrum(p, d_adj, d_other, NBINS, want_trial=True)
            synchronize()
            arena.check_guards()
            arena.recycle()
        got = E.ss_spectrum(p, d_adj, d_m, NBINS, want_trial=True)
        synchronize()
        arena.check_guards()
        assert len(arena.records) == 2                                   # the workspace and the rows, and nothing else
        nbytes = E.lib().scldpc_ss_spectrum_workspace_bytes(C.byref(p), T)
        assert arena.records[0].nbytes == nbytes and (nbytes > 256) == force and arena.records[1].nbytes == 16 * T
        for name, w in zip(("hist", "pos_hist", "trial"), want):
            poison.assert_defined_equal((key, mode, name), got[name].cpu().numpy(), w)
        monkeypatch.undo()
    assert (d_adj.cpu().numpy() == rows).all()                           # inputs are only read
    assert (E.unpack_bits(d_m.cpu().numpy(), p.n).astype(bool) == mem).all()


@pytest.mark.parametrize("force", [False, True], ids=["lds", "workspace"])
def test_outputs_between_red_zones_and_a_batch_split_in_two(E, oracle, monkeypatch, force):
    """The entry called directly: the three outputs and the workspace between guard zones, the inputs inside larger
    allocations; one call over T trials and two calls over T1 + T2 accumulate the same sums on top of what the histograms held,
    and the rows of the second call land behind those of the first."""
    import torch
    if force:
        monkeypatch.setenv(FORCE, "1")
    else:
        monkeypatch.delenv(FORCE, raising=False)
    key = "3-6-olmos"
    p, rows, mem, want, d_adj, d_m = inputs(E, oracle, key, adj16=False)
    T = len(rows)
    arena = poison.Arena(0x5A)
    d_rows = arena((T + 2, p.n, p.dv), dtype=torch.int32, device="cuda:0")
    d_rows[1:T + 1] = d_adj
    d_bits = arena((T + 2, p.nw), dtype=torch.int32, device="cuda:0")
    d_bits[1:T + 1] = d_m
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = E.lib()

    def call(hist, pos, trial, t0, n):
        nbytes = lib.scldpc_ss_spectrum_workspace_bytes(C.byref(p), n)
        ws = arena(nbytes, dtype=torch.uint8, device="cuda:0")
        E.check(lib.scldpc_ss_spectrum_device(C.byref(p), n, d_rows[1 + t0].data_ptr(), 0, d_bits[1 + t0].data_ptr(), NBINS,
                                              hist.data_ptr(), pos.data_ptr() if pos is not None else None,
                                              trial[t0:].data_ptr() if trial is not None else None, ws.data_ptr(), nbytes, stream))
        synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0                 # the status word: no CN id out of range
    base_h = 1000 + np.arange(NBINS, dtype=np.int64)
    base_p = 5 + np.arange(p.L * 8, dtype=np.int64).reshape(p.L, 8)
    bufs = []
    for _ in range(3):
        h, q = arena((NBINS,), dtype=torch.int64, device="cuda:0"), arena((p.L, 8), dtype=torch.int64, device="cuda:0")
        h.copy_(torch.from_numpy(base_h))
        q.copy_(torch.from_numpy(base_p))
        bufs.append((h, q, arena((T, 4), dtype=torch.int32, device="cuda:0")))
    call(*bufs[0], 0, T)
    T1 = T // 3 + 1
    call(*bufs[1], 0, T1)
    call(*bufs[1], T1, T - T1)
    call(bufs[2][0], None, None, 0, T)                                   # the two optional outputs left out
    arena.check_guards()
    for k, what in ((0, "one call"), (1, "two calls")):
        poison.assert_defined_equal((what, "hist"), bufs[k][0].cpu().numpy(), base_h + want[0])
        poison.assert_defined_equal((what, "pos_hist"), bufs[k][1].cpu().numpy(), base_p + want[1])
        poison.assert_defined_equal((what, "trial"), bufs[k][2].cpu().numpy(), want[2])
    poison.assert_defined_equal("hist alone", bufs[2][0].cpu().numpy(), base_h + want[0])
    assert (bufs[2][1].cpu().numpy() == base_p).all() and (bufs[2][2].cpu().numpy().view(np.uint8) == 0x5A).all()
    for d_big, d_in in ((d_rows, d_adj), (d_bits, d_m)):
        edge = torch.cat([d_big[:1], d_big[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all() and (d_big[1:T + 1] == d_in).all()
