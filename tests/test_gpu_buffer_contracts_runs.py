"""Buffer contract of the two device entries of include/scldpc_runs.h (-m gpu), as tests/test_gpu_buffer_contracts_ss.py keeps it
for include/scldpc_ss.h: the entries are called directly with every output between guard zones of a poison.Arena and the inputs
inside larger poisoned allocations:
  * the accumulators change only by the sums (on top of what they held), exactly;
  * d_trial, d_fail_bits and the carry are written exactly as the header lists them, padding bits zero, and an optional output
    left out is left alone;
  * no guard byte changes, and no input changes;
  * engine.chain_runs allocates its two per-trial outputs through engine._uninit and nothing else.
The file also checks that it covers every device entry of the header."""
import ctypes as C

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_runs_host import HEADER, np_chain_runs, np_stream_runs, synthetic_chain_bits, synthetic_stream_rows
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu


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
    assert header_device_entries(HEADER) == {
        "scldpc_chain_runs_device": ["d_pos", "d_run_hist", "d_fail_hist", "d_trial", "d_fail_bits"],
        "scldpc_stream_runs_device": ["d_carry", "d_hist", "d_sums", "d_phase"]}


@pytest.mark.parametrize("L,V", [(12, 20), (70, 33)])
def test_chain_outputs_between_red_zones(E, L, V):
    import torch
    T = 64
    bits = synthetic_chain_bits(L, V, T, .5 if L == 70 else .35, .1 if L == 70 else .2)
    want_acc, want_trial, want_fb = np_chain_runs(bits, L, V)
    p = E.CodeParams(1, 1, L, V, V)
    words = E.pack_bits(bits.astype(np.uint8)).view(np.int32)
    if (L * V) % 32:
        words[:, -1] |= np.array([poison.padding_mask(L * V)], np.uint32).view(np.int32)[0]     # garbage beyond n
    arena = poison.Arena(0x5A)
    d_in = arena((T + 2, p.nw), dtype=torch.int32, device="cuda:0")
    d_in[1:T + 1] = torch.from_numpy(words).cuda()
    before = d_in.clone()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fw = (L + 31) // 32
    shapes = (("pos", (L, 4)), ("run_hist", (L + 1, 2)), ("fail_hist", (L + 1,)))
    base = {k: 1000 + np.arange(int(np.prod(sh)), dtype=np.int64).reshape(sh) for k, sh in shapes}

    def outputs():
        acc = {}
        for k, sh in shapes:
            acc[k] = arena(sh, dtype=torch.int64, device="cuda:0")
            acc[k].copy_(torch.from_numpy(base[k]))
        return acc, arena((T, 4), dtype=torch.int32, device="cuda:0"), arena((T, fw), dtype=torch.int32, device="cuda:0")

    def call(acc, trial, fb, t0, n):
        E.check(E.lib().scldpc_chain_runs_device(C.byref(p), n, d_in[1 + t0].data_ptr(), acc["pos"].data_ptr(),
                                                 acc["run_hist"].data_ptr(), acc["fail_hist"].data_ptr(),
                                                 trial[t0:].data_ptr() if trial is not None else None,
                                                 fb[t0:].data_ptr() if fb is not None else None, stream))
        synchronize()

    one, two, bare = outputs(), outputs(), outputs()
    call(*one, 0, T)
    call(*two, 0, 23)
    call(*two, 23, T - 23)
    call(bare[0], None, None, 0, T)                                      # the two optional outputs left out
    arena.check_guards()
    for what, (acc, trial, fb) in (("one call", one), ("two calls", two)):
        for k, _ in shapes:
            poison.assert_defined_equal((what, k), acc[k].cpu().numpy(), base[k] + want_acc[k])
        poison.assert_defined_equal((what, "trial"), trial.cpu().numpy(), want_trial)
        got = fb.cpu().numpy().view(np.uint32)
        poison.assert_defined_equal((what, "fail_bits"), got, want_fb)
        assert not (got[:, -1] & poison.padding_mask(L)).any()          # padding bits are zero
    for k, _ in shapes:
        poison.assert_defined_equal(("alone", k), bare[0][k].cpu().numpy(), base[k] + want_acc[k])
    assert (bare[1].cpu().numpy().view(np.uint8) == 0x5A).all() and (bare[2].cpu().numpy().view(np.uint8) == 0x5A).all()
    assert torch.equal(d_in, before)                                     # inputs are only read


def test_chain_wrapper_allocates_its_rows_through_the_seam(E, monkeypatch):
    import torch
    L, V, T = 12, 20, 64
    bits = synthetic_chain_bits(L, V, T, .35, .2)
    want_acc, want_trial, want_fb = np_chain_runs(bits, L, V)
    p = E.CodeParams(1, 1, L, V, V)
    d_bits = torch.from_numpy(E.pack_bits(bits.astype(np.uint8)).view(np.int32)).cuda()
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            E.chain_runs(p, (~d_bits).contiguous(), want_trial=True, want_fail_bits=True)
            synchronize()
            arena.recycle()
        got = E.chain_runs(p, d_bits, want_trial=True, want_fail_bits=True)
        synchronize()
        arena.check_guards()
        assert [r.nbytes for r in arena.records] == [16 * T, 4 * T]
        for k in want_acc:
            poison.assert_defined_equal((mode, k), got[k].cpu().numpy(), want_acc[k])
        poison.assert_defined_equal((mode, "trial"), got["trial"].cpu().numpy(), want_trial)
        poison.assert_defined_equal((mode, "fail_bits"), got["fail_bits"].cpu().numpy().view(np.uint32), want_fb)
        monkeypatch.undo()


@pytest.mark.parametrize("with_phase", [True, False])
def test_stream_outputs_between_red_zones(E, with_phase):
    import torch
    S, P, nbins, doped = 8, 500, 32, (8, 9)
    rows = synthetic_stream_rows()
    counters = np.zeros((S, 10), np.int64)
    counters[6, 9] = -3                                                  # an unusable stream: skipped, carry kept
    ref = np_stream_runs(S, 4, doped, nbins, with_phase=with_phase)
    ref.carry[6] = (9, 1, 1, 0, 4, 0, 0, 0)
    carry0 = ref.carry.copy()
    ref.feed(rows, skip=(6,))
    p = E.make_params(4, 8, 20, 64)
    arena = poison.Arena(0xFF)
    d_rows = arena((S + 2, P, 10), dtype=torch.int32, device="cuda:0")
    d_rows[1:S + 1] = torch.from_numpy(rows).cuda()
    d_cnt = arena((S + 2, 10), dtype=torch.int64, device="cuda:0")
    d_cnt[1:S + 1] = torch.from_numpy(counters).cuda()
    before = (d_rows.clone(), d_cnt.clone())
    base_h = 7 + np.arange(4 * nbins, dtype=np.int64).reshape(4, nbins)
    base_s = 100 + np.arange(8, dtype=np.int64)
    base_p = 50 + np.arange(30, dtype=np.int64).reshape(10, 3)
    hist, sums = arena((4, nbins), dtype=torch.int64, device="cuda:0"), arena((8,), dtype=torch.int64, device="cuda:0")
    phase, carry = arena((10, 3), dtype=torch.int64, device="cuda:0"), arena((S, 8), dtype=torch.int64, device="cuda:0")
    for d, b in ((hist, base_h), (sums, base_s), (phase, base_p), (carry, carry0)):
        d.copy_(torch.from_numpy(b))
    darr = np.array(doped, np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # two calls over 137 + 363 rows: the rows of a call are one contiguous [S, npos, 10] block
    for k0, k1 in ((0, 137), (137, P)):
        part = arena((S, k1 - k0, 10), dtype=torch.int32, device="cuda:0")
        part.copy_(d_rows[1:S + 1, k0:k1])
        E.check(E.lib().scldpc_stream_runs_device(C.byref(p), S, k1 - k0, part.data_ptr(), d_cnt[1].data_ptr(), darr.size,
                                                  darr.ctypes.data, nbins, carry.data_ptr(), hist.data_ptr(), sums.data_ptr(),
                                                  phase.data_ptr() if with_phase else None, stream))
        synchronize()
        assert (part.cpu().numpy() == rows[:, k0:k1]).all()
    arena.check_guards()
    poison.assert_defined_equal("hist", hist.cpu().numpy(), base_h + ref.hist)
    poison.assert_defined_equal("sums", sums.cpu().numpy(), base_s + ref.sums)
    poison.assert_defined_equal("carry", carry.cpu().numpy(), ref.carry)
    assert (ref.carry[6] == carry0[6]).all() and not ref.carry[:, 5:].any()
    if with_phase:
        poison.assert_defined_equal("phase", phase.cpu().numpy(), base_p + ref.phase)
    else:
        assert (phase.cpu().numpy() == base_p).all()
    assert torch.equal(d_rows, before[0]) and torch.equal(d_cnt, before[1])
