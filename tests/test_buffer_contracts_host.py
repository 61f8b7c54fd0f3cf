"""The buffer-contract harness without a GPU: tests/poison.py finds what it is for (fake "kernels" in torch on CPU tensors),
every device entry of include/scldpc.h is in the GPU file's case table or excluded with a reason, and engine.py allocates
outputs and workspaces through its one seam."""
import inspect
import os
import re

import pytest
import torch

import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 6, 5


# ---- fake kernels: out int32 [ROWS, COLS] = 2 * x + 1, with a workspace of ROWS words ------------------------------------------
def _flat(t, lo, hi):
    """Elements lo .. hi-1 relative to t's first element, as a kernel indexing off its pointer would reach them."""
    return torch.as_strided(t, (hi - lo,), (1,), t.storage_offset() + lo)


def k_correct(x, out, ws):
    ws.copy_(x.sum(dim=1))                               # writes its workspace before it reads it
    out.copy_(2 * x + 1)
    out[:, 0] += ws - x.sum(dim=1)


def k_skips_last_row(x, out, ws):
    ws.zero_()
    out[:-1].copy_(2 * x[:-1] + 1)


def k_writes_past_the_end(x, out, ws):
    k_correct(x, out, ws)
    _flat(out, out.numel(), out.numel() + 1).fill_(7)


def k_writes_a_row_past_the_end(x, out, ws):
    k_correct(x, out, ws)
    _flat(out, out.numel(), out.numel() + out.shape[1]).fill_(7)         # a lane of an absent trial writing row [ROWS]


def k_writes_before_the_start(x, out, ws):
    k_correct(x, out, ws)
    _flat(out, -1, 0).fill_(7)


def k_reads_workspace_first(x, out, ws):
    out.copy_(2 * x + 1)
    out[:, 0] += ws                                      # relies on the words being zero
    ws.zero_()                                           # ... and leaves them zero, as a finished peel does


def _call(arena, kernel, seed):
    x = torch.arange(ROWS * COLS, dtype=torch.int32).reshape(ROWS, COLS) * (seed + 1)
    out = arena((ROWS, COLS), dtype=torch.int32, device="cpu")
    ws = arena(ROWS, dtype=torch.int32, device="cpu")
    kernel(x, out, ws)
    arena.check_guards()
    return out, 2 * x + 1


def _run(kernel, mode):
    """The GPU file's protocol: under `stale`, the same entry on other inputs first."""
    arena = poison.Arena(mode)
    if mode == "stale":
        _call(arena, kernel, 3)
        arena.recycle()
    out, want = _call(arena, kernel, 0)
    poison.assert_defined_equal("fake kernel", out.numpy(), want.numpy())


@pytest.mark.parametrize("mode", poison.MODES)
def test_a_correct_kernel_passes(mode):
    _run(k_correct, mode)


@pytest.mark.parametrize("mode", poison.MODES)
def test_a_skipped_row_is_found(mode):
    # stale: the row still holds what the priming call, which skipped it too, was given
    with pytest.raises(AssertionError, match=r"fake kernel: 5 defined element\(s\) differ, first at \(5, 0\)"):
        _run(k_skips_last_row, mode)


@pytest.mark.parametrize("mode", poison.MODES)
def test_a_write_past_the_end_is_found(mode):
    with pytest.raises(poison.GuardError, match=r"allocation #\d+ \(120 bytes, shape \(6, 5\), torch.int32\): guard byte changed "
                                                r"1 byte\(s\) past the end"):
        _run(k_writes_past_the_end, mode)


def test_a_write_one_whole_row_past_the_end_is_found():
    """A row longer than GUARD: the guard is sized to it, so the store of an absent trial's lane cannot jump over it."""
    arena = poison.Arena(0xFF)
    out = arena((3, 200), dtype=torch.int32, device="cpu")               # 800 bytes per row: a guard of 1024
    _flat(out, out.numel() + 199, out.numel() + 200).fill_(7)            # the last element of row [3]
    with pytest.raises(poison.GuardError, match=r"guard byte changed 797 byte\(s\) past the end"):
        arena.check_guards()
    with pytest.raises(poison.GuardError, match=r"guard byte changed 1 byte\(s\) past the end \(20 guard bytes changed"):
        _run(k_writes_a_row_past_the_end, 0x5A)


@pytest.mark.parametrize("mode", poison.MODES)
def test_a_write_before_the_start_is_found(mode):
    with pytest.raises(poison.GuardError, match=r"\(120 bytes, shape \(6, 5\), torch.int32\): guard byte changed 1 byte\(s\) "
                                                r"before the start"):
        _run(k_writes_before_the_start, mode)


@pytest.mark.parametrize("mode", (0xFF, 0x5A))
def test_a_workspace_read_before_it_is_written_is_found(mode):
    with pytest.raises(AssertionError, match=r"fake kernel: 6 defined element\(s\) differ, first at \(0, 0\)"):
        _run(k_reads_workspace_first, mode)


def test_a_workspace_that_a_finished_run_zeroed_hides_the_read_under_stale_only():
    """Why the fills exist: what the caching allocator hands back today (the previous call's block, driven back to zero) lets
    this kernel pass, and `stale` reproduces exactly that — the first time a size is met it is filled with 0xFF."""
    arena = poison.Arena("stale")
    with pytest.raises(AssertionError):
        _call_and_compare(arena, k_reads_workspace_first, 3)
    arena.recycle()
    _call_and_compare(arena, k_reads_workspace_first, 0)                 # passes: the words are the zeros it left


def _call_and_compare(arena, kernel, seed):
    out, want = _call(arena, kernel, seed)
    poison.assert_defined_equal("fake kernel", out.numpy(), want.numpy())


def test_arena_layout_and_records():
    arena = poison.Arena(0x5A)
    a = arena((3, 7), dtype=torch.int16, device="cpu")
    b = arena(1000, dtype=torch.uint8, device="cpu")
    assert a.shape == (3, 7) and a.dtype == torch.int16 and a.is_contiguous() and (a == 0x5A5A).all()
    assert b.shape == (1000,) and (b == 0x5A).all() and poison.GUARD % 512 == 0
    assert [r.nbytes for r in arena.records] == [42, 1000] and [r.order for r in arena.records] == [0, 1]
    assert a.data_ptr() - arena.records[0].raw.data_ptr() == poison.GUARD == arena.records[0].guard
    big = arena((4, 300, 3), dtype=torch.int32, device="cpu")            # a slice along dim 0 is 3600 bytes: a guard of 4096
    assert arena.records[2].guard == 4096 == big.data_ptr() - arena.records[2].raw.data_ptr()
    assert poison.guard_bytes((5, 128), 5 * 512) == 512 and poison.guard_bytes((5, 129), 5 * 516) == 1024
    assert poison.guard_bytes((100000,), 100000) == 512
    assert arena.poison_value(torch.int32) == 0x5A5A5A5A and poison.Arena(0xFF).poison_value(torch.int32) == -1
    arena.check_guards()
    stale = poison.Arena("stale")
    c = stale(16, dtype=torch.uint8, device="cpu")
    assert (c == 0xFF).all()
    c.copy_(torch.arange(16, dtype=torch.uint8))
    stale.recycle()
    d = stale(16, dtype=torch.uint8, device="cpu")
    assert d.data_ptr() == c.data_ptr() and (d == torch.arange(16, dtype=torch.uint8)).all()
    assert (stale((4, 4), dtype=torch.uint8, device="cpu") == 0xFF).all()          # the pool held one buffer of 16 bytes only


def test_defined_masks():
    import numpy as np
    assert poison.padding_mask(216) == 0xFF000000 and poison.padding_mask(64) == 0 and poison.padding_mask(33) == 0xFFFFFFFE
    bits = np.ones((2, 40), dtype=np.uint8)
    assert poison.bitmap_expected(bits).tolist() == [[0xFFFFFFFF, 0xFF]] * 2             # padding bits: 0
    m = poison.rows_defined([0, 2, 9], 4)
    assert m.shape == (3, 4, 3) and m[:, :, 0].tolist() == [[False] * 4, [True, True, False, False], [True] * 4]
    assert poison.r1_defined(2, 5).shape == (2, 6) and poison.r1_defined(2, 5).all()
    poison.assert_defined_equal("x", np.array([1, 2, 3]), np.array([1, 9, 3]), np.array([True, False, True]))
    with pytest.raises(AssertionError, match=r"x: 1 defined element\(s\) differ, first at \(1,\): got 2, want 9"):
        poison.assert_defined_equal("x", np.array([1, 2, 3]), np.array([1, 9, 3]))


# ---- inventory -----------------------------------------------------------------------------------------------------------------
def header_device_entries():
    """{scldpc_* function: its non-const d_* pointer parameters (outputs, in/out buffers, d_workspace)} from the header."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scldpc.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(scldpc_\w+)\s*\(([^;{]*?)\)\s*;", text):
        params = [a.strip() for a in m.group(2).split(",")]
        outs = [a.split("*")[-1].strip() for a in params if re.search(r"\*\s*d_\w+$", a) and not a.startswith("const")]
        if outs:
            out[m.group(1)] = outs
    return out


def test_every_device_entry_of_the_header_is_in_the_case_table_or_excluded_with_a_reason():
    import test_gpu_buffer_contracts as G
    entries = header_device_entries()
    assert len(entries) >= 52 and "scldpc_full_bp_device" in entries and "scldpc_glibc_state_init" not in entries
    assert entries["scldpc_peel_pick_device_adj16"] == ["d_mt_state", "d_r1", "d_moments", "d_out", "d_workspace"]
    covered = G.covered_symbols()
    assert covered <= set(entries), covered - set(entries)
    assert not covered & set(G.EXCLUDED), covered & set(G.EXCLUDED)
    missing = sorted(set(entries) - covered - set(G.EXCLUDED))
    assert not missing, "entries of include/scldpc.h that no buffer-contract case runs: %s" % missing
    stale = sorted(set(G.EXCLUDED) - set(entries))
    assert not stale, stale
    caller_owned = {"d_state", "d_run", "d_moments", "d_mt_state", "d_chan_bits"}           # (d_counters: the streaming entries'
    # running totals only, which come with d_state; a decoder's d_counters is an output and excludes nothing)
    for name, reason in G.EXCLUDED.items():
        assert reason and "\n" not in reason, name
        # the one kind of exclusion a device entry can have: a buffer the caller initialises (no host-only entry has a d_ pointer)
        assert set(entries[name]) & caller_owned, (name, entries[name])
        assert "caller" in reason, (name, reason)


def test_the_case_table_keeps_two_shapes_per_case():
    import test_gpu_buffer_contracts as G
    from fl_scaling_sc_ldpc_amd import engine as E
    G.check_table(E)
    sh = G.shapes()
    assert [sh[k].n for k in G.SMALL[:4]] == [216, 602, 150, 420] and sh["a"].p.cns_pos == 12
    assert sh["b"].total_size < sh["b"].p.nk and sh["b"].doped
    for k, s in sh.items():
        if k.startswith("ws_"):
            assert (s.dv, s.dc) == (4, 8)
    names = [c.name for c in G.cases()]
    assert len(names) == len(set(names))
    for which in G.SIDE:
        name, key = which.split("@")
        assert name in names and key in sh


# ---- the seam ------------------------------------------------------------------------------------------------------------------
def test_engine_allocates_outputs_and_workspaces_through_the_seam():
    from fl_scaling_sc_ldpc_amd import engine as E
    src = inspect.getsource(E)
    uses = [ln.strip() for ln in src.split("\n") if re.search(r"\btorch\.empty(_like|_strided)?\s*\(", ln)]
    assert uses == ["return torch.empty(shape, dtype=dtype, device=device)"], uses
    assert "new_rows=torch." not in src
    assert inspect.signature(E._full_bp).parameters["new_rows"].default is None        # resolved when called, not when defined
    t = E._uninit((3, 4), dtype=torch.int16, device="cpu")
    assert t.shape == (3, 4) and t.dtype == torch.int16 and t.is_contiguous() and t.device.type == "cpu"
    z = E._zeroed((2, 5, 3), dtype=torch.int32, device="cpu")
    assert z.shape == (2, 5, 3) and z.dtype == torch.int32 and not z.any()


def test_the_seam_is_looked_up_at_call_time(monkeypatch):
    from fl_scaling_sc_ldpc_amd import engine as E
    arena = poison.Arena(0xFF)
    monkeypatch.setattr(E, "_uninit", arena)
    z = E._zeroed((2, 3), dtype=torch.int32, device="cpu")                 # the wrappers' rows come out of the arena too
    assert len(arena.records) == 1 and not z.any()
    arena.check_guards()
