"""Buffer contract of the device entry of include/scldpc_uncoupled_wide.h (-m gpu), as tests/test_gpu_buffer_contracts_unc.py
keeps it for include/scldpc_uncoupled.h: the entry runs with engine._uninit replaced by a poison.Arena — outputs filled with 0xFF,
with 0x5A, or with what a run on another seed left behind, between two guard zones — and
  * every element of every output equals the CPU twin's loop (tests/test_gpu_uncoupled.py), under each fill, so a skipped element
    fails — with a cap that some trials meet, so the zeros of a trial without a graph are written, not found;
  * no guard byte changes;
  * written through a view that starts one trial into a larger allocation, the trials before and behind the view stay untouched.
The file also checks that it covers every device entry of the header.  Integer work: exact, no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_gpu_uncoupled import twin, params
from test_uncoupled_host import header_device_entries

pytestmark = pytest.mark.gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scldpc_uncoupled_wide.h")
T = 12
# key -> (dv, dc, M, eps, seed, cap): M = 2752 (whole words, 8256 sockets), M = 9998 (ragged, four parts) and M = 16382 (ragged,
# 32 764 sockets); the cap cuts some trials
SHAPES = {"36-M2752": (3, 6, 2752, 0.4, 11, 150), "36-M9998": (3, 6, 9998, 0.45, 19, 150), "24-M16382": (2, 4, 16382, 0.45, 19, 4)}


def reference(key, alt=False):
    dv, dc, M, eps, seed, cap = SHAPES[key]
    if alt:
        seed, eps = seed + 1000, 0.8 - eps
    rows, words, att = twin(dv, dc, M, seed, 3, T, eps, cap)
    return dict(p=params(dv, dc, M), seed=seed, eps=eps, cap=cap, want={"rows": rows, "chan": words, "attempts": att})


def run_sampler(E, ref):
    d_adj, d_ch, d_att = E.sample_philox_uncoupled_wide(ref["p"], ref["seed"], 3, T, ref["eps"], ref["cap"])
    return {"rows": d_adj, "chan": d_ch, "attempts": d_att}


CASES = {"scldpc_sample_philox_uncoupled_wide_device": run_sampler}


def compare(what, got, want):
    assert set(got) == set(want), (what, sorted(got))
    for name, w in want.items():
        g = got[name].cpu().numpy()
        poison.assert_defined_equal("%s %s" % (what, name), g.view(np.uint32) if name == "chan" else g, w)


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


def test_the_table_covers_every_device_entry_of_the_header():
    assert set(CASES) == set(header_device_entries(HEADER))
    assert header_device_entries(HEADER)["scldpc_sample_philox_uncoupled_wide_device"] == ["d_vn_adj", "d_chan_bits", "d_attempts"]


def test_the_shapes_are_whole_and_ragged_and_the_cap_cuts_some_trials():
    ms = [SHAPES[k][2] for k in SHAPES]
    assert ms[0] % 32 == 0 and ms[1] % 32 != 0 and ms[2] % 32 != 0
    for key in SHAPES:
        att = reference(key)["want"]["attempts"]
        assert (att == 0).any() and (att > 0).any(), (key, att)
    assert reference("24-M16382")["want"]["attempts"].tolist() == [0, 0, 2, 4, 1, 0, 4, 3, 2, 2, 3, 1]


@pytest.mark.parametrize("key", list(SHAPES))
def test_poisoned_outputs_and_red_zones(E, monkeypatch, key):
    ref, prime = reference(key), reference(key, True)
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            run_sampler(E, prime)                                        # another seed and eps first
            synchronize()
            arena.check_guards()
            arena.recycle()
        got = run_sampler(E, ref)
        synchronize()
        arena.check_guards()
        assert len(arena.records) == len(got)                            # every output came out of the arena, and nothing else
        compare((key, mode), got, ref["want"])
        monkeypatch.undo()


@pytest.mark.parametrize("key", list(SHAPES))
def test_a_view_one_trial_into_a_larger_allocation(E, key):
    """T trials written through pointers that start one trial into buffers of T + 2 trials (the entry called directly): trials 0
    and T + 1 of every buffer keep their poison, trials 1 .. T hold the reference."""
    import torch
    ref = reference(key)
    p = ref["p"]
    arena = poison.Arena(0x5A)
    mk = lambda shape, dtype: arena((T + 2,) + shape, dtype=dtype, device="cuda:0")
    bufs = {"rows": mk((p.n, p.dv), torch.int32), "chan": mk((p.nw,), torch.int32), "attempts": mk((1,), torch.int32)}
    E.check(E.lib().scldpc_sample_philox_uncoupled_wide_device(
        C.byref(p), ref["seed"], 3, T, float(ref["eps"]), ref["cap"], bufs["rows"][1].data_ptr(), bufs["chan"][1].data_ptr(),
        bufs["attempts"][1].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    synchronize()
    arena.check_guards()
    for name, buf in bufs.items():
        edge = torch.cat([buf[:1], buf[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all(), (key, name, "a trial outside the view was written")
    got = {k: v[1:T + 1] for k, v in bufs.items()}
    got["attempts"] = got["attempts"].reshape(T)
    compare((key, "view"), got, ref["want"])
