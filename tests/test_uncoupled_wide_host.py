"""The wide rejection sampler of the uncoupled ensemble on the CPU: the symbols of the extension header
include/scldpc_uncoupled_wide.h, the shape rule and the order of the checks of its entry (decided before any device work:
placeholder pointers that are never dereferenced, as tests/test_uncoupled_host.py), the pure selector select_uncoupled, and which
engine entry simulate_peeling_decoder_ldpc_uncoupled(rng="philox") calls, with the engine's device calls replaced by stand-ins."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
from test_uncoupled_host import header_device_entries

ONE = C.c_void_p(16)                                                    # non-null placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_uncoupled_wide.h")
ENTRY = "scldpc_sample_philox_uncoupled_wide_device"
GOOD = P(3, 6, 1, 8, 16)


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_UNCOUPLED_WIDE) and len(declared) == 2
    assert not declared & (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED))
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc_uncoupled.h"' in text and L.scldpc_abi_version() == 2
    assert header_device_entries(HEADER) == {ENTRY: ["d_vn_adj", "d_chan_bits", "d_attempts"]}
    assert L.scldpc_sample_philox_uncoupled_wide_device.argtypes == L.scldpc_sample_philox_uncoupled_device.argtypes
    assert "scldpc_uncoupled_wide.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_uncoupled_wide.h"\nint main(void){scldpc_code_params p={3,6,1,5000,10000};'
                   'int (*f)(const scldpc_code_params *) = scldpc_sample_philox_uncoupled_wide_supported;'
                   'int (*g)(const scldpc_code_params *) = scldpc_sample_philox_uncoupled_supported;'
                   'return (int)sizeof(p)-20+(f==0)+(g==0);}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the shape rule ---------------------------------------------------------------------------------------------------------
def sample(p, seed=1, trial0=0, ntrials=0, eps=0.5, cap=100, adj=ONE, ch=ONE, att=ONE):
    rc = _lib.lib().scldpc_sample_philox_uncoupled_wide_device(C.byref(p), seed, trial0, ntrials, eps, cap, adj, ch, att, None)
    return rc, _lib.lib().scldpc_last_error().decode()


@pytest.mark.parametrize("p", [
    P(3, 6, 1, 8, 16), P(3, 6, 1, 1365, 2730), P(4, 8, 1, 1024, 2048), P(3, 6, 1, 1366, 2732),       # 8190, 8192, 8196 sockets
    P(3, 6, 1, 5000, 10000), P(2, 4, 1, 8192, 16384), P(3, 4, 1, 8190, 10920),                       # 30 000, 32 768, 32 760
    P(8, 8, 1, 8, 8), P(3, 6, 1, 3, 6),                                                              # dv = 8; dv = cns_pos
], ids=lambda p: "%d-%d-M%d" % (p.dv, p.dc, p.vns_pos))
def test_supported_over_a_table(p):
    assert E.uncoupled_wide_supported(p)
    assert sample(p)[0] == OK                                            # an empty batch is judged by the same rule


@pytest.mark.parametrize("p,code,part", [
    (P(2, 4, 1, 8193, 16386), TOO_LARGE, "at most 32768 sockets"),                 # 32 772 sockets
    (P(3, 6, 2, 8, 16), BAD_ARG, "L must be 1"),
    (P(9, 18, 1, 8, 16), TOO_LARGE, "dv <= 8"),
    (P(5, 10, 1, 4, 8), BAD_ARG, "dv > cns_pos"),
    (P(3, 6, 1, 8, 17), BAD_ARG, "must equal"),                                    # invalid parameters
], ids=["32772", "L2", "dv9", "dv-gt-cns", "invalid"])
def test_refusals_name_the_limit_even_for_an_empty_batch(p, code, part):
    assert not E.uncoupled_wide_supported(p)
    assert part in _lib.lib().scldpc_last_error().decode()
    for ntrials in (0, 1):
        rc, msg = sample(p, ntrials=ntrials)
        assert rc == code and part in msg, (ntrials, rc, msg)
        if part != "must equal":
            assert msg.startswith(ENTRY + ": "), msg


def test_the_checks_come_in_the_documented_order():
    # parameters, L, size, dv <= cns_pos: each one before those behind it
    assert "must equal" in sample(P(3, 6, 2, 8, 17))[1]
    assert "L must be 1" in sample(P(9, 18, 2, 1000, 2000))[1]
    assert "dv <= 8" in sample(P(9, 18, 1, 4000, 8000))[1]                  # 72 000 sockets: dv is named first
    assert "at most 32768 sockets" in sample(P(8, 16, 1, 4000, 8000))[1]
    assert sample(P(5, 10, 1, 4, 8), eps=2.0)[1].endswith("(got dv = 5, cns_pos = 4)")
    # the shape before eps, eps before max_attempts, that before trial0, that before ntrials, all before the buffers
    rc, msg = sample(GOOD, eps=1.5, cap=0, trial0=1 << 41, ntrials=-1, adj=None)
    assert rc == BAD_ARG and "eps=1.5 outside [0,1]" in msg
    rc, msg = sample(GOOD, eps=float("nan"))
    assert rc == BAD_ARG and "outside [0,1]" in msg
    for cap in (0, -5, (1 << 24) + 1):
        rc, msg = sample(GOOD, cap=cap, trial0=1 << 41, ntrials=-1, adj=None)
        assert rc == BAD_ARG and "1 <= max_attempts <= 16777216" in msg, cap
    rc, msg = sample(GOOD, trial0=(1 << 40) - 3, ntrials=4, adj=None)
    assert rc == BAD_ARG and "trial0 + ntrials <= 2^40" in msg
    rc, msg = sample(GOOD, trial0=(1 << 40) + 1, ntrials=-1, adj=None)
    assert rc == BAD_ARG and "trial0 + ntrials <= 2^40" in msg
    rc, msg = sample(GOOD, ntrials=-1, adj=None)
    assert rc == BAD_ARG and "negative ntrials" in msg
    # an empty batch is fine with any buffers, at either end of the ranges
    assert sample(GOOD, ntrials=0, adj=None, ch=None, att=None)[0] == OK
    assert sample(P(3, 6, 1, 5000, 10000), ntrials=0, cap=1 << 24, trial0=1 << 40, eps=1.0, adj=None, ch=None, att=None)[0] == OK
    assert sample(GOOD, ntrials=0, cap=1, eps=0.0)[0] == OK
    for kw in (dict(adj=None), dict(ch=None), dict(att=None)):
        rc, msg = sample(P(3, 6, 1, 5000, 10000), ntrials=1, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer", kw


# ---- the selector ------------------------------------------------------------------------------------------------------------
def test_the_selector_over_its_truth_table():
    p = P(3, 6, 1, 5000, 10000)
    sel = PD.select_uncoupled
    assert PD.UNCOUPLED_WIDE_BY_DEFAULT is False
    #           first_ok  wide_ok  by_default
    assert sel(p, True, True, False) == "first"
    assert sel(p, True, False, False) == "first"
    assert sel(p, True, True, True) == "wide"
    assert sel(p, True, False, True) == "first"                          # the flag sends nothing where the wide one refuses
    assert sel(p, False, True, False) == "wide"
    assert sel(p, False, True, True) == "wide"
    assert sel(p, True, True) == "first"                                 # the default of the fourth argument
    for by_default in (False, True):
        with pytest.raises(ValueError, match=r"at most 32768 sockets \(sample_philox_uncoupled: 8192\); got dv = 3, dc = 6, "
                                             r"cns_pos = 5000, M = 10000: 30000 sockets"):
            sel(p, False, False, by_default)
    assert [q.name for q in inspect.signature(sel).parameters.values()] == ["p", "first_ok", "wide_ok", "wide_by_default"]


def test_the_selector_on_the_librarys_answers():
    for p, want in [(P(3, 6, 1, 8, 16), "first"), (P(3, 6, 1, 1365, 2730), "first"), (P(4, 8, 1, 1024, 2048), "first"),
                    (P(3, 6, 1, 1366, 2732), "wide"), (P(3, 6, 1, 5000, 10000), "wide"), (P(2, 4, 1, 8192, 16384), "wide")]:
        first_ok, wide_ok = E.uncoupled_supported(p), E.uncoupled_wide_supported(p)
        assert PD.select_uncoupled(p, first_ok, wide_ok, False) == want
        assert PD.select_uncoupled(p, first_ok, wide_ok, True) == "wide"
    p = P(2, 4, 1, 8193, 16386)
    with pytest.raises(ValueError, match="32772 sockets"):
        PD.select_uncoupled(p, E.uncoupled_supported(p), E.uncoupled_wide_supported(p), False)


# ---- the simulator's routing ---------------------------------------------------------------------------------------------
def stand_ins(monkeypatch):
    import torch
    seen = []

    def sampler(name):
        def f(p, seed, trial0, ntrials, eps, max_attempts, device=None, out=None):
            seen.append((name, trial0, ntrials, max_attempts))
            z = torch.zeros((ntrials, 1, 1), dtype=torch.int32)              # (the stand-in pick reads the trial count alone)
            return z, torch.zeros((ntrials, p.nw), dtype=torch.int32), torch.ones(ntrials, dtype=torch.int32)
        return f

    def peel_pick(p, d_adj, d_chan, total_size, num_steps, mt_state=None, seed=0, trial0=0, want_r1=True, moments=None):
        T = d_adj.shape[0]
        return {"out": torch.zeros((T, 4), dtype=torch.int32), "r1": torch.zeros((T, num_steps + 1), dtype=torch.int32)}

    monkeypatch.setattr(E, "sample_philox_uncoupled", sampler("first"))
    monkeypatch.setattr(E, "sample_philox_uncoupled_wide", sampler("wide"))
    monkeypatch.setattr(E, "peel_pick", peel_pick)
    return seen


def test_the_simulator_routes_by_the_socket_count(monkeypatch):
    seen = stand_ins(monkeypatch)
    f = PD.simulate_peeling_decoder_ldpc_uncoupled
    # M = 10000 at (3,6): 30 000 sockets, the wide entry; default batch = the wide budget / exp(5), below the 8192 of memory
    monkeypatch.setattr(PD, "UNCOUPLED_WIDE_ATTEMPTS_PER_LAUNCH", 100 * np.exp(5.0) + 1)
    out = f(0.42, 3, 6, 10000, 250, device="cpu", rng="philox", max_attempts=77)
    assert seen == [("wide", 0, 100, 77), ("wide", 100, 100, 77), ("wide", 200, 50, 77)]
    assert out[0] is None and out[1].shape == (250, 5201) and out[2].shape == (250,) and out[3] == [0] * 250
    del seen[:]
    f(0.42, 3, 6, 10000, 250, device="cpu", rng="philox", batch=128)        # an explicit batch is taken as it is
    assert seen == [("wide", 0, 128, 1 << 20), ("wide", 128, 122, 1 << 20)]
    del seen[:]
    # M = 16: the first entry and its own budget, whatever the wide one's
    monkeypatch.setattr(PD, "UNCOUPLED_WIDE_ATTEMPTS_PER_LAUNCH", 1)
    monkeypatch.setattr(PD, "UNCOUPLED_ATTEMPTS_PER_LAUNCH", 100 * np.exp(5.0) + 1)
    f(0.4, 3, 6, 16, 150, device="cpu", rng="philox")
    assert seen == [("first", 0, 100, 1 << 20), ("first", 100, 50, 1 << 20)]
    del seen[:]
    monkeypatch.setattr(PD, "UNCOUPLED_WIDE_BY_DEFAULT", True)              # the flag: the wide entry, the batch rule unchanged
    f(0.4, 3, 6, 16, 150, device="cpu", rng="philox")
    assert seen == [("wide", 0, 100, 1 << 20), ("wide", 100, 50, 1 << 20)]


def test_the_simulator_refuses_a_shape_neither_takes_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("sample_philox_uncoupled", "sample_philox_uncoupled_wide", "peel_pick", "to_device", "local_device", "_require_gpu"):
        monkeypatch.setattr(E, name, no_device)
    with pytest.raises(ValueError, match=r"at most 32768 sockets .*M = 16386: 32772 sockets"):
        PD.simulate_peeling_decoder_ldpc_uncoupled(0.3, 2, 4, 16386, 2, rng="philox", device="cpu")


def test_the_engine_signatures_are_the_siblings():
    assert ([(q.name, q.default) for q in inspect.signature(E.sample_philox_uncoupled_wide).parameters.values()]
            == [(q.name, q.default) for q in inspect.signature(E.sample_philox_uncoupled).parameters.values()])
    assert list(inspect.signature(E.uncoupled_wide_supported).parameters) == ["p"]
