"""The rejection sampler of the uncoupled ensemble on the CPU: the symbols of the extension header include/scldpc_uncoupled.h,
the shape rule and the order of the checks of its entry (decided before any device work: placeholder pointers that are never
dereferenced, as tests/test_sweep_ens_host.py), and what simulate_peeling_decoder_ldpc_uncoupled refuses before it touches a
device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ONE = C.c_void_p(16)                                                    # non-null placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_uncoupled.h")
ENTRY = "scldpc_sample_philox_uncoupled_device"
GOOD = P(3, 6, 1, 8, 16)


def header_device_entries(path=HEADER):
    """tests/test_buffer_contracts_host.py's header_device_entries, on this header: {scldpc_* function: its non-const d_*
    pointer parameters}."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(scldpc_\w+)\s*\(([^;{]*?)\)\s*;", text):
        params = [a.strip() for a in m.group(2).split(",")]
        outs = [a.split("*")[-1].strip() for a in params if re.search(r"\*\s*d_\w+$", a) and not a.startswith("const")]
        if outs:
            out[m.group(1)] = outs
    return out


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_UNCOUPLED) and len(declared) == 2
    assert not declared & (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES))      # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc.h"' in text and L.scldpc_abi_version() == 2
    assert header_device_entries() == {ENTRY: ["d_vn_adj", "d_chan_bits", "d_attempts"]}
    assert "scldpc_uncoupled.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_uncoupled.h"\nint main(void){scldpc_code_params p={3,6,1,8,16};'
                   'int (*f)(const scldpc_code_params *) = scldpc_sample_philox_uncoupled_supported;'
                   'return (int)sizeof(p)-20+(f==0);}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the shape rule ---------------------------------------------------------------------------------------------------------
def sample(p, seed=1, trial0=0, ntrials=0, eps=0.5, cap=100, adj=ONE, ch=ONE, att=ONE):
    rc = _lib.lib().scldpc_sample_philox_uncoupled_device(C.byref(p), seed, trial0, ntrials, eps, cap, adj, ch, att, None)
    return rc, _lib.lib().scldpc_last_error().decode()


@pytest.mark.parametrize("p,want", [
    (P(3, 6, 1, 8, 16), True), (P(3, 6, 1, 1365, 2730), True), (P(4, 8, 1, 1024, 2048), True),      # 8190 and 8192 sockets
    (P(2, 4, 1, 16, 32), True), (P(3, 4, 1, 12, 16), True), (P(4, 6, 1, 32, 48), True), (P(5, 10, 1, 4, 8), False),
    (P(8, 8, 1, 8, 8), True), (P(3, 6, 1, 3, 6), True),                                           # dv = 8; dv = cns_pos
])
def test_supported_over_a_small_table(p, want):
    assert E.uncoupled_supported(p) == want
    assert sample(p)[0] == (OK if want else BAD_ARG)                     # an empty batch is judged by the same rule


@pytest.mark.parametrize("p,code,part", [
    (P(3, 6, 2, 8, 16), BAD_ARG, "L must be 1"),
    (P(3, 6, 1, 1366, 2732), TOO_LARGE, "at most 8192 sockets"),                   # 8196 sockets
    (P(9, 18, 1, 8, 16), TOO_LARGE, "dv <= 8"),
    (P(5, 10, 1, 4, 8), BAD_ARG, "dv > cns_pos"),
    (P(3, 6, 1, 8, 17), BAD_ARG, "must equal"),                                    # invalid parameters
], ids=["L2", "8196", "dv9", "dv-gt-cns", "invalid"])
def test_refusals_name_the_limit_even_for_an_empty_batch(p, code, part):
    assert _lib.lib().scldpc_sample_philox_uncoupled_supported(C.byref(p)) == 0
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
    assert "dv <= 8" in sample(P(9, 18, 1, 4, 8))[1]
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
    assert sample(GOOD, ntrials=0, cap=1 << 24, trial0=1 << 40, eps=1.0, adj=None, ch=None, att=None)[0] == OK
    assert sample(GOOD, ntrials=0, cap=1, eps=0.0)[0] == OK
    for kw in (dict(adj=None), dict(ch=None), dict(att=None)):
        rc, msg = sample(GOOD, ntrials=1, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer", kw


# ---- the Python side ---------------------------------------------------------------------------------------------------------
def test_the_simulator_refuses_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("sample_philox_uncoupled", "peel_pick", "to_device", "local_device", "_require_gpu"):
        monkeypatch.setattr(E, name, no_device)
    f = PD.simulate_peeling_decoder_ldpc_uncoupled
    with pytest.raises(ValueError, match="rng must be 'numpy' or 'philox'"):
        f(0.4, 3, 6, 16, 2, rng="x")
    for cap in (0, (1 << 24) + 1):
        for rng in ("numpy", "philox"):
            with pytest.raises(ValueError, match="max_attempts"):
                f(0.4, 3, 6, 16, 2, rng=rng, max_attempts=cap)
    with pytest.raises(ValueError, match="divisible"):
        f(0.4, 3, 6, 17, 2, rng="philox")
    with pytest.raises(ValueError, match="divisible"):
        f(0.4, 3, 4, 18, 2, rng="philox", device="cpu")


def test_the_signature_keeps_its_first_six_parameters():
    ps = list(inspect.signature(PD.simulate_peeling_decoder_ldpc_uncoupled).parameters.values())
    assert [q.name for q in ps[:6]] == ["e", "l_deg", "r_deg", "M", "num_repeats", "device"]
    assert [q.default for q in ps[:6]] == [inspect.Parameter.empty] * 4 + [None, None]
    assert [(q.name, q.default) for q in ps[6:]] == [("rng", "numpy"), ("seed", 0), ("batch", None), ("want_moments", False),
                                                     ("max_attempts", 1 << 20)]
    assert [(q.name, q.default) for q in list(inspect.signature(E.sample_philox_uncoupled).parameters.values())] == [
        ("p", inspect.Parameter.empty), ("seed", inspect.Parameter.empty), ("trial0", inspect.Parameter.empty),
        ("ntrials", inspect.Parameter.empty), ("eps", inspect.Parameter.empty), ("max_attempts", inspect.Parameter.empty),
        ("device", "cuda:0"), ("out", None)]


def test_the_default_batch_is_capped_by_the_expected_attempts(monkeypatch):
    """batch * exp((l-1)(r-1)/2) stays below UNCOUPLED_ATTEMPTS_PER_LAUNCH; an explicit batch is taken as it is."""
    import numpy as np
    import torch
    seen = []

    def sample_philox_uncoupled(p, seed, trial0, ntrials, eps, max_attempts, device=None, out=None):
        seen.append((trial0, ntrials, max_attempts))
        z = torch.zeros((ntrials, p.n, p.dv), dtype=torch.int32)
        return z, torch.zeros((ntrials, p.nw), dtype=torch.int32), torch.ones(ntrials, dtype=torch.int32)

    def peel_pick(p, d_adj, d_chan, total_size, num_steps, mt_state=None, seed=0, trial0=0, want_r1=True, moments=None):
        T = d_adj.shape[0]
        return {"out": torch.zeros((T, 4), dtype=torch.int32), "r1": torch.zeros((T, num_steps + 1), dtype=torch.int32)}

    monkeypatch.setattr(E, "sample_philox_uncoupled", sample_philox_uncoupled)
    monkeypatch.setattr(E, "peel_pick", peel_pick)
    monkeypatch.setattr(PD, "UNCOUPLED_ATTEMPTS_PER_LAUNCH", 100 * np.exp(10.5) + 1)
    out = PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 4, 8, 16, 250, device="cpu", rng="philox", max_attempts=77)
    assert seen == [(0, 100, 77), (100, 100, 77), (200, 50, 77)]
    assert out[0] is None and out[1].shape == (250, 9) and out[2].shape == (250,) and out[3] == [0] * 250
    del seen[:]
    PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 4, 8, 16, 250, device="cpu", rng="philox", batch=128)
    assert seen == [(0, 128, 1 << 20), (128, 122, 1 << 20)]
