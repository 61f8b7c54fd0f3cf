"""The covariance workflow on the CPU: the symbols of the extension header include/scldpc_cov.h, the workspace arithmetic and the
checks of its device entry (decided before any device work: placeholder pointers that are never dereferenced, as
tests/test_uncoupled_host.py), what simulate_pd_covariance and its command line refuse before they touch a device, and
cov_from_gram against exact rational arithmetic."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG = 0, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_cov.h")
ENTRY = "scldpc_r1_gram_device"


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_COV) and len(declared) == 3
    assert {"scldpc_r1_gram_workspace_bytes", ENTRY} <= declared
    others = set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
    assert not declared & others                                         # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_cov.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    assert "#define SCLDPC_COV_MAX_STEPS 4096" in text and _lib.COV_MAX_STEPS == 4096 == PD.COV_MAX_STEPS


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_cov.h"\nint main(void){'
                   'int64_t (*f)(int32_t, int32_t) = scldpc_r1_gram_workspace_bytes;'
                   'int (*g)(int32_t, int32_t, const int32_t *, int32_t, const int32_t *, int64_t *, void *, int64_t, void *)'
                   ' = scldpc_r1_gram_device;'
                   'return (f==0)+(g==0)+SCLDPC_COV_MAX_STEPS-4096+SCLDPC_COV_STEP_CLAMPED-1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- sizes and checks, without a device ----------------------------------------------------------------------------------
def ws_bytes(T, K):
    return _lib.lib().scldpc_r1_gram_workspace_bytes(T, K)


@pytest.mark.parametrize("T,K", [(0, 1), (1, 1), (32, 64), (33, 65), (8192, 4096), (5000, 65), (2 ** 31 - 1, 4096)])
def test_workspace_bytes_is_the_status_slot_and_the_padded_panel(T, K):
    tpad, kpad = -(-T // 32) * 32, -(-K // 64) * 64
    assert ws_bytes(T, K) == 256 + 4 * tpad * kpad


@pytest.mark.parametrize("T,K,part", [(-1, 1, "negative ntrials"), (1, 0, "1 <= k <= 4096 (got k = 0)"),
                                      (1, 4097, "1 <= k <= 4096 (got k = 4097)"), (1, -3, "1 <= k <= 4096")])
def test_the_queries_refuse_bad_sizes(T, K, part):
    for fn in ("scldpc_r1_gram_workspace_bytes", "scldpc_r1_gram_trial_splits"):
        assert getattr(_lib.lib(), fn)(T, K) == -1
        msg = _lib.lib().scldpc_last_error().decode()
        assert msg.startswith(fn + ": ") and part in msg, msg


def test_trial_splits_fill_the_device_at_small_k_and_not_beyond_the_chunks():
    assert E.r1_gram_trial_splits(0, 5) == 0
    assert E.r1_gram_trial_splits(1, 1) == 1 and E.r1_gram_trial_splits(32, 300) == 1
    assert E.r1_gram_trial_splits(33, 64) == 2                            # two chunks of 32 trials, one tile
    assert E.r1_gram_trial_splits(5000, 65) == 157                         # 4 tiles: every chunk its own workgroup
    assert E.r1_gram_trial_splits(8192, 256) == 64                         # 16 tiles x 64 = 1024 workgroups
    assert E.r1_gram_trial_splits(8192, 4096) == 1
    with pytest.raises(E.ScldpcError, match="1 <= k <= 4096"):
        E.r1_gram_trial_splits(5, 0)


def gram_call(T=1, ncols=8, r1=ONE, K=2, steps=ONE, gram=ONE, ws=ONE, wsb=None):
    wsb = ws_bytes(max(T, 0), min(max(K, 1), 4096)) if wsb is None else wsb
    rc = _lib.lib().scldpc_r1_gram_device(T, ncols, r1, K, steps, gram, ws, wsb, None)
    return rc, _lib.lib().scldpc_last_error().decode()


def test_the_entry_refuses_with_a_text_and_no_device():
    for K in (0, 4097):
        rc, msg = gram_call(K=K)
        assert rc == BAD_ARG and msg == "%s: 1 <= k <= 4096 (got k = %d)" % (ENTRY, K)
    assert gram_call(K=0, T=0)[0] == BAD_ARG                             # k is judged even for an empty batch
    rc, msg = gram_call(T=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": negative ntrials"
    rc, msg = gram_call(ncols=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": negative ncols"
    rc, msg = gram_call(ncols=0)
    assert rc == BAD_ARG and "ncols = 0" in msg
    for kw in (dict(r1=None), dict(steps=None), dict(gram=None), dict(ws=None)):
        rc, msg = gram_call(**kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer", kw
    rc, msg = gram_call(ws=C.c_void_p(260))
    assert rc == BAD_ARG and "16-byte aligned" in msg
    need = ws_bytes(1, 2)
    rc, msg = gram_call(wsb=need - 1)
    assert rc == BAD_ARG and msg == "%s: workspace of %d bytes, %d needed" % (ENTRY, need - 1, need)
    # an empty batch is fine with any buffers and touches nothing
    assert gram_call(T=0, r1=None, steps=None, gram=None, ws=None, wsb=0)[0] == OK
    assert gram_call(T=0, ncols=0)[0] == OK


# ---- the simulator and the command line ------------------------------------------------------------------------------------
def test_the_simulator_refuses_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("sample_philox", "peel_pick", "peel_pick_deg", "r1_moments", "r1_gram", "to_device", "local_device", "_require_gpu"):
        monkeypatch.setattr(E, name, no_device)
    f = lambda steps, **kw: PD.simulate_pd_covariance(0.45, 4, 8, 10, 40, False, False, kw.pop("n", 4), steps, **kw)
    # num_pd_steps = int(40 * 10 * 0.55) = 220
    for steps in ([3, 2], [0, 5, 5], [5, 1, 9]):
        with pytest.raises(ValueError, match="strictly increasing"):
            f(steps)
    for steps in ([0, 221], [-1, 4], [500]):
        with pytest.raises(ValueError, match="out of range"):
            f(steps)
    for steps in ([], 0, -7, [1.5, 2.5], [[1, 2]]):
        with pytest.raises(ValueError, match="steps"):
            f(steps)
    with pytest.raises(ValueError, match="soft-doping"):
        f(7, doping_points={3: 0.5})
    with pytest.raises(ValueError, match="num_repeats"):
        f(7, n=0)
    with pytest.raises(ValueError, match="at most 4096 steps"):           # num_pd_steps = int(1000 * 10 * 0.55) = 5500 > 4097 steps
        PD.simulate_pd_covariance(0.45, 4, 8, 10, 1000, False, False, 4, 1)
    with pytest.raises(ValueError, match="at most 4096 steps"):
        PD.simulate_pd_covariance(0.45, 4, 8, 10, 1000, False, False, 4, list(range(4097)))
    # total_size = 2^23 CNs per position x 10 positions, 2^20 trials
    with pytest.raises(ValueError, match=">= 2\\^63"):
        PD.simulate_pd_covariance(0.45, 4, 8, 10, 1 << 24, False, False, 1 << 20, [0, 5])
    ts = (1 << 23) * 10
    assert ts * ts * (1 << 20) >= 1 << 63 > 200 * 200 * 4


def test_a_stride_means_every_stride_th_step():
    assert PD._cov_steps(7, 220).tolist() == list(range(0, 221, 7)) and len(PD._cov_steps(7, 220)) == 32
    assert PD._cov_steps(1, 5).tolist() == [0, 1, 2, 3, 4, 5]
    assert PD._cov_steps(np.array([0, 220]), 220).dtype == np.int64
    import torch
    assert PD._cov_steps(torch.tensor([0, 3, 220], dtype=torch.int32), 220).tolist() == [0, 3, 220]


@pytest.mark.parametrize("extra,part", [
    (["--rng", "numpy"], "Philox mode only"), (["--sweep", "small"], "--sweep chooses the sweep decoder"),
    (["--local-tables", "on"], "--local-tables chooses the tables"), (["--pick", "best"], "--pick takes first, multi or auto"),
])
def test_the_command_line_refuses_with_the_reason(monkeypatch, tmp_path, extra, part):
    monkeypatch.setattr(PD, "simulate_pd_covariance", lambda *a, **k: pytest.fail("ran"))
    argv = [str(tmp_path / "o.pkl"), "4", "8", "10", "40", "0.45", "N", "U", "4", "7"] + extra
    with pytest.raises(SystemExit) as ei:
        PD.main_simulate_covariance(argv)
    assert part in str(ei.value)
    assert not (tmp_path / "o.pkl").exists()


def test_the_command_line_wants_its_ten_arguments(tmp_path):
    with pytest.raises(SystemExit, match="OUT l r L M e"):
        PD.main_simulate_covariance([str(tmp_path / "o.pkl"), "4", "8", "10", "40", "0.45", "N", "U", "4"])


def test_the_command_line_passes_its_options_and_writes_arrays_only(monkeypatch, tmp_path):
    seen = {}

    def fake(e, l, r, L, M, term, proto, runs, steps, **kw):
        seen.update(args=(e, l, r, L, M, term, proto, runs, steps), kw=kw)
        return (np.arange(3, dtype=np.int64), np.ones((3, 3, 3), np.int64), np.zeros((3, 9), np.int64), np.array([0.25, 0.5]))
    monkeypatch.setattr(PD, "simulate_pd_covariance", fake)
    out = tmp_path / "o.pkl"
    PD.main_simulate_covariance([str(out), "4", "8", "10", "40", "0.45", "T", "P", "2", "7", "--seed", "5", "--batch", "16",
                                 "--pick", "first", "--device", "cpu", "--rng", "philox"])
    assert seen["args"] == (0.45, 4, 8, 10, 40, True, True, 2, 7)
    assert seen["kw"] == dict(seed=5, batch=16, pick="first", device="cpu")
    with open(out, "rb") as f:
        steps, gram, mom, plrs = PD._ArraysOnly(f).load()
    assert steps.tolist() == [0, 1, 2] and gram.shape == (3, 3, 3) and mom.shape == (3, 9) and plrs.tolist() == [0.25, 0.5]


# ---- cov_from_gram against exact rationals ------------------------------------------------------------------------------------
def gram_of(x):
    x = np.asarray(x, dtype=object)
    m = (x != 0).astype(int).astype(object)
    return np.stack([m.T @ m, x.T @ m, x.T @ x]).astype(np.int64)


def exact_cov(x):
    T, K = x.shape
    out = np.empty((K, K), dtype=object)
    for i in range(K):
        for j in range(K):
            both = [t for t in range(T) if x[t, i] != 0 and x[t, j] != 0]
            n = len(both)
            if n == 0:
                out[i, j] = None
                continue
            si, sj = sum(int(x[t, i]) for t in both), sum(int(x[t, j]) for t in both)
            sij = sum(int(x[t, i]) * int(x[t, j]) for t in both)
            out[i, j] = Fraction(sij, n) - Fraction(si, n) * Fraction(sj, n)
    return out


def rows(name):
    rng = np.random.default_rng(17)
    if name == "near-constant":                                          # x = 100 000 +- 3, T = 50
        return 100000 + rng.integers(-3, 4, size=(50, 6))
    if name == "zeros":                                                  # columns partly and wholly zero, one never zero
        x = rng.integers(1, 5000, size=(40, 7))
        x[rng.random((40, 7)) < 0.35] = 0
        x[:, 2] = 0
        x[:, 4] = np.arange(1, 41)
        x[:20, 5] = 0                                                    # 5 and 6 are never non-zero together
        x[20:, 6] = 0
        return x
    if name == "constant":                                               # zero variance comes out as exactly 0
        return np.full((30, 3), 12345) + np.array([0, 1, 2])
    if name == "wide":                                                   # g0 * Σ(x_i - k_i)(x_j - k_j) = 4 * 2^60: beyond int64
        x = np.empty((4, 5), dtype=np.int64)
        for j in range(5):
            x[:, j] = 1 + j
            x[j % 2::2, j] = (1 << 30) - 1 - j
        return x
    if name == "decaying":                                               # trajectories that die out at different steps
        x = np.maximum(0, 300 - 30 * np.arange(12)[None, :] + rng.integers(-40, 40, size=(200, 12)))
        x[np.cumsum(x == 0, axis=1) > 0] = 0
        return x
    raise KeyError(name)


@pytest.mark.parametrize("name", ["near-constant", "zeros", "constant", "wide", "decaying"])
def test_cov_from_gram_against_fractions(name):
    x = rows(name)
    g = gram_of(x)
    cov, counts = PD.cov_from_gram(g)
    want = exact_cov(x)
    assert counts.dtype == np.int64 and (counts == g[0]).all() and cov.dtype == np.float64
    K = x.shape[1]
    for i in range(K):
        for j in range(K):
            if want[i, j] is None:
                assert counts[i, j] == 0 and np.isnan(cov[i, j]), (i, j)
                continue
            assert counts[i, j] > 0 and not np.isnan(cov[i, j]), (i, j)
            w = want[i, j]
            if w == 0:
                assert cov[i, j] == 0.0, (i, j, cov[i, j])
            else:
                assert abs(Fraction(float(cov[i, j])) - w) <= Fraction(1, 10 ** 12) * abs(w), (name, i, j, cov[i, j], float(w))
    assert (np.isnan(cov) == (counts == 0)).all()
    if name == "zeros":
        assert np.isnan(cov[2]).all() and np.isnan(cov[:, 2]).all() and np.isnan(cov[5, 6]) and not np.isnan(cov[4, 4])
    if name == "near-constant":
        # the textbook form g2/g0 - (g1/g0)^2 in floating point loses these digits: the test is not vacuous
        naive = g[2] / g[0] - (g[1] / g[0]) * (g[1].T / g[0])
        worst = max(abs(Fraction(float(naive[i, j])) - want[i, j]) / abs(want[i, j]) for i in range(K) for j in range(K) if want[i, j])
        assert worst > Fraction(1, 10 ** 9)


def test_cov_from_gram_refuses_other_shapes():
    for bad in (np.zeros((2, 3, 3), np.int64), np.zeros((3, 2, 3), np.int64), np.zeros((3, 3, 3))):
        with pytest.raises(ValueError):
            PD.cov_from_gram(bad)
