"""Error-propagation statistics on the CPU: the two numpy references of the GPU tests (np_chain_runs, np_stream_runs, written
from the definitions in include/scldpc_runs.h) on hand-built cases and across chunk splits; the symbols of the extension header;
every refusal of its two device entries in the documented order (placeholder pointers that are never dereferenced, as
tests/test_ss_host.py); what Simulator(runs=True) and the command lines refuse before device work; and `--runs` over an engine
fake: the pickle, and a .dat that is byte for byte the one written without the switch."""
import ctypes as C
import os
import pickle
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as BP
from fl_scaling_sc_ldpc_amd import engine as E

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_runs.h")
CHAIN, STREAM = "scldpc_chain_runs_device", "scldpc_stream_runs_device"


# ---- the references of the GPU tests -----------------------------------------------------------------------------------------
def np_chain_runs(bits, L, V, acc=None):
    """bits: bool/uint8 [T, >= L * V] (anything at or beyond L * V is ignored).  Returns (acc, trial int32 [T, 4], fail_bits
    uint32 [T, ceil(L / 32)]) with acc = {"pos" [L, 4], "run_hist" [L + 1, 2], "fail_hist" [L + 1]} int64, accumulated into
    the given acc."""
    bits = np.asarray(bits)
    T = bits.shape[0]
    if acc is None:
        acc = dict(pos=np.zeros((L, 4), np.int64), run_hist=np.zeros((L + 1, 2), np.int64), fail_hist=np.zeros(L + 1, np.int64))
    pos, run_hist, fail_hist = acc["pos"], acc["run_hist"], acc["fail_hist"]
    trial = np.zeros((T, 4), np.int32)
    fail_bits = np.zeros((T, (L + 31) // 32), np.uint32)
    for t in range(T):
        e = [int(np.count_nonzero(bits[t, u * V:(u + 1) * V])) for u in range(L)]
        f = [x > 0 for x in e]
        runs, u = [], 0
        while u < L:
            if f[u]:
                s = u
                while u < L and f[u]:
                    u += 1
                runs.append((s, u - s))
            else:
                u += 1
        nfail = sum(f)
        first = f.index(True) if nfail else L
        for u in range(L):
            pos[u, 0] += f[u]
            pos[u, 1] += e[u]
            if f[u]:
                fail_bits[t, u >> 5] |= np.uint32(1) << np.uint32(u & 31)
        if nfail:
            pos[first, 2] += 1
        else:
            run_hist[0, 0] += 1
        for s, ln in runs:
            pos[s, 3] += 1
            run_hist[ln, 0] += 1
            if s + ln == L:
                run_hist[ln, 1] += 1
        fail_hist[nfail] += 1
        trial[t] = (nfail, first, len(runs), max([ln for _, ln in runs], default=0))
    return acc, trial, fail_bits


def is_doped(d, doped):
    """position_is_doped (BPF:1589-1612)."""
    if not doped:
        return False
    period = doped[-1] + 1
    return (d % period) in doped


class np_stream_runs:
    """The state machine of include/scldpc_runs.h in plain Python: feed(rows int [S, P, 10]) in any split."""

    def __init__(self, S, dv, doped, nbins, with_phase=True):
        self.ms, self.doped, self.nbins = dv - 1, tuple(doped), nbins
        self.period = self.doped[-1] + 1 if self.doped else 1
        self.carry = np.zeros((S, 8), np.int64)
        self.hist = np.zeros((4, nbins), np.int64)
        self.sums = np.zeros(8, np.int64)
        self.phase = np.zeros((self.period, 3), np.int64) if with_phase else None

    def feed(self, rows, skip=()):
        rows = np.asarray(rows)
        nb, hist, sums = self.nbins, self.hist, self.sums
        for s in range(rows.shape[0]):
            if s in skip:
                continue
            c = self.carry[s]
            for row in rows[s]:
                pos, nep = int(row[0]), int(row[1])
                if pos < self.ms:
                    continue
                d, x = pos - self.ms, nep > 0
                c[0] += 1
                sums[0] += 1
                if self.phase is not None:
                    self.phase[d % self.period] += (1, int(x), nep if x else 0)
                if x:
                    sums[1] += 1
                    sums[2] += nep
                    if c[2] == 0:
                        if c[4] == 0:
                            hist[3][min(d, nb - 1)] += 1
                        else:
                            hist[2][min(c[3], nb - 1)] += 1
                            sums[7] += c[3]
                    c[1] += 1; c[2] += 1; c[4] += 1; c[3] = 0
                else:
                    if c[1]:
                        hist[0][min(c[1], nb - 1)] += 1
                        sums[3] += 1
                        sums[4] += c[1]
                        c[1] = 0
                    if c[2] and not is_doped(d, self.doped):
                        hist[1][min(c[2], nb - 1)] += 1
                        sums[5] += 1
                        sums[6] += c[2]
                        c[2] = 0
                    c[3] += 1
        return self

    def open_hist(self):
        out = np.zeros((2, self.nbins), np.int64)
        for row, col in ((0, 1), (1, 2)):
            for v in self.carry[:, col]:
                if v > 0:
                    out[row, min(v, self.nbins - 1)] += 1
        return out

    def state(self):
        return [self.hist.tolist(), self.sums.tolist(), None if self.phase is None else self.phase.tolist(), self.carry.tolist()]


def stream_rows(x_by_d, ms, nep=None):
    """Trace rows [1, ms + len, 10] whose decided position d fails where x_by_d[d]; the first ms rows decide nothing."""
    P = ms + len(x_by_d)
    rows = np.full((1, P, 10), -7, np.int64)
    rows[0, :, 0] = np.arange(P)
    rows[0, :, 1] = 0
    for d, x in enumerate(x_by_d):
        rows[0, ms + d, 1] = (nep[d] if nep is not None else 3) if x else 0
    return rows


def test_the_chain_reference_on_hand_built_cases():
    L, V = 6, 3
    bits = np.zeros((4, L * V + 5), np.uint8)
    bits[0, [3, 4, 7]] = 1                                               # positions 1, 2: one run of 2
    bits[1, [0, 9, 15, 16, 17]] = 1                                      # positions 0, 3, 5: three runs, the last reaches L - 1
    bits[2, L * V:] = 1                                                  # beyond n only: no failure
    bits[3, :L * V] = 1                                                  # everything
    acc, trial, fb = np_chain_runs(bits, L, V)
    assert trial.tolist() == [[2, 1, 1, 2], [3, 0, 3, 1], [0, 6, 0, 0], [6, 0, 1, 6]]
    assert fb[:, 0].tolist() == [0b000110, 0b101001, 0, 0b111111]
    assert acc["pos"].tolist() == [[2, 4, 2, 2], [2, 5, 1, 1], [2, 4, 0, 0], [2, 4, 0, 1], [1, 3, 0, 0], [2, 6, 0, 1]]
    assert acc["run_hist"].tolist() == [[1, 0], [3, 1], [1, 0], [0, 0], [0, 0], [0, 0], [1, 1]]
    assert acc["fail_hist"].tolist() == [1, 0, 1, 1, 0, 0, 1]
    # L = 1: a run of one that is also the end of the chain
    acc1, trial1, fb1 = np_chain_runs(np.array([[0, 1, 0], [0, 0, 0]]), 1, 3)
    assert trial1.tolist() == [[1, 0, 1, 1], [0, 1, 0, 0]] and fb1.tolist() == [[1], [0]]
    assert acc1["pos"].tolist() == [[1, 1, 1, 1]] and acc1["run_hist"].tolist() == [[1, 0], [1, 1]] and acc1["fail_hist"].tolist() == [1, 1]
    # accumulation and split invariance
    a, _, _ = np_chain_runs(bits[:1], L, V)
    a, _, _ = np_chain_runs(bits[1:], L, V, acc=a)
    assert all((a[k] == acc[k]).all() for k in acc)


def test_the_stream_reference_on_hand_built_cases():
    ms, doped = 3, (4, 5)                                                # dv = 4, period 6, positions 4 and 5 of every period doped
    assert [is_doped(d, doped) for d in range(12)] == [False] * 4 + [True, True] + [False] * 4 + [True, True]
    assert not is_doped(5, ()) and is_doped(6, (0,)) and [is_doped(d, (1, 3)) for d in range(4)] == [False, True, False, True]
    # first failure at d = 0; the run 0..3 ends only on the doped position 4, and the EVENT lives on across 4 and 5 (both doped,
    # not failing), takes the run 6..7 in, and ends at the non-doped position 8
    x = [1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    r = np_stream_runs(1, 4, doped, 8).feed(stream_rows(x, ms))
    assert r.hist[3].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]                # time to first failure: d = 0
    assert r.hist[0].tolist() == [0, 1, 1, 0, 1, 0, 0, 0]                # runs of 4, 2 and 1
    assert r.hist[1].tolist() == [0, 1, 0, 0, 0, 0, 1, 0]                # events: 4 + 2 = 6 failing positions, then 1
    assert r.hist[2].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]                # gap between the events: positions 8, 9, 10
    assert r.sums.tolist() == [13, 7, 21, 3, 7, 2, 7, 3]
    assert r.carry.tolist() == [[13, 0, 0, 1, 7, 0, 0, 0]]
    assert r.phase.tolist() == [[3, 2, 6], [2, 2, 6], [2, 1, 3], [2, 1, 3], [2, 0, 0], [2, 1, 3]]
    # the run that fails ON a doped position keeps going: an event spanning two doped positions, still open at the end
    x2 = [0, 0, 0, 1, 1, 1, 1, 0]
    r2 = np_stream_runs(1, 4, doped, 4).feed(stream_rows(x2, ms))
    assert r2.hist[3].tolist() == [0, 0, 0, 1] and r2.hist[0].tolist() == [0, 0, 0, 1] and r2.hist[1].tolist() == [0, 0, 0, 1]
    assert r2.carry.tolist() == [[8, 0, 0, 1, 4, 0, 0, 0]] and not r2.open_hist().any()
    r3 = np_stream_runs(1, 4, doped, 4).feed(stream_rows(x2[:6], ms))
    assert r3.open_hist().tolist() == [[0, 0, 0, 1], [0, 0, 0, 1]] and not r3.hist[:3].any()     # censored: clamped to the last bin
    # nbins = 2 clamps everything to bin 1; nothing doped: period 1
    r4 = np_stream_runs(1, 4, (), 2).feed(stream_rows(x, ms))
    assert r4.period == 1 and r4.phase.tolist() == [[13, 7, 21]] and r4.hist.tolist() == [[0, 3], [0, 3], [0, 2], [1, 0]]


def synthetic_stream_rows(seed=4321, S=8, P=500, ms=3, doped=(8, 9), V=64):
    """The rows of the GPU tests' synthetic stream: bursts that doped positions cut; the other eight columns are poisoned."""
    rs = np.random.RandomState(seed)
    rows = np.full((S, P, 10), -0x0BADBEEF, np.int32)
    for s in range(S):
        x = 0
        for k in range(P):
            d = k - ms
            if d >= 0:
                x = int(rs.rand() < (0.8 if x else 0.05)) and not is_doped(d, doped)
            rows[s, k, 0] = k
            rows[s, k, 1] = rs.randint(1, V + 1) if (d >= 0 and x) else 0
    return rows


def test_the_stream_reference_is_chunk_invariant_and_gives_the_pinned_values():
    rows = synthetic_stream_rows()
    states = []
    for chunk in (64, 7, 500, 1):
        r = np_stream_runs(8, 4, (8, 9), 32)
        for k in range(0, 500, chunk):
            r.feed(rows[:, k:k + chunk])
        states.append(r.state())
    assert states[0] == states[1] == states[2] == states[3]
    assert r.sums.tolist() == [3976, 462, 14279, 167, 462, 160, 462, 3133]
    assert r.hist[0][:9].tolist() == [0, 58, 37, 25, 15, 10, 14, 3, 5]
    assert r.hist[1][10] > 0 and r.hist[1][13] > 0 and r.hist[0][10] == 0 and r.hist[0][13] == 0
    assert not r.open_hist()[0].any()


def test_the_chain_reference_gives_the_pinned_values():
    for (L, V, T, q, rho), want in SYNTH_CHAIN.items():
        acc, trial, _ = np_chain_runs(synthetic_chain_bits(L, V, T, q, rho), L, V)
        check_synthetic_chain(acc, trial, want)


SYNTH_CHAIN = {                                                          # (runs, reach end, failing, Σe)
    (12, 100, 64, .35, .05): (177, 20, 262, 1341),
    (12, 20, 64, .35, .2): (176, 19, 260, 1043),
    (70, 33, 64, .5, .1): (1116, 37, 2140, 7301),
    (50, 1000, 16, .2, .01): (139, None, 174, 1734),
}


def synthetic_chain_bits(L, V, T, q, rho):
    rs = np.random.RandomState(1234)
    g = rs.rand(T, L) < q
    return ((rs.rand(T, L, V) < rho) & g[:, :, None]).reshape(T, L * V)


def check_synthetic_chain(acc, trial, want):
    """The conditions on the INPUTS that the GPU test's shapes were chosen for, on the reference."""
    runs, reach, failing, esum = want
    assert acc["run_hist"][1:, 0].sum() == runs and acc["pos"][:, 0].sum() == failing and acc["pos"][:, 1].sum() == esum
    if reach is not None:
        assert acc["run_hist"][:, 1].sum() == reach
    L = acc["pos"].shape[0]
    if (L, runs) == (12, 177):
        assert (trial[:, 2] >= 2).sum() == 61
    if L == 70:
        assert np.count_nonzero(acc["run_hist"][1:, 0]) == 10 and trial[:, 3].max() == 15


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_RUNS) == {CHAIN, STREAM}
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
              | set(_lib.EXPORTS_COV) | set(_lib.EXPORTS_SS))
    assert not declared & others                                         # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
    raw = C.CDLL(_lib.LIB_PATH)                                         # exported by the shared object itself …
    for name in declared:
        assert C.cast(getattr(raw, name), C.c_void_p).value, name
    assert len(L.scldpc_chain_runs_device.argtypes) == 9 and len(L.scldpc_stream_runs_device.argtypes) == 13     # … and bound
    assert '#include "scldpc.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_runs.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    for name, value in (("MAX_L", 1024), ("MAX_BINS", 4096), ("MAX_PERIOD", 4096), ("CARRY", 8)):
        assert re.search(r"#define SCLDPC_RUNS_%s\s+%d\b" % (name, value), text), name
        assert getattr(_lib, "RUNS_" + name) == value == getattr(E, "RUNS_" + name)


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_runs.h"\nint main(void){'
                   'int (*f)(const scldpc_code_params *, int32_t, const uint32_t *, int64_t *, int64_t *, int64_t *, int32_t *,'
                   ' uint32_t *, void *) = scldpc_chain_runs_device;'
                   'int (*g)(const scldpc_code_params *, int32_t, int32_t, const int32_t *, const int64_t *, int32_t,'
                   ' const int32_t *, int32_t, int64_t *, int64_t *, int64_t *, int64_t *, void *) = scldpc_stream_runs_device;'
                   'return (f==0)+(g==0)+SCLDPC_RUNS_MAX_L-1024+SCLDPC_RUNS_MAX_BINS-4096+SCLDPC_RUNS_MAX_PERIOD-4096'
                   '+SCLDPC_RUNS_CARRY-8;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the checks, without a device ---------------------------------------------------------------------------------------------
def err():
    return _lib.lib().scldpc_last_error().decode()


def chain(p=None, T=1, bits=ONE, pos=ONE, rh=ONE, fh=ONE, trial=ONE, fb=ONE):
    p = E.make_params(4, 8, 12, 100) if p is None else p
    rc = _lib.lib().scldpc_chain_runs_device(C.byref(p) if p is not False else None, T, bits, pos, rh, fh, trial, fb, None)
    return rc, err()


def stream(p=None, S=1, P=1, trace=ONE, counters=ONE, doped=(), nbins=16, carry=ONE, hist=ONE, sums=ONE, phase=ONE, ndoped=None):
    p = E.make_params(4, 8, 20, 10) if p is None else p
    arr = np.ascontiguousarray(doped, dtype=np.int32)
    rc = _lib.lib().scldpc_stream_runs_device(C.byref(p), S, P, trace, counters, arr.size if ndoped is None else ndoped,
                                              arr.ctypes.data if arr.size else None, nbins, carry, hist, sums, phase, None)
    return rc, err()


def test_the_chain_entry_refuses_in_the_documented_order_and_without_a_device():
    # parameters, L, ntrials — each before the next, whatever the buffers
    rc, msg = chain(p=E.CodeParams(4, 8, 2000, 50, 99), T=-1, bits=None)
    assert rc == BAD_ARG and "must equal" in msg
    assert chain(p=False)[0] == BAD_ARG and "null" in err()
    rc, msg = chain(p=E.make_params(4, 8, 1025, 2), T=-1, bits=None)
    assert rc == TOO_LARGE and msg == CHAIN + ": L <= 1024 (got L = 1025)"
    rc, msg = chain(p=E.make_params(4, 8, 1024, 2), T=-1, bits=None)
    assert rc == BAD_ARG and msg == CHAIN + ": negative ntrials"
    # an empty batch is fine with any buffers and touches nothing
    assert chain(T=0, bits=None, pos=None, rh=None, fh=None, trial=None, fb=None)[0] == OK
    for kw in (dict(bits=None), dict(pos=None), dict(rh=None), dict(fh=None)):
        rc, msg = chain(**kw)
        assert rc == BAD_ARG and msg == CHAIN + ": null buffer", kw


def test_the_stream_entry_refuses_in_the_documented_order_and_without_a_device():
    rc, msg = stream(p=E.CodeParams(4, 8, 20, 5, 11), S=-1, nbins=1)
    assert rc == BAD_ARG and "must equal" in msg
    for kw in (dict(S=-1), dict(P=-1)):
        rc, msg = stream(nbins=1, doped=(3, 2), **kw)
        assert rc == BAD_ARG and msg == STREAM + ": negative nstreams or npos", kw
    rc, msg = stream(P=(1 << 28) + 1, nbins=1, doped=(3, 2))
    assert rc == TOO_LARGE and "npos <= 268435456" in msg
    # the doped positions: too many, missing, negative, descending, repeated — before nbins
    for kw in (dict(doped=tuple(range(33))), dict(ndoped=-1), dict(ndoped=2)):
        rc, msg = stream(nbins=1, **kw)
        assert rc == BAD_ARG and "0 <= ndoped <= 32" in msg, kw
    for doped in ((9, 8), (-1, 4), (3, 3)):
        rc, msg = stream(nbins=1, doped=doped)
        assert rc == BAD_ARG and "non-negative and ascending" in msg, doped
    for nbins in (1, 0, -4, 4097):
        rc, msg = stream(nbins=nbins, doped=(4096,), S=0)
        assert rc == BAD_ARG and msg == "%s: 2 <= nbins <= 4096 (got nbins = %d)" % (STREAM, nbins)
    # period 4097 with d_phase is refused, even for no stream; without d_phase, and period 4096 with it, are taken
    rc, msg = stream(doped=(4096,), S=0)
    assert rc == TOO_LARGE and msg == STREAM + ": d_phase takes a doping period <= 4096 (got 4097)"
    assert stream(doped=(4096,), S=0, phase=None)[0] == OK and stream(doped=(7, 4095), S=0)[0] == OK
    assert stream(nbins=2, S=0)[0] == OK and stream(nbins=4096, S=0)[0] == OK
    # nothing to do is fine with any buffers and touches nothing
    assert stream(S=0, trace=None, counters=None, carry=None, hist=None, sums=None, phase=None)[0] == OK
    assert stream(P=0, trace=None, counters=None, carry=None, hist=None, sums=None, phase=None)[0] == OK
    for kw in (dict(trace=None), dict(carry=None), dict(hist=None), dict(sums=None)):
        rc, msg = stream(**kw)
        assert rc == BAD_ARG and msg == STREAM + ": null buffer", kw


# ---- the simulators and the command lines --------------------------------------------------------------------------------------
def no_device(*a, **k):
    raise AssertionError("device work before the arguments were checked")


def block_the_device(monkeypatch):
    for name in ("sample_philox", "sample_philox_cn16", "sample_philox_sock16", "full_bp", "full_bp_cn16", "full_bp_caps_cn16", "sw_bp",
                 "chain_runs", "local_device", "_require_gpu", "new_run", "Streams", "StreamRuns", "GlibcStreamRun", "init_distributed"):
        monkeypatch.setattr(E, name, no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    monkeypatch.setattr(torch, "zeros", no_device)


def test_the_simulator_and_the_command_lines_refuse_before_any_device_work(monkeypatch, tmp_path):
    block_the_device(monkeypatch)
    p = E.make_params(4, 8, 12, 100)
    with pytest.raises(ValueError, match="^runs=True: the cap checkpoints"):
        BP.Simulator(p, max_it=50, caps=[10, 20], runs=True, device="cpu")
    common = ["--L", "12", "--N", "100", "--num-points", "1", "--max-frames", "8", "--seed", "1", "--outdir", str(tmp_path), "--quiet"]
    opts = BP._parser("bp_lim_iter").parse_args(["0", "0", "0", "50", "--runs", "--caps", "10,20"] + common)
    with pytest.raises(SystemExit, match="^--runs: the cap checkpoints of --caps keep no erased bits"):
        BP.run_program("bp_lim_iter", 0, 0, 0, 50, None, opts)
    opts = BP._parser("bp_traj").parse_args(["0", "0", "0", "50", "1", "--runs"] + common)
    with pytest.raises(SystemExit, match="^--runs: bp_traj writes trajectories"):
        BP.run_program("bp_traj", 0, 0, 0, 50, 1, opts)
    for prog, argv in (("bp_lim_iter", ["0", "0", "0", "50", "--runs", "--caps", "10,20"]), ("bp_traj", ["0", "0", "0", "50", "1", "--runs"])):
        with pytest.raises(SystemExit, match="^--runs: "):
            BP.main(prog, argv + common)                                 # … and before the job is joined
    with pytest.raises(SystemExit, match="^--nbins sizes the histograms of --runs"):
        BP.streaming(["0", "6", "0", "--nbins", "32", "--outdir", str(tmp_path)])
    for nbins in ("1", "0", "4097"):
        with pytest.raises(SystemExit, match="^--nbins: 2 <= nbins <= 4096"):
            BP.streaming(["0", "6", "0", "--runs", "--nbins", nbins, "--outdir", str(tmp_path)])
    assert os.listdir(str(tmp_path)) == []


class FakeChain:
    """The engine as pure functions of the GLOBAL trial index (CPU tensors): trial i fails (as a frame) where failing(i), and its
    "erased bits" are its own index; chain_runs adds i % L to pos so that the sums say which trials were fed."""
    L = 12

    @staticmethod
    def failing(ids):
        return ((ids * 2654435761 + 12345) >> 5) % 3 == 0

    def __init__(self, seen):
        self.seen = seen

    def install(self, mod):
        real = mod.E
        fake = types.SimpleNamespace(**{k: getattr(real, k) for k in dir(real) if not k.startswith("__")})
        seen = self.seen

        def sampler(p, seed, trial0, ntrials, eps, doped=(), device="cpu", out=None, **kw):
            ids = torch.arange(trial0, trial0 + ntrials, dtype=torch.int64) % BP.POINT_STRIDE
            out[-1][:, 0] = ids.to(torch.int32)                           # the channel words carry the trial's index
            return out

        def decoder(p, d_adj, *rest, counters=None, want_erased=False, **kw):
            d_ch = [x for x in rest if torch.is_tensor(x) and x.dtype == torch.int32 and x.dim() == 2][-1]
            ids = d_ch[:, 0].to(torch.int64)
            bad = FakeChain.failing(ids)
            counters.zero_()
            counters[:, 0] = bad.to(torch.int32) * 3
            counters[:, 1] = bad.to(torch.int32)
            return {"counters": counters, "erased": d_ch.clone() if want_erased else None, "rows": None}

        def accumulate_run(cnt, run, stop_frame_err=0):                  # plr_computation + willIstop, in trial order
            r = run.numpy()
            for row in cnt.numpy():
                if stop_frame_err > 0 and r[1] >= stop_frame_err:
                    break
                r[7] += 1; r[0] += row[0]; r[1] += row[0] > 0; r[3] += row[1]
            return run

        def chain_runs(p, d_bits, acc=None, want_trial=False, want_fail_bits=False):
            assert d_bits.shape[0] > 0 and d_bits.is_contiguous()
            acc = dict(acc) if acc is not None else {}
            for name, shape in BP.runs_shapes(p.L):
                if acc.get(name) is None:
                    acc[name] = torch.zeros(shape, dtype=torch.int64)
            ids = d_bits[:, 0].to(torch.int64)
            seen.append(ids.tolist())
            for i in ids.tolist():
                acc["pos"][i % p.L, 0] += 1
                acc["pos"][i % p.L, 1] += i
                acc["run_hist"][1 + i % p.L, 0] += 1
                acc["fail_hist"][i % (p.L + 1)] += 1
            return acc

        for name in dir(real):
            if name.startswith("sample_philox") and not name.endswith("supported"):
                setattr(fake, name, sampler)
            if name.startswith("full_bp") and not name.endswith("supported"):
                setattr(fake, name, decoder)
        fake.sw_bp, fake.accumulate_run, fake.chain_runs = decoder, accumulate_run, chain_runs
        fake.new_run = lambda device="cpu": torch.zeros(BP.NRUN, dtype=torch.int64)
        fake.local_device = lambda: torch.device("cpu")
        fake.cn_sockets = lambda p, d_adj, out=None: out
        mod.E = fake
        return real

    @staticmethod
    def want(ids, L=12):
        pos, rh, fh = np.zeros((L, 4), np.int64), np.zeros((L + 1, 2), np.int64), np.zeros(L + 1, np.int64)
        for i in ids:
            pos[i % L, 0] += 1; pos[i % L, 1] += i; rh[1 + i % L, 0] += 1; fh[i % (L + 1)] += 1
        return dict(pos=pos, run_hist=rh, fail_hist=fh)


@pytest.mark.parametrize("prog,extra", [("bp_lim_iter", []), ("bp_lim_iter", ["--window", "classical"]), ("sw_lim_iter", ["4"])])
def test_runs_writes_the_pickle_and_the_same_dat(monkeypatch, tmp_path, prog, extra):
    seen = []
    real = FakeChain(seen).install(BP)
    try:
        args = ["0", "4", "0", "4"] + [x for x in extra if not x.startswith("--") and x != "classical"]
        flags = [x for x in extra if x.startswith("--") or x == "classical"]
        common = flags + ["--L", "12", "--N", "100", "--num-points", "3", "--max-frames", "40", "--min-frame-err", "6", "--batch", "16",
                          "--seed", "1", "--quiet", "--eps-ini", "0.45", "--eps-delta", "0.01"]
        a, b = tmp_path / "plain", tmp_path / "runs"
        assert BP.main(prog, args + common + ["--outdir", str(a)]) == 0
        assert seen == []                                                # without the switch nobody asks for the pass
        assert BP.main(prog, args + common + ["--outdir", str(b), "--runs"]) == 0
    finally:
        BP.E = real
    (dat,) = os.listdir(str(a))
    assert sorted(os.listdir(str(b))) == [dat, dat + ".runs.pkl"]
    assert (a / dat).read_bytes() == (b / dat).read_bytes()
    with open(str(b / (dat + ".runs.pkl")), "rb") as f:
        points = pickle.load(f)
    assert [round(pt["eps"], 6) for pt in points] == [0.45, 0.44, 0.43] and all(sorted(pt) == ["eps", "fail_hist", "frames", "pos", "run_hist"] for pt in points)
    # every point stopped at its 6th failing frame, inside a batch: the pass saw exactly frames 0 .. frames - 1
    ids = np.arange(40)
    stop = int(np.flatnonzero(np.cumsum(FakeChain.failing(torch.from_numpy(ids)).numpy()) == 6)[0]) + 1
    assert stop < 40 and stop % 16 != 0
    fed = sorted(i for c in seen for i in c)
    assert fed == sorted(list(range(stop)) * 3)
    for pt in points:
        assert pt["frames"] == stop
        want = FakeChain.want(range(stop))
        for k in ("pos", "run_hist", "fail_hist"):
            assert pt[k].dtype == np.int64 and (pt[k] == want[k]).all(), k
