"""Exact per-frame erasure thresholds on the CPU: the symbols of the extension header include/scldpc_thresh.h, every check its
entries decide before any device work (placeholder pointers that are never dereferenced, as tests/test_bp_eps_host.py), the
workspace query, the definition of T* in numpy (the bisection inside the residual against direct fixpoints, and T* - 1 = the
largest key of the critical residual), the host logic of bp_decoding.run_thresholds over an engine fake, and the exits of the
bp_thresholds command line.  host_fixpoint and host_bisect are the references of tests/test_gpu_thresh.py as well."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as BP
from fl_scaling_sc_ldpc_amd import engine as E
from test_bp_eps_host import numpy_code
from test_eps_host import QCAP, WORKSPACE_M

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_thresh.h")
KEYS, FT, FT16 = "scldpc_channel_keys_device", "scldpc_frame_threshold_device", "scldpc_frame_threshold_device_adj16"
QUERY = "scldpc_frame_threshold_workspace_query"
TMAX = 2147483647


def err():
    return _lib.lib().scldpc_last_error().decode()


# ---- the references: numpy ------------------------------------------------------------------------------------------------
def host_fixpoint(adj, U, cn_lim, ncn):
    """The maximal stopping set inside the bool set U over the CNs below cn_lim, by flooding rounds like
    test_gpu_bp_eps.host_rounds: every CN < cn_lim that holds one VN of the set releases it, until none does.
    adj: int [n, dv], global CN ids."""
    idx = np.flatnonzero(U)
    while idx.size:
        a = adj[idx]
        fire = np.bincount(a.ravel(), minlength=ncn) == 1
        fire[cn_lim:] = False
        lone = fire[a].any(axis=1)
        if not lone.any():
            break
        idx = idx[~lone]
    out = np.zeros(U.shape, dtype=bool)
    out[idx] = True
    return out


def host_bisect(adj, keys, t_lo, t_hi, cn_lim, ncn, vns_pos):
    """The issue's search, without the cut of the upper end: (thresh, status, size, first position, last position, #key < t_hi)
    and the critical residual as a bool vector.  keys: uint32-valued integers [n]."""
    keys = np.asarray(keys, dtype=np.int64)
    erased = int((keys < t_hi).sum())
    R = host_fixpoint(adj, keys < t_hi, cn_lim, ncn)
    if not R.any():
        return [-1, 1, 0, -1, -1, erased], R
    low = host_fixpoint(adj, R & (keys < t_lo), cn_lim, ncn)
    if low.any():
        R, thresh, status = low, t_lo, 2
    else:
        lo, hi = t_lo, t_hi
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            U = host_fixpoint(adj, R & (keys < mid), cn_lim, ncn)
            if U.any():
                R, hi = U, mid
            else:
                lo = mid
        thresh, status = hi, 0
    at = np.flatnonzero(R)
    return [thresh, status, int(at.size), int(at[0]) // vns_pos, int(at[-1]) // vns_pos, erased], R


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_THRESH) and len(declared) == 4
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
              | set(_lib.EXPORTS_COV) | set(_lib.EXPORTS_SS) | set(_lib.EXPORTS_RUNS) | set(_lib.EXPORTS_EPS)
              | set(_lib.EXPORTS_BP_EPS))
    assert not declared & others                                         # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name               # bound with a signature
    assert '#include "scldpc_bp_eps.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_thresh.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    assert "_lib.EXPORTS_THRESH" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "#define SCLDPC_THRESH_NCOLS 8" in text and _lib.THRESH_NCOLS == 8 == len(_lib.THRESH_NAMES)
    assert "#define SCLDPC_THRESH_MAX 2147483647u" in text and _lib.THRESH_MAX == TMAX == E.erasure_threshold(1.0)


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_thresh.h"\nint main(void){'
                   'int (*k)(const scldpc_code_params *, uint64_t, uint64_t, int32_t, int32_t, const int32_t *, uint32_t *, void *)'
                   ' = scldpc_channel_keys_device;'
                   'int (*g)(const scldpc_code_params *, int32_t, const int32_t *, const uint32_t *, uint32_t, uint32_t, int32_t,'
                   ' int32_t *, uint32_t *, void *, uint64_t, void *) = scldpc_frame_threshold_device;'
                   'int (*h)(const scldpc_code_params *, int32_t, const uint16_t *, const uint32_t *, uint32_t, uint32_t, int32_t,'
                   ' int32_t *, uint32_t *, void *, uint64_t, void *) = scldpc_frame_threshold_device_adj16;'
                   'int64_t (*w)(const scldpc_code_params *, int32_t, int32_t) = scldpc_frame_threshold_workspace_query;'
                   'return (k==0)+(g==0)+(h==0)+(w==0)+SCLDPC_THRESH_NCOLS-8+(SCLDPC_THRESH_MAX!=2147483647u);}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the checks decided before any device work ----------------------------------------------------------------------------
def keys_call(p=None, T=1, doped=(), out=ONE, ndoped=None):
    p = E.make_params(4, 8, 12, 32) if p is None else p
    darr, dptr = _lib.doped_array(doped)
    rc = _lib.lib().scldpc_channel_keys_device(C.byref(p), 1, 0, T, darr.size if ndoped is None else ndoped, dptr, out, None)
    return rc, err()


def test_the_keys_entry_refuses_with_a_text_and_no_device():
    """scldpc_channel_levels_device's checks and their order, without the grid."""
    rc, msg = keys_call(p=E.CodeParams(3, 6, 10, 64, 127))
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = keys_call(p=E.CodeParams(3, 6, 10, 64, 127), T=-1)         # the parameters come first
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = keys_call(T=-1)
    assert rc == BAD_ARG and msg == KEYS + ": null buffer or negative ntrials"
    rc, msg = keys_call(out=None)
    assert rc == BAD_ARG and msg == KEYS + ": null buffer or negative ntrials"
    rc, msg = keys_call(out=None, doped=list(range(33)))                 # the buffer before the doping
    assert rc == BAD_ARG and msg == KEYS + ": null buffer or negative ntrials"
    rc, msg = keys_call(doped=list(range(33)))
    assert rc == BAD_ARG and "0 <= ndoped <= 32" in msg
    rc, msg = keys_call(ndoped=-1)
    assert rc == BAD_ARG and "0 <= ndoped <= 32" in msg
    rc, msg = keys_call(ndoped=2)                                        # positions announced, none given
    assert rc == BAD_ARG and "0 <= ndoped <= 32" in msg
    rc, msg = keys_call(doped=[12])
    assert rc == BAD_ARG and msg == "doped position 12 outside [0,12)"
    rc, msg = keys_call(doped=[-1])
    assert rc == BAD_ARG and msg == "doped position -1 outside [0,12)"
    assert keys_call(T=0, out=None)[0] == OK                             # an empty batch touches nothing
    assert keys_call(T=0, out=None, doped=[12])[0] == OK                 # ... and is judged no further, as the levels entry's


def entry_call(p=None, T=1, adj=ONE, keys=ONE, lo=100, hi=200, is_term=1, out=ONE, bits=None, ws=None, wsb=0, entry=FT16):
    p = E.make_params(4, 8, 12, 32) if p is None else p
    rc = getattr(_lib.lib(), entry)(C.byref(p), T, adj, keys, lo, hi, is_term, out, bits, ws, wsb, None)
    return rc, err()


@pytest.mark.parametrize("entry", [FT, FT16])
def test_the_entries_refuse_with_a_text_and_no_device(entry):
    """full_bp_eps's order and wording: the parameters, null buffers, the window, the empty batch, the limits, the LDS, the
    workspace.  Each call below is wrong in one thing only, except where the order itself is shown."""
    window = "%s: 0 <= t_lo < t_hi <= 2147483647 (got t_lo = %d, t_hi = %d)"
    rc, msg = entry_call(p=E.CodeParams(3, 6, 10, 64, 127), entry=entry)
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = entry_call(p=E.CodeParams(3, 6, 10, 64, 127), T=-1, lo=5, hi=5, entry=entry)      # the parameters come first
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = entry_call(T=-1, entry=entry)
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for kw in (dict(adj=None), dict(keys=None), dict(out=None)):
        rc, msg = entry_call(entry=entry, **kw)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials", kw
    rc, msg = entry_call(out=None, lo=5, hi=5, entry=entry)              # the buffers before the window
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for lo, hi in ((5, 5), (6, 5), (0, 0), (TMAX, TMAX), (0, TMAX + 1), (7, 0xFFFFFFFF)):
        rc, msg = entry_call(lo=lo, hi=hi, entry=entry)
        assert rc == BAD_ARG and msg == window % (entry, lo, hi), (lo, hi, msg)
    rc, msg = entry_call(lo=9, hi=9, T=0, adj=None, keys=None, out=None, entry=entry)   # the window before the empty batch
    assert rc == BAD_ARG and msg == window % (entry, 9, 9)
    for lo, hi in ((0, 1), (0, TMAX), (TMAX - 1, TMAX)):
        assert entry_call(lo=lo, hi=hi, T=0, adj=None, keys=None, out=None, entry=entry)[0] == OK   # an empty batch touches nothing
    assert entry_call(p=E.CodeParams(9, 18, 4, 8, 16), T=0, entry=entry)[0] == OK        # ... and is judged no further
    for is_term in (0, 1):
        rc, msg = entry_call(p=E.CodeParams(9, 18, 4, 8, 16), is_term=is_term, entry=entry)     # dc = 18 > 15
        assert rc == TOO_LARGE and msg == entry + ": needs dc <= 15, dv <= 8, dc*n < 2^24"
    huge = E.make_params(3, 6, 64, 1 << 15)                              # two VN bitmaps of 64 K words: beyond one CU's LDS
    rc, msg = entry_call(p=huge, entry=entry)
    assert rc == TOO_LARGE and msg.startswith(entry + ": ") and "do not fit 160 KiB of LDS" in msg
    big = E.make_params(4, 8, 50, 5000)                                  # the words go to the workspace: none given
    rc, msg = entry_call(p=big, T=2, entry=entry)
    assert rc == BAD_ARG and "workspace" in msg
    rc, msg = entry_call(p=big, T=2, ws=ONE, wsb=2 * 4 * big.nk - 1, entry=entry)        # ... or one byte short
    assert rc == BAD_ARG and "workspace" in msg


def test_the_workspace_query_answers_without_a_device():
    lib = _lib.lib()
    q = lambda p, T, a16: lib.scldpc_frame_threshold_workspace_query(C.byref(p), T, a16)
    small, bench, big = E.make_params(4, 8, 12, 16), E.make_params(4, 8, 50, 1000), E.make_params(4, 8, 50, 5000)
    for T in (0, 1, 77):
        for a16 in (0, 1):
            assert q(small, T, a16) == 0 and q(bench, T, a16) == 0       # the words stay in LDS
            assert q(big, T, a16) == T * 4 * big.nk                      # 32-bit words in the workspace, one slice per frame
    wsp = E.make_params(4, 8, 50, WORKSPACE_M)
    for T in (1, 4):
        assert q(wsp, T, 0) == 4 * wsp.nk * T > 0                        # int32 rows at the GPU tests' workspace shape
    assert E.frame_threshold_workspace_bytes(wsp, 4, False) == 4 * 4 * wsp.nk
    assert E.frame_threshold_workspace_bytes(small, 256, True) == 0
    for pair in ((3, 6), (5, 10)):
        assert q(E.make_params(*pair, 50, 1000), 5, 1) == 0
    # the shape rule is full_bp_eps's, shape for shape
    for M in range(1300, 1340, 2):
        pm = E.make_params(4, 8, 50, M)
        assert q(pm, 3, 0) == lib.scldpc_full_bp_eps_workspace_query(C.byref(pm), 3, 0), M
    assert q(E.CodeParams(3, 6, 10, 64, 127), 1, 0) == BAD_ARG and "must equal" in err()
    huge = E.make_params(3, 6, 64, 1 << 15)
    assert q(huge, 1, 0) == TOO_LARGE and "do not fit 160 KiB of LDS" in err() and err().startswith(QUERY + ": ")
    with pytest.raises(E.ScldpcError, match="LDS"):
        E.frame_threshold_workspace_bytes(huge, 1, False)


def test_the_queue_cap_is_read_per_call_and_changes_no_answer(monkeypatch):
    p = E.make_params(4, 8, 12, 32)
    for v in ("8", "0", "-5", "100000"):
        monkeypatch.setenv(QCAP, v)
        assert _lib.lib().scldpc_frame_threshold_workspace_query(C.byref(p), 3, 1) == 0
        assert entry_call(lo=3, hi=3)[0] == BAD_ARG


def test_the_engine_refuses_before_it_allocates(monkeypatch):
    monkeypatch.setattr(E, "_require_gpu", lambda: None)
    monkeypatch.setattr(E, "_uninit", lambda *a, **k: pytest.fail("allocated before the call was checked"))
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        E.frame_threshold(E.make_params(4, 8, 12, 16), None, None, -1, 5)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        E.frame_threshold(E.make_params(4, 8, 12, 16), None, None, 0, 1 << 32)


# ---- the definition, in numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,r,L,N,is_term,window", [(4, 8, 12, 16, 1, (0.40, 0.50)), (3, 6, 10, 20, 1, (0.40, 0.50)),
                                                    (3, 6, 10, 20, 0, (0.20, 0.40))],
                         ids=["4-8-terminated", "3-6-terminated", "3-6-truncated"])
def test_the_bisection_finds_the_least_failing_threshold(l, r, L, N, is_term, window):
    """100 codes with integer keys: the bisection's T* has a non-empty fixpoint at T* and an empty one at T* - 1; the largest key
    of the critical residual is T* - 1 (what lets the kernel cut the upper end); and at six thresholds across the window the
    number of codes with T* <= t is the number of codes whose direct fixpoint at t is non-empty.
    Pure numpy: this pins the REFERENCE (host_bisect against host_fixpoint) and the identity the kernel rests on, not the product,
    so it passes without the feature; the tests that fail without it are the engine-fake and command-line tests of this file
    and the comparisons of tests/test_gpu_thresh.py, which hold the kernel to this reference."""
    p = E.make_params(l, r, L, N)
    cn_lim = p.nk if is_term else p.L * p.cns_pos
    t_lo, t_hi = E.erasure_threshold(window[0]), E.erasure_threshold(window[1])
    ts = [int(t) for t in np.linspace(t_lo, t_hi, 6)]
    by_rows, direct, statuses, sizes = np.zeros(6, dtype=int), np.zeros(6, dtype=int), [0, 0, 0], []
    for seed in range(100):
        rng = np.random.RandomState(seed)
        adj = numpy_code(l, r, L, N, rng)
        keys = rng.randint(0, 1 << 31, size=p.n).astype(np.int64)
        row, R = host_bisect(adj, keys, t_lo, t_hi, cn_lim, p.nk, p.vns_pos)
        thresh, status = row[0], row[1]
        statuses[status] += 1
        assert row[5] == int((keys < t_hi).sum())
        if status == 0:
            assert t_lo < thresh <= t_hi
            at = host_fixpoint(adj, keys < thresh, cn_lim, p.nk)
            assert at.any() and (at == R).all(), seed                    # S(T*) is the critical residual
            assert not host_fixpoint(adj, keys < thresh - 1, cn_lim, p.nk).any(), seed
            assert int(keys[R].max()) == thresh - 1, seed
            sizes.append(row[2])
        elif status == 2:
            assert (R == host_fixpoint(adj, keys < t_lo, cn_lim, p.nk)).all() and R.any() and thresh == t_lo
        else:
            assert not R.any() and not host_fixpoint(adj, keys < t_hi, cn_lim, p.nk).any() and row[:5] == [-1, 1, 0, -1, -1]
        if status != 1:
            at = np.flatnonzero(R)
            assert row[2:5] == [at.size, at[0] // p.vns_pos, at[-1] // p.vns_pos] and row[2] >= 2
        for i, t in enumerate(ts):
            by_rows[i] += status == 2 or (status == 0 and thresh <= t)
            direct[i] += host_fixpoint(adj, keys < t, cn_lim, p.nk).any()
    print("status 0 / 1 / 2:", statuses, "| failing codes at the six thresholds:", direct.tolist(),
          "| critical residuals:", (min(sizes), int(np.median(sizes)), max(sizes)) if sizes else None)
    assert (by_rows == direct).all(), (by_rows, direct)
    assert statuses[0] >= 30                                             # the window holds thresholds


# ---- the host logic of run_thresholds over an engine fake ---------------------------------------------------------------------
def fake_row(frame, t_lo, t_hi):
    """A frame's row: a hash of the frame places its threshold below, inside or above the window."""
    h = (frame * 2654435761 + 12345) % 1000
    if h < 100:
        return [t_lo, 2, 9 + frame % 5, 1, 3, 2, 0, 40 + frame % 7]
    if h >= 800:
        return [-1, 1, 0, -1, -1, 1, 0, 40 + frame % 7]
    return [t_lo + 1 + (h - 100) * ((t_hi - t_lo - 1) // 700), 0, 2 + frame % 30, 2, 2 + frame % 3, 12, 0, 40 + frame % 7]


class FakeEngine:
    """Stands in for the engine calls of run_thresholds on CPU tensors and records them."""

    def __init__(self, monkeypatch, index, seed, doped=()):
        self.rounds, self.state, self.index, self.seed, self.doped = [], None, index, seed, tuple(doped)
        for name in ("sample_philox", "channel_keys", "frame_threshold"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device="cpu", out=None, adj16=False, ensemble="olmos"):
        assert self.state is None, "one sampler call per round"
        assert seed == self.seed and out is not None and out[0].dtype == torch.int16 and out[0].shape == (ntrials, p.n, p.dv)
        frame0 = trial0 - BP.trial_key(self.index, 0, 0)
        assert 0 <= frame0 < BP.POINT_STRIDE and trial0 == BP.trial_key(self.index, 0, frame0)     # the key of point 0
        assert tuple(doped) == self.doped
        self.state = [frame0, ntrials, eps, False]
        return out

    def channel_keys(self, p, seed, trial0, ntrials, doped=(), device="cpu", out=None):
        assert seed == self.seed and trial0 == BP.trial_key(self.index, 0, self.state[0]) and ntrials == self.state[1]
        assert tuple(doped) == self.doped and out.shape == (ntrials, p.n) and out.dtype == torch.int32
        self.state[3] = True
        return out

    def frame_threshold(self, p, d_adj, d_keys, t_lo, t_hi, is_term=True, want_bits=False, rows=None):
        frame0, ntrials, eps, keyed = self.state
        assert keyed and d_adj.shape[0] == ntrials == d_keys.shape[0] and is_term
        assert rows.shape == (ntrials, 8) and rows.is_contiguous() and rows.dtype == torch.int32
        self.rounds.append((frame0, ntrials, eps, t_lo, t_hi))
        self.state = None
        for t in range(ntrials):
            rows[t] = torch.tensor(fake_row(frame0 + t, t_lo, t_hi), dtype=torch.int32)
        bits = torch.full((ntrials, p.nw), 0, dtype=torch.int32) if want_bits else None
        if want_bits:
            bits[:, 0] = torch.arange(frame0, frame0 + ntrials, dtype=torch.int32)
        return {"rows": rows, "bits": bits}


def test_the_frames_over_a_fake_engine(monkeypatch):
    fake = FakeEngine(monkeypatch, index=3, seed=9, doped=(2,))
    p = E.make_params(4, 8, 12, 16)
    t_lo, t_hi = E.erasure_threshold(0.40), E.erasure_threshold(0.50)
    res = BP.run_thresholds(p, 0.40, 0.50, 150, seed=9, index=3, doped=(2,), batch=64, device="cpu", want_bits=True)
    want = np.array([fake_row(f, t_lo, t_hi) for f in range(150)], dtype=np.int64)
    assert res.rows.dtype == np.int64 and res.rows.shape == (150, 8) and (res.rows == want).all()         # in frame order
    assert (res.t_lo, res.t_hi) == (t_lo, t_hi)
    assert [r[:2] for r in fake.rounds] == [(0, 64), (64, 64), (128, 22)]                                 # a last partial batch
    assert all(r[2:] == (0.50, t_lo, t_hi) for r in fake.rounds)
    assert res.bits.dtype == np.uint32 and res.bits.shape == (150, p.nw) and (res.bits[:, 0] == np.arange(150)).all()
    star = res.eps_star()
    inside = want[:, 1] == 0
    assert star.dtype == np.float64 and np.isnan(star[~inside]).all() and (star[inside] == want[inside, 0] / 2147483647.0).all()
    assert 20 <= inside.sum() <= 140 and (want[:, 1] == 1).any() and (want[:, 1] == 2).any()
    es = [0.40, 0.4001, 0.43, 0.46, 0.4999, 0.50]
    got = res.fer_at(es)
    count = [sum(1 for r in want if r[1] == 2 or (r[1] == 0 and r[0] <= E.erasure_threshold(e))) for e in es]
    assert got.tolist() == count and got[0] == (want[:, 1] == 2).sum() and got[-1] == (want[:, 1] != 1).sum()
    assert len(set(count)) >= 4
    for e in (0.39, 0.5001, float(np.nextafter(0.40, 0.0)) - 1e-9):
        with pytest.raises(ValueError, match="outside the window"):
            res.fer_at([0.45, e])
    bare = BP.run_thresholds(p, 0.40, 0.50, 64, seed=9, index=3, doped=(2,), batch=64, device="cpu")
    assert bare.bits is None and (bare.rows == want[:64]).all()
    none = BP.run_thresholds(p, 0.40, 0.50, 0, seed=9, index=3, doped=(2,), batch=64, device="cpu")
    assert none.rows.shape == (0, 8) and none.fer_at([0.45]).tolist() == [0]


def test_run_thresholds_refuses_before_it_allocates(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the call was checked")
    for name in ("sample_philox", "channel_keys", "frame_threshold", "local_device", "_require_gpu", "_uninit"):
        monkeypatch.setattr(E, name, no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    p = E.make_params(4, 8, 12, 16)
    with pytest.raises(ValueError, match=r"^thresholds: .*scldpc_frame_threshold_workspace_query: .*do not fit 160 KiB of LDS"):
        BP.run_thresholds(E.make_params(3, 6, 64, 1 << 15), 0.40, 0.50, 10, seed=1)
    with pytest.raises(ValueError, match=r"^thresholds: .*dc <= 15"):
        BP.run_thresholds(E.CodeParams(9, 18, 4, 8, 16), 0.40, 0.50, 10, seed=1)
    for lo, hi in ((0.5, 0.4), (0.45, 0.45), (0.45, float(np.nextafter(0.45, 0.0))), (-0.1, 0.4), (0.4, 1.1)):
        with pytest.raises(ValueError, match=r"^thresholds: the window"):
            BP.run_thresholds(p, lo, hi, 10, seed=1)


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_the_command_line_exits_before_any_device_work(monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("device work before the command line was checked")
    for name in ("sample_philox", "channel_keys", "frame_threshold", "local_device", "_require_gpu", "init_distributed"):
        monkeypatch.setattr(E, name, no_device)
    monkeypatch.setattr(BP, "run_thresholds", no_device)
    out = ["--outdir", str(tmp_path / "o"), "--N", "16", "--L", "12"]

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            BP.bp_thresholds(out + argv)                                 # (an option given twice: the later one holds)
        code = str(e.value.code)
        assert code.startswith("bp_thresholds: ") and text in code, code
    refused(["0", "5", "0", "100"], "W = 5")
    refused(["0", "0", "0", "0"], "FRAMES = 0")
    refused(["0", "0", "0", "-3"], "FRAMES = -3")
    refused(["0", "0", "0", "100", "--eps-lo", "0.48", "--eps-hi", "0.44"], "the window needs")
    refused(["0", "0", "0", "100", "--eps-lo", "0.45", "--eps-hi", "0.45"], "the window needs")
    refused(["0", "0", "0", "100", "--eps-hi", "1.5"], "the window needs")
    refused(["0", "0", "2", "100", "3"], "NUM_DOPED=2 but only 1 position arguments")
    refused(["0", "0", "1", "100", "12"], "doped positions outside [0,12)")
    refused(["0", "0", "0", "100", "--dv", "3", "--dc", "6", "--L", "64", "--N", "32768"], "scldpc_frame_threshold_workspace_query: ")
    refused(["0", "0", "0", "100", "--dv", "9", "--dc", "18", "--N", "16", "--L", "4"], "dc <= 15")
    refused(["0", "0", "0", "100", "--N", "15"], "divisible")
    assert not os.path.exists(str(tmp_path / "o"))
    # a command line that passes: the run itself is the next thing that happens
    with pytest.raises(AssertionError, match="device work"):
        BP.bp_thresholds(out + ["0", "0", "1", "100", "3"])
    # the defaults: bp_lim_iter's ensemble, and its grid's last and first point as the window
    opts = BP._thresholds_parser().parse_args(["0", "0", "0", "10"])
    g = BP.DEFAULTS["bp_lim_iter"]["grid"]
    assert (opts.eps_lo, opts.eps_hi) == (g.eps(g.num_points - 1), g.eps(0)) == (0.48 - 25 * 0.00125, 0.48)
    p, doped = BP._check_thresholds(opts)
    assert p.key() == E.make_params(4, 8, 50, 1000).key() and doped == [] and opts.is_term == 1 and opts.batch == 2048
    assert BP._parser("bp_lim_iter").parse_args(["0", "0", "0", "5"]).MAX_IT == 5        # the other programs' parser is as it was
