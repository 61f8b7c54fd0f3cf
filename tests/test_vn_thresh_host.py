"""Exact per-VN and per-position erasure thresholds on the CPU: the symbols of the extension header include/scldpc_vn_thresh.h,
every check its entries decide before any device work (placeholder pointers that are never dereferenced), the workspace query,
the reference host_vn_thresholds — the walk over the keys of the residual in descending order, incrementally on CN counts —
against a brute force (one fixpoint per distinct key of the window), against the local equation tau satisfies and against
tests/test_thresh_host.host_bisect, the host logic of bp_decoding.run_vn_thresholds and VnThresholds over an engine fake, and
the exits of the bp_curves command line.  host_vn_thresholds is the reference of tests/test_gpu_vn_thresh.py as well."""
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
from test_thresh_host import host_bisect, host_fixpoint

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_vn_thresh.h")
VT, VT16, QUERY = "scldpc_vn_threshold_device", "scldpc_vn_threshold_device_adj16", "scldpc_vn_threshold_workspace_query"
CCAP = "SCLDPC_DEBUG_VNT_CCAP"
TMAX = 2147483647
NONE = 0xFFFFFFFF


def err():
    return _lib.lib().scldpc_last_error().decode()


# ---- the references ------------------------------------------------------------------------------------------------------------
def host_vn_thresholds(adj, keys, t_lo, t_hi, cn_lim, ncn, vns_pos, grid=()):
    """The walk of include/scldpc_vn_thresh.h on the host, O(edges + n log n): R = the fixpoint at t_hi; the VNs of R by
    descending key, equal keys as one step; a step removes its VNs from the CN counts and peels on from every CN < cn_lim that
    is left with one VN (the sum of the ids of a CN's VNs names it), stamping everything it removes with key + 1; what is left
    below t_lo gets t_lo.  adj: int [n, dv], global CN ids; keys: uint32-valued integers [n].
    Returns dict: row = [thresh, status, |S(t_hi)|, critical size, steps, #key < t_hi] (the device's columns 0-4 and 7), tau and
    pos int64 (NONE = 0xFFFFFFFF), counts int64 [len(grid)], releases = the VNs removed by each step."""
    keys = np.asarray(keys, dtype=np.int64)
    n, dv = adj.shape
    R = host_fixpoint(adj, keys < t_hi, cn_lim, ncn)
    members = np.flatnonzero(R)
    tau = np.full(n, NONE, dtype=np.int64)
    cnt = np.bincount(adj[members].ravel(), minlength=ncn).tolist()
    ids = np.bincount(adj[members].ravel(), weights=np.repeat(members, dv), minlength=ncn).astype(np.int64).tolist()
    rows_of = adj.tolist()
    in_r = R.tolist()
    order = members[np.argsort(-keys[members], kind="stable")].tolist()
    key_of = keys.tolist()
    left, releases, i = len(order), [], 0
    while i < len(order) and left:
        m = key_of[order[i]]
        if m < t_lo:
            break
        e = i
        while e < len(order) and key_of[order[e]] == m:
            e += 1
        stack, gone = [], []

        def remove(j):
            in_r[j] = False
            gone.append(j)
            for c in rows_of[j]:
                cnt[c] -= 1
                ids[c] -= j
                if cnt[c] == 1 and c < cn_lim:
                    stack.append(c)
        for j in order[i:e]:
            if in_r[j]:
                remove(j)
        while stack:
            c = stack.pop()
            if cnt[c] == 1:
                assert in_r[ids[c]]
                remove(ids[c])
        if gone:
            tau[gone] = m + 1
            releases.append(len(gone))
            left -= len(gone)
        i = e
    rest = np.flatnonzero(np.array(in_r, dtype=bool))
    tau[rest] = t_lo
    top = int(members.size)
    status = 1 if top == 0 else 2 if rest.size else 0
    thresh = -1 if status == 1 else t_lo if status == 2 else int(tau.min())
    size = 0 if status == 1 else int(rest.size) if status == 2 else releases[-1]
    g = np.asarray(grid, dtype=np.int64).reshape(-1)
    return dict(row=[thresh, status, top, size, len(releases), int((keys < t_hi).sum())], tau=tau,
                pos=tau.reshape(-1, vns_pos).min(axis=1), counts=(tau[None, :] <= g[:, None]).sum(axis=1), releases=releases)


def host_brute_tau(adj, keys, t_lo, t_hi, cn_lim, ncn):
    """tau by its definition: one host_fixpoint of {key < t} at t_lo and at every distinct key + 1 of the window, and tau(j) the
    least of those t with j in S(t) (S changes at no other t)."""
    keys = np.asarray(keys, dtype=np.int64)
    tau = np.full(keys.size, NONE, dtype=np.int64)
    ts = sorted(set([t_lo] + [int(k) + 1 for k in keys if t_lo <= k < t_hi]))
    for t in reversed(ts):
        tau[host_fixpoint(adj, keys < t, cn_lim, ncn)] = t
    return tau


def local_equation_violations(adj, keys, tau, t_lo, cn_lim, ncn):
    """rho = tau - 1 solves rho(v) = max(key[v], max over the CNs c < cn_lim of v of min over the other members u of c in R0 of
    rho(u)) at every VN of R0 with tau > t_lo (a VN at t_lo stands for "at or below": its rho enters as t_lo - 1, which never
    decides a maximum that is at least t_lo)."""
    members = np.flatnonzero(tau != NONE)
    of_cn = [[] for _ in range(ncn)]
    for v in members:
        for c in adj[v]:
            of_cn[c].append(int(v))
    rho, bad = tau - 1, 0
    for v in members:
        if tau[v] <= t_lo:
            continue
        want = int(keys[v])
        for c in adj[v]:
            if c < cn_lim:
                others = [int(rho[u]) for u in of_cn[c] if u != v]
                assert others                                            # a CN below cn_lim never holds a VN of R0 alone
                want = max(want, min(others))
        bad += int(rho[v]) != want
    return bad


SEED0 = 1000        # seeds SEED0 … SEED0 + 99: with them both terminated (4,8) and (3,6) windows hold all three statuses
TOY = {  # key -> (l, r, L, N, is_term, tied keys)
    "4-8-terminated": (4, 8, 12, 16, 1, False), "3-6-terminated": (3, 6, 10, 20, 1, False), "3-6-truncated": (3, 6, 10, 20, 0, False),
    "5-10-terminated": (5, 10, 8, 16, 1, False), "4-8-truncated-tied": (4, 8, 12, 16, 0, True),
}


def toy_code(key, seed):
    """Code, keys and window of one of the toy configurations."""
    l, r, L, N, is_term, tied = TOY[key]
    p = E.make_params(l, r, L, N)
    rng = np.random.RandomState(SEED0 + seed)
    adj = numpy_code(l, r, L, N, rng)
    if tied:
        keys, t_lo, t_hi = rng.randint(0, 40, size=p.n).astype(np.int64), 12, 24
    else:
        keys, t_lo, t_hi = rng.randint(0, 1 << 31, size=p.n).astype(np.int64), E.erasure_threshold(0.30), E.erasure_threshold(0.55)
    return p, adj, keys, t_lo, t_hi, (p.nk if is_term else p.L * p.cns_pos)


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_VN_THRESH) and len(declared) == 3
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
              | set(_lib.EXPORTS_COV) | set(_lib.EXPORTS_SS) | set(_lib.EXPORTS_RUNS) | set(_lib.EXPORTS_EPS)
              | set(_lib.EXPORTS_BP_EPS) | set(_lib.EXPORTS_THRESH))
    assert not declared & others
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name               # bound with a signature
    assert '#include "scldpc_thresh.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_vn_thresh.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    assert "_lib.EXPORTS_VN_THRESH" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "#define SCLDPC_VNT_NCOLS 8" in text and _lib.VNT_NCOLS == 8 == len(_lib.VNT_NAMES)
    assert "#define SCLDPC_VNT_MAX_POINTS 256" in text and _lib.VNT_MAX_POINTS == 256
    assert "#define SCLDPC_VNT_NONE 0xFFFFFFFFu" in text and _lib.VNT_NONE == NONE
    assert (E.VNT_NCOLS, E.VNT_MAX_POINTS, E.VNT_NONE, E.VNT_NAMES) == (8, 256, NONE, _lib.VNT_NAMES)


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_vn_thresh.h"\nint main(void){'
                   'int (*g)(const scldpc_code_params *, int32_t, const int32_t *, const uint32_t *, uint32_t, uint32_t, int32_t,'
                   ' int32_t, const uint32_t *, int32_t *, uint32_t *, int32_t *, uint32_t *, void *, uint64_t, void *)'
                   ' = scldpc_vn_threshold_device;'
                   'int (*h)(const scldpc_code_params *, int32_t, const uint16_t *, const uint32_t *, uint32_t, uint32_t, int32_t,'
                   ' int32_t, const uint32_t *, int32_t *, uint32_t *, int32_t *, uint32_t *, void *, uint64_t, void *)'
                   ' = scldpc_vn_threshold_device_adj16;'
                   'int64_t (*w)(const scldpc_code_params *, int32_t, int32_t) = scldpc_vn_threshold_workspace_query;'
                   'return (g==0)+(h==0)+(w==0)+SCLDPC_VNT_NCOLS-8+SCLDPC_VNT_MAX_POINTS-256+(SCLDPC_VNT_NONE!=0xFFFFFFFFu)'
                   '+(SCLDPC_THRESH_MAX!=2147483647u);}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the checks decided before any device work -----------------------------------------------------------------------------------
def entry_call(p=None, T=1, adj=ONE, keys=ONE, lo=100, hi=200, is_term=1, grid=(), npoints=None, rows=ONE, pos=ONE, counts=ONE,
               tau=None, ws=None, wsb=0, entry=VT16, null_grid=False):
    p = E.make_params(4, 8, 12, 32) if p is None else p
    g = np.ascontiguousarray(grid, dtype=np.uint32)
    K = g.size if npoints is None else npoints
    gp = None if null_grid or g.size == 0 else g.ctypes.data
    rc = getattr(_lib.lib(), entry)(C.byref(p), T, adj, keys, lo, hi, is_term, K, gp, rows, pos, counts, tau, ws, wsb, None)
    return rc, err()


@pytest.mark.parametrize("entry", [VT, VT16])
def test_the_entries_refuse_with_a_text_and_no_device(entry):
    """scldpc_frame_threshold_device's order and wording, with the grid between the window and the empty batch.  Each call below
    is wrong in one thing only, except where the order itself is shown."""
    window = "%s: 0 <= t_lo < t_hi <= 2147483647 (got t_lo = %d, t_hi = %d)"
    rc, msg = entry_call(p=E.CodeParams(3, 6, 10, 64, 127), entry=entry)
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = entry_call(p=E.CodeParams(3, 6, 10, 64, 127), T=-1, lo=5, hi=5, entry=entry)      # the parameters come first
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = entry_call(T=-1, entry=entry)
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for kw in (dict(adj=None), dict(keys=None), dict(rows=None), dict(pos=None)):
        rc, msg = entry_call(entry=entry, **kw)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials", kw
    rc, msg = entry_call(rows=None, lo=5, hi=5, entry=entry)             # the buffers before the window
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for lo, hi in ((5, 5), (6, 5), (0, 0), (TMAX, TMAX), (0, TMAX + 1), (7, 0xFFFFFFFF)):
        rc, msg = entry_call(lo=lo, hi=hi, entry=entry)
        assert rc == BAD_ARG and msg == window % (entry, lo, hi), (lo, hi, msg)
    rc, msg = entry_call(lo=9, hi=9, grid=[300, 200], entry=entry)       # the window before the grid
    assert rc == BAD_ARG and msg == window % (entry, 9, 9)
    # the grid
    for K in (-1, 257):
        rc, msg = entry_call(grid=list(range(100, 101 + 99)), npoints=K, entry=entry)
        assert rc == BAD_ARG and msg == "%s: 0 <= npoints <= 256 (got npoints = %d)" % (entry, K)
    rc, msg = entry_call(lo=0, hi=1000, grid=list(range(257)), entry=entry)
    assert rc == BAD_ARG and "0 <= npoints <= 256 (got npoints = 257)" in msg
    rc, msg = entry_call(grid=[150], counts=None, entry=entry)
    assert rc == BAD_ARG and msg == entry + ": npoints = 1 needs a grid and d_counts"
    rc, msg = entry_call(grid=[150], null_grid=True, entry=entry)
    assert rc == BAD_ARG and msg == entry + ": npoints = 1 needs a grid and d_counts"
    for grid, k in (([150, 140], 1), ([150, 150], 1), ([99, 150], 0), ([100, 201], 1), ([120, 130, 125, 190], 2)):
        rc, msg = entry_call(grid=grid, entry=entry)
        assert rc == BAD_ARG and msg == "%s: the grid must ascend strictly inside [t_lo, t_hi] (grid[%d] = %d)" % (entry, k, grid[k]), msg
    rc, msg = entry_call(grid=[150, 140], T=0, adj=None, keys=None, rows=None, pos=None, counts=None, entry=entry)
    assert rc == BAD_ARG and "the grid must ascend" in msg               # the grid before the empty batch
    for grid in ((), [100], [200], [100, 200], list(range(100, 201, 1))[:256]):
        assert entry_call(grid=grid, T=0, adj=None, keys=None, rows=None, pos=None, counts=None, entry=entry)[0] == OK
    assert entry_call(p=E.CodeParams(9, 18, 4, 8, 16), T=0, entry=entry)[0] == OK        # an empty batch is judged no further
    for is_term in (0, 1):
        rc, msg = entry_call(p=E.CodeParams(9, 18, 4, 8, 16), is_term=is_term, entry=entry)     # dc = 18 > 15
        assert rc == TOO_LARGE and msg == entry + ": needs dc <= 15, dv <= 8, dc*n < 2^24"
    huge = E.make_params(3, 6, 64, 1 << 15)
    rc, msg = entry_call(p=huge, entry=entry)
    assert rc == TOO_LARGE and msg.startswith(entry + ": ") and "do not fit 160 KiB of LDS" in msg
    big = E.make_params(4, 8, 50, 5000)                                  # the words go to the workspace: none given
    rc, msg = entry_call(p=big, T=2, entry=entry)
    assert rc == BAD_ARG and "workspace" in msg
    rc, msg = entry_call(p=big, T=2, ws=ONE, wsb=2 * 4 * big.nk - 1, entry=entry)        # ... or one byte short
    assert rc == BAD_ARG and "workspace" in msg


def test_the_workspace_query_answers_without_a_device():
    lib = _lib.lib()
    q = lambda p, T, a16: lib.scldpc_vn_threshold_workspace_query(C.byref(p), T, a16)
    small, big = E.make_params(4, 8, 12, 16), E.make_params(4, 8, 50, 5000)
    for T in (0, 1, 77):
        for a16 in (0, 1):
            assert q(small, T, a16) == 0
            assert q(big, T, a16) == T * 4 * big.nk                      # the workspace form, one slice of 32-bit words per frame
    for pair in ((4, 8), (3, 6), (5, 10)):                               # the shipped size keeps its CN words in LDS
        for a16 in (0, 1):
            assert q(E.make_params(*pair, 50, 1000), 5, a16) == 0, (pair, a16)
    wsp = E.make_params(4, 8, 50, WORKSPACE_M)
    for T in (1, 4):
        assert q(wsp, T, 0) == 4 * wsp.nk * T > 0                        # int32 rows at the GPU tests' workspace shape
    for M in range(1300, 1340, 2):                                       # from n = 47 000 on the shape rule is the sibling's
        pm = E.make_params(4, 8, 50, M)
        assert q(pm, 3, 0) == lib.scldpc_frame_threshold_workspace_query(C.byref(pm), 3, 0), M
    assert E.vn_threshold_workspace_bytes(wsp, 4, False) == 4 * 4 * wsp.nk
    assert E.vn_threshold_workspace_bytes(small, 256, True) == 0
    assert q(E.CodeParams(3, 6, 10, 64, 127), 1, 0) == BAD_ARG and "must equal" in err()
    huge = E.make_params(3, 6, 64, 1 << 15)
    assert q(huge, 1, 0) == TOO_LARGE and "do not fit 160 KiB of LDS" in err() and err().startswith(QUERY + ": ")
    with pytest.raises(E.ScldpcError, match="LDS"):
        E.vn_threshold_workspace_bytes(huge, 1, False)


def test_the_debug_caps_are_read_per_call_and_change_no_answer(monkeypatch):
    p, wsp = E.make_params(4, 8, 12, 32), E.make_params(4, 8, 50, WORKSPACE_M)
    for name in (QCAP, CCAP):
        for v in ("8", "1", "0", "-5", "100000"):
            monkeypatch.setenv(name, v)
            assert _lib.lib().scldpc_vn_threshold_workspace_query(C.byref(p), 3, 1) == 0
            assert _lib.lib().scldpc_vn_threshold_workspace_query(C.byref(wsp), 3, 0) == 3 * 4 * wsp.nk
            assert entry_call(lo=3, hi=3)[0] == BAD_ARG
        monkeypatch.delenv(name)


def test_the_engine_refuses_before_it_allocates(monkeypatch):
    monkeypatch.setattr(E, "_require_gpu", lambda: None)
    monkeypatch.setattr(E, "_uninit", lambda *a, **k: pytest.fail("allocated before the call was checked"))
    p = E.make_params(4, 8, 12, 16)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        E.vn_threshold(p, None, None, -1, 5)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        E.vn_threshold(p, None, None, 0, 1 << 32)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        E.vn_threshold(p, None, None, 0, 5, grid=[1, -2])


# ---- the reference, on the toy configurations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(TOY))
def test_the_walk_equals_the_definition(key):
    """100 codes: host_vn_thresholds' tau equals the brute force at every VN; tau solves the local equation; thresh, status and
    the size of the critical residual are host_bisect's; the position minima, the counts on a grid and the steps follow from
    tau.  On the two terminated (4,8) and (3,6) configurations the window shows all three statuses, a walk of at least ten
    steps and a step that releases more than eight VNs.
    Pure numpy: this pins the REFERENCE, so it passes without the feature's kernel; the tests that hold the product to it are
    those of tests/test_gpu_vn_thresh.py, and the engine-fake and command-line tests below fail without the feature."""
    statuses, most_steps, most_release, violations = [0, 0, 0], 0, 0, 0
    for seed in range(100):
        p, adj, keys, t_lo, t_hi, cn_lim = toy_code(key, seed)
        grid = sorted(set(int(t) for t in np.linspace(t_lo, t_hi, 9)))
        ref = host_vn_thresholds(adj, keys, t_lo, t_hi, cn_lim, p.nk, p.vns_pos, grid)
        tau = ref["tau"]
        assert (tau == host_brute_tau(adj, keys, t_lo, t_hi, cn_lim, p.nk)).all(), seed
        violations += local_equation_violations(adj, keys, tau, t_lo, cn_lim, p.nk)
        row, R = host_bisect(adj, keys, t_lo, t_hi, cn_lim, p.nk, p.vns_pos)
        assert ref["row"][:2] == row[:2] and ref["row"][3] == row[2] and ref["row"][5] == row[5], (seed, ref["row"], row)
        if row[1] == 0:
            assert ((tau == row[0]) == R).all() and tau.min() == row[0]
        if row[1] == 2:
            assert ((tau == t_lo) == R).all()
        inside = tau[(tau > t_lo) & (tau != NONE)]
        assert ref["row"][4] == np.unique(inside).size == len(ref["releases"]) and sum(ref["releases"]) == inside.size
        assert ref["row"][2] == (tau != NONE).sum() == host_fixpoint(adj, keys < t_hi, cn_lim, p.nk).sum()
        assert (ref["pos"] == [tau[q * p.vns_pos:(q + 1) * p.vns_pos].min() for q in range(p.L)]).all()
        for k, g in enumerate(grid):
            assert ref["counts"][k] == host_fixpoint(adj, keys < g, cn_lim, p.nk).sum(), (seed, k)
        statuses[row[1]] += 1
        most_steps = max(most_steps, ref["row"][4])
        most_release = max(most_release, max(ref["releases"], default=0))
    print(key, "status 0 / 1 / 2:", statuses, "| most steps:", most_steps, "| largest release of a step:", most_release)
    assert violations == 0
    if key in ("4-8-terminated", "3-6-terminated"):
        assert min(statuses) >= 1 and most_steps >= 10 and most_release > 8


def test_the_reference_at_a_large_chain():
    """n = 66 000: the reference stays usable where the brute force is not (one frame, a narrow window)."""
    p = E.make_params(4, 8, 66, 1000)
    rng = np.random.RandomState(3)
    adj = numpy_code(4, 8, 66, 1000, rng)
    keys = rng.randint(0, 1 << 31, size=p.n).astype(np.int64)
    t_lo, t_hi = E.erasure_threshold(0.47), E.erasure_threshold(0.50)
    ref = host_vn_thresholds(adj, keys, t_lo, t_hi, p.nk, p.nk, p.vns_pos, [t_lo, t_hi])
    assert p.n == 66000 and ref["row"][2] > 0 and ref["counts"][1] == ref["row"][2]
    for t in (t_lo, (t_lo + t_hi) // 2, t_hi):
        assert ((ref["tau"] <= t) == host_fixpoint(adj, keys < t, p.nk, p.nk)).all()


# ---- the host logic of run_vn_thresholds over an engine fake ---------------------------------------------------------------------
def fake_frame(frame, L, n, t_lo, t_hi):
    """A frame's tau from a hash of the frame and the VN: NONE, t_lo or a value inside the window."""
    j = np.arange(n, dtype=np.int64)
    h = (j * 2654435761 + frame * 40503 + 12345) % 1000
    span = (t_hi - t_lo - 1) // 700
    tau = np.where(h >= 300 + 5 * (frame % 60), NONE, t_lo + 1 + (h % 700) * span)
    if frame % 7 in (1, 5):                                              # some VNs are lost at the bottom of the window
        tau[h < 50 + frame % 40] = t_lo
    if frame % 7 == 3:                                                   # the frame decodes at the top
        tau[:] = NONE
    return tau


class FakeEngine:
    """Stands in for the engine calls of run_vn_thresholds on CPU tensors and records them."""

    def __init__(self, monkeypatch, index, seed, doped=()):
        self.rounds, self.state, self.index, self.seed, self.doped = [], None, index, seed, tuple(doped)
        for name in ("sample_philox", "channel_keys", "vn_threshold"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device="cpu", out=None, adj16=False, ensemble="olmos"):
        assert self.state is None, "one sampler call per round"
        assert seed == self.seed and out is not None and out[0].dtype == torch.int16 and out[0].shape == (ntrials, p.n, p.dv)
        frame0 = trial0 - BP.trial_key(self.index, 0, 0)
        assert 0 <= frame0 < BP.POINT_STRIDE and trial0 == BP.trial_key(self.index, 0, frame0)
        assert tuple(doped) == self.doped
        self.state = [frame0, ntrials, eps, False]
        return out

    def channel_keys(self, p, seed, trial0, ntrials, doped=(), device="cpu", out=None):
        assert seed == self.seed and trial0 == BP.trial_key(self.index, 0, self.state[0]) and ntrials == self.state[1]
        assert tuple(doped) == self.doped and out.shape == (ntrials, p.n) and out.dtype == torch.int32
        self.state[3] = True
        return out

    def vn_threshold(self, p, d_adj, d_keys, t_lo, t_hi, grid=(), is_term=True, want_tau=False, rows=None):
        frame0, ntrials, eps, keyed = self.state
        assert keyed and d_adj.shape[0] == ntrials == d_keys.shape[0] and is_term
        assert rows.shape == (ntrials, 8) and rows.is_contiguous() and rows.dtype == torch.int32
        assert list(grid) == sorted(set(grid)) and all(t_lo <= g <= t_hi for g in grid)
        self.rounds.append((frame0, ntrials, eps, t_lo, t_hi, tuple(grid)))
        self.state = None
        tau = np.array([fake_frame(frame0 + t, p.L, p.n, t_lo, t_hi) for t in range(ntrials)])
        as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.uint32)).view(np.int32))
        rows[:] = torch.from_numpy(fake_rows(tau, t_lo).astype(np.int32))
        counts = np.array([[(t <= g).sum() for g in grid] for t in tau], dtype=np.int32).reshape(ntrials, len(grid))
        return {"rows": rows, "pos_thresh": as_i32(tau.reshape(ntrials, p.L, -1).min(axis=2)),
                "counts": torch.from_numpy(counts) if len(grid) else None, "tau": as_i32(tau) if want_tau else None}


def fake_rows(tau, t_lo):
    low = tau.min(axis=1)
    status = np.where(low == NONE, 1, np.where(low == t_lo, 2, 0))
    rows = np.zeros((tau.shape[0], 8), dtype=np.int64)
    rows[:, 0] = np.where(status == 1, -1, low)
    rows[:, 1] = status
    rows[:, 2] = (tau != NONE).sum(axis=1)
    rows[:, 3] = (tau == low[:, None]).sum(axis=1) * (status != 1)
    return rows


def test_the_frames_over_a_fake_engine(monkeypatch):
    fake = FakeEngine(monkeypatch, index=3, seed=9, doped=(2,))
    p = E.make_params(4, 8, 12, 16)
    t_lo, t_hi = E.erasure_threshold(0.40), E.erasure_threshold(0.50)
    es = [0.47, 0.40, 0.50, 0.43, 0.47]                                  # unsorted, one point twice
    grid = sorted(set(E.erasure_threshold(e) for e in es))
    res = BP.run_vn_thresholds(p, 0.40, 0.50, 150, seed=9, es=es, index=3, doped=(2,), batch=64, device="cpu", want_tau=True)
    tau = np.array([fake_frame(f, p.L, p.n, t_lo, t_hi) for f in range(150)])
    assert [r[:2] for r in fake.rounds] == [(0, 64), (64, 64), (128, 22)]                                 # a last partial batch
    assert all(r[2:] == (0.50, t_lo, t_hi, tuple(grid)) for r in fake.rounds)
    assert res.grid == grid and (res.t_lo, res.t_hi) == (t_lo, t_hi)
    assert res.rows.dtype == np.int64 and (res.rows == fake_rows(tau, t_lo)).all()                        # in frame order
    assert res.tau.dtype == np.int64 and (res.tau == tau).all()
    pos = tau.reshape(150, p.L, -1).min(axis=2)
    assert res.pos_thresh.dtype == np.int64 and (res.pos_thresh == pos).all() and (pos == NONE).any()
    assert res.counts.shape == (150, 4) and (res.counts == [[(t <= g).sum() for g in grid] for t in tau]).all()
    status = res.rows[:, 1]
    assert all((status == s).sum() >= 10 for s in (0, 1, 2))
    # the curves, at the grid's points and between them
    points = es + [0.4001, 0.46, 0.4999]
    ths = [E.erasure_threshold(e) for e in points]
    assert res.fer_at(points).tolist() == [int((tau.min(axis=1) <= th).sum()) for th in ths]
    assert (res.fer_at(points) == BP.FrameThresholds(res.rows, t_lo, t_hi).fer_at(points)).all()
    bler = res.bler_at(points)
    assert bler.dtype == np.int64 and bler.shape == (len(points), p.L)
    assert (bler == [(pos <= th).sum(axis=0) for th in ths]).all()
    assert res.block_err_at(points).tolist() == [int((pos <= th).sum()) for th in ths]
    assert res.ber_at(points).tolist() == [int((tau <= th).sum()) for th in ths]
    assert len(set(res.ber_at(points).tolist())) >= 5
    star = res.pos_eps_star()
    inside = (pos > t_lo) & (pos != NONE)
    assert star.dtype == np.float64 and star.shape == pos.shape and np.isnan(star[~inside]).all()
    assert (star[inside] == pos[inside] / 2147483647.0).all() and inside.sum() >= 100 and (~inside).sum() >= 100
    for e in (0.39, 0.5001):
        for method in (res.fer_at, res.bler_at, res.block_err_at, res.ber_at):
            with pytest.raises(ValueError, match="outside the window"):
                method([0.45, e])
    # without tau the lost VNs are known on the grid only
    bare = BP.run_vn_thresholds(p, 0.40, 0.50, 64, seed=9, es=es, index=3, doped=(2,), batch=64, device="cpu")
    assert bare.tau is None and (bare.rows == res.rows[:64]).all()
    assert bare.ber_at(es).tolist() == [int((tau[:64] <= E.erasure_threshold(e)).sum()) for e in es]
    with pytest.raises(ValueError, match="not on the grid"):
        bare.ber_at([0.46])
    assert bare.bler_at([0.46]).tolist() == [(pos[:64] <= E.erasure_threshold(0.46)).sum(axis=0).tolist()]
    gridless = BP.run_vn_thresholds(p, 0.40, 0.50, 10, seed=9, index=3, doped=(2,), batch=64, device="cpu")
    assert gridless.counts.shape == (10, 0) and gridless.grid == [] and fake.rounds[-1][5] == ()
    none = BP.run_vn_thresholds(p, 0.40, 0.50, 0, seed=9, es=es, index=3, doped=(2,), batch=64, device="cpu")
    assert none.rows.shape == (0, 8) and none.pos_thresh.shape == (0, p.L) and none.fer_at([0.45]).tolist() == [0]
    assert none.bler_at([0.45]).tolist() == [[0] * p.L] and none.ber_at([0.47]).tolist() == [0]


def test_run_vn_thresholds_refuses_before_it_allocates(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the call was checked")
    for name in ("sample_philox", "channel_keys", "vn_threshold", "local_device", "_require_gpu", "_uninit"):
        monkeypatch.setattr(E, name, no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    p = E.make_params(4, 8, 12, 16)
    with pytest.raises(ValueError, match=r"^thresholds: .*scldpc_vn_threshold_workspace_query: .*do not fit 160 KiB of LDS"):
        BP.run_vn_thresholds(E.make_params(3, 6, 64, 1 << 15), 0.40, 0.50, 10, seed=1)
    with pytest.raises(ValueError, match=r"^thresholds: .*dc <= 15"):
        BP.run_vn_thresholds(E.CodeParams(9, 18, 4, 8, 16), 0.40, 0.50, 10, seed=1)
    for lo, hi in ((0.5, 0.4), (0.45, 0.45), (-0.1, 0.4), (0.4, 1.1)):
        with pytest.raises(ValueError, match=r"^thresholds: the window"):
            BP.run_vn_thresholds(p, lo, hi, 10, seed=1)
    with pytest.raises(ValueError, match=r"^thresholds: the points of es lie outside the window"):
        BP.run_vn_thresholds(p, 0.40, 0.50, 10, seed=1, es=[0.45, 0.51])
    with pytest.raises(ValueError, match=r"^thresholds: 257 distinct thresholds"):
        BP.run_vn_thresholds(p, 0.40, 0.50, 10, seed=1, es=np.linspace(0.40, 0.50, 257))
    with pytest.raises(ValueError, match=r"^thresholds: a negative number of frames"):
        BP.run_vn_thresholds(p, 0.40, 0.50, -1, seed=1)


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_the_command_line_exits_before_any_device_work(monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("device work before the command line was checked")
    for name in ("sample_philox", "channel_keys", "vn_threshold", "frame_threshold", "local_device", "_require_gpu", "init_distributed"):
        monkeypatch.setattr(E, name, no_device)
    monkeypatch.setattr(BP, "run_vn_thresholds", no_device)
    out = ["--outdir", str(tmp_path / "o"), "--N", "16", "--L", "12"]

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            BP.bp_curves(out + argv)                                     # (an option given twice: the later one holds)
        code = str(e.value.code)
        assert code.startswith("bp_curves: ") and text in code, code
    refused(["0", "5", "0", "100"], "W = 5")
    refused(["0", "0", "0", "0"], "FRAMES = 0")
    refused(["0", "0", "0", "100", "--eps-lo", "0.48", "--eps-hi", "0.44"], "the window needs")
    refused(["0", "0", "0", "100", "--eps-hi", "1.5"], "the window needs")
    refused(["0", "0", "0", "100", "--points", "0"], "--points 0")
    refused(["0", "0", "0", "100", "--points", "257"], "--points 257")
    refused(["0", "0", "2", "100", "3"], "NUM_DOPED=2 but only 1 position arguments")
    refused(["0", "0", "1", "100", "12"], "doped positions outside [0,12)")
    refused(["0", "0", "0", "100", "--dv", "3", "--dc", "6", "--L", "64", "--N", "32768"], "scldpc_vn_threshold_workspace_query: ")
    refused(["0", "0", "0", "100", "--dv", "9", "--dc", "18", "--N", "16", "--L", "4"], "dc <= 15")
    refused(["0", "0", "0", "100", "--N", "15"], "divisible")
    assert not os.path.exists(str(tmp_path / "o"))
    with pytest.raises(AssertionError, match="device work"):             # a command line that passes: the run is what comes next
        BP.bp_curves(out + ["0", "0", "1", "100", "3"])
    # the defaults: bp_lim_iter's ensemble and its grid, point for point
    opts = BP._curves_parser().parse_args(["0", "0", "0", "10"])
    g = BP.DEFAULTS["bp_lim_iter"]["grid"]
    assert BP._curves_points(opts) == [g.eps(i) for i in range(26)] and opts.points == 26 and opts.batch == 2048
    opts = BP._curves_parser().parse_args(["0", "0", "0", "10", "--eps-lo", "0.40", "--eps-hi", "0.50", "--points", "5"])
    pts = BP._curves_points(opts)
    assert pts[0] == 0.50 and pts[-1] == 0.40 and len(pts) == 5 and np.allclose(pts, [0.50, 0.475, 0.45, 0.425, 0.40])
    assert BP._thresholds_parser().parse_args(["0", "0", "0", "5"]).FRAMES == 5 and BP._thresholds_parser().prog == "bp_thresholds"
    with pytest.raises(SystemExit) as e:                                 # the sibling's refusals keep their name
        BP.bp_thresholds(out + ["0", "5", "0", "100"])
    assert str(e.value.code).startswith("bp_thresholds: ")
