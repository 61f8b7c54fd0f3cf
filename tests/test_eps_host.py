"""The eps-descending sweep on the CPU: the symbols of the extension header include/scldpc_eps.h, every check its entries decide
before any device work (placeholder pointers that are never dereferenced, as tests/test_ss_host.py), the workspace query, the
host logic of simulate_sc_ldpc_curve over an engine fake (sorting, merging of equal thresholds, the caller's order, finished
points dropped, one sampler call per round), its refusals, the command line's --eps-fused, and the identity the decoder rests on,
R_k = residual(R_{k-1} ∩ E_k), on oracle/pd_oracle.peel_closure."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_eps.h")
LEVELS, SWEEP, SWEEP16 = "scldpc_channel_levels_device", "scldpc_peel_sweep_eps_device", "scldpc_peel_sweep_eps_device_adj16"
QCAP = "SCLDPC_DEBUG_EPS_QCAP"
ES = [0.50, 0.48, 0.46, 0.44, 0.42, 0.40]


def err():
    return _lib.lib().scldpc_last_error().decode()


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_EPS) and len(declared) == 4
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
              | set(_lib.EXPORTS_COV) | set(_lib.EXPORTS_SS) | set(_lib.EXPORTS_RUNS))
    assert not declared & others                                         # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_eps.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    assert "#define SCLDPC_EPS_MAX_POINTS 64" in text and _lib.EPS_MAX_POINTS == 64 == E.EPS_MAX_POINTS
    assert "_lib.EXPORTS_EPS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_eps.h"\nint main(void){'
                   'int (*f)(const scldpc_code_params *, uint64_t, uint64_t, int32_t, int32_t, const double *, int32_t,'
                   ' const int32_t *, uint8_t *, void *) = scldpc_channel_levels_device;'
                   'int (*g)(const scldpc_code_params *, int32_t, const int32_t *, const uint8_t *, int32_t, int32_t, int32_t, int32_t,'
                   ' int32_t *, uint32_t *, void *, uint64_t, void *) = scldpc_peel_sweep_eps_device;'
                   'int (*h)(const scldpc_code_params *, int32_t, const uint16_t *, const uint8_t *, int32_t, int32_t, int32_t, int32_t,'
                   ' int32_t *, uint32_t *, void *, uint64_t, void *) = scldpc_peel_sweep_eps_device_adj16;'
                   'int64_t (*w)(const scldpc_code_params *, int32_t, int32_t) = scldpc_peel_sweep_eps_workspace_query;'
                   'return (f==0)+(g==0)+(h==0)+(w==0)+SCLDPC_EPS_MAX_POINTS-64;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the checks decided before any device work ----------------------------------------------------------------------------
def levels(p=None, T=1, es=ES, doped=(), out=ONE, K=None):
    p = E.make_params(4, 8, 12, 32) if p is None else p
    eps = np.ascontiguousarray(es, dtype=np.float64)
    darr, dptr = _lib.doped_array(doped)
    rc = _lib.lib().scldpc_channel_levels_device(C.byref(p), 1, 0, T, len(eps) if K is None else K,
                                                 eps.ctypes.data if eps.size else None, darr.size, dptr, out, None)
    return rc, err()


def test_the_levels_entry_refuses_with_a_text_and_no_device():
    rc, msg = levels(p=E.CodeParams(3, 6, 10, 64, 127))
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = levels(T=-1)
    assert rc == BAD_ARG and msg == LEVELS + ": null buffer or negative ntrials"
    rc, msg = levels(out=None)
    assert rc == BAD_ARG and msg == LEVELS + ": null buffer or negative ntrials"
    for K, es in ((0, []), (65, list(np.linspace(0.9, 0.1, 65))), (0, ES), (-1, ES)):
        rc, msg = levels(es=es, K=K)
        assert rc == BAD_ARG and msg == "%s: 1 <= npoints <= 64 and a non-null eps (got npoints = %d)" % (LEVELS, K)
    assert levels(es=list(np.linspace(0.9, 0.1, 64)), T=0)[0] == OK      # 64 points are fine
    rc, msg = levels(es=[0.5, 0.45, 0.45, 0.4], T=0)                    # judged even for an empty batch
    assert rc == BAD_ARG and "strictly decreasing" in msg and "eps[2]" in msg
    rc, msg = levels(es=[0.4, 0.45])
    assert rc == BAD_ARG and "strictly decreasing" in msg and "eps[1]" in msg
    # two eps that round to one threshold are equal thresholds
    a = 0.45
    b = np.nextafter(a, 0.0)
    assert E.erasure_threshold(a) == E.erasure_threshold(b)
    rc, msg = levels(es=[a, b])
    assert rc == BAD_ARG and "strictly decreasing" in msg
    rc, msg = levels(es=[0.5, -0.1])
    assert rc == BAD_ARG and "outside [0,1]" in msg
    rc, msg = levels(es=[1.5])
    assert rc == BAD_ARG and "outside [0,1]" in msg
    rc, msg = levels(doped=[12])
    assert rc == BAD_ARG and msg == "doped position 12 outside [0,12)"
    rc, msg = levels(doped=list(range(33)))
    assert rc == BAD_ARG and "0 <= ndoped <= 32" in msg
    assert levels(T=0, out=None)[0] == OK                                # an empty batch touches nothing


def test_the_threshold_rule_is_the_librarys():
    # erased iff the 31-bit draw < ceil(eps * RAND_MAX)
    assert E.erasure_threshold(0.0) == 0 and E.erasure_threshold(1.0) == 2147483647 and E.erasure_threshold(0.5) == 1073741824
    assert E.erasure_threshold(0.25) == 536870912 and E.erasure_threshold(1e-12) == 1


def sweep(p=None, T=1, adj=ONE, lev=ONE, K=6, total=None, lo=0, hi=None, out=ONE, lost=None, ws=None, wsb=0, entry=SWEEP16):
    p = E.make_params(4, 8, 12, 32) if p is None else p
    total = p.nk if total is None else total
    rc = getattr(_lib.lib(), entry)(C.byref(p), T, adj, lev, K, total, lo, p.nk if hi is None else hi, out, lost, ws, wsb, None)
    return rc, err()


@pytest.mark.parametrize("entry", [SWEEP, SWEEP16])
def test_the_decoder_entries_refuse_with_a_text_and_no_device(entry):
    rc, msg = sweep(p=E.CodeParams(3, 6, 10, 64, 127), entry=entry)
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = sweep(T=-1, entry=entry)
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for kw in (dict(adj=None), dict(lev=None), dict(out=None)):
        rc, msg = sweep(entry=entry, **kw)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials", kw
    for K in (0, 65, -3):
        rc, msg = sweep(K=K, entry=entry)
        assert rc == BAD_ARG and msg == "%s: 1 <= npoints <= 64 (got npoints = %d)" % (entry, K)
    p = E.make_params(4, 8, 12, 32)
    assert p.nk == 240
    for kw in (dict(total=-1), dict(total=241), dict(lo=-1), dict(hi=241)):
        rc, msg = sweep(entry=entry, **kw)
        assert rc == BAD_ARG and msg == entry + ": CN ranges outside [0,240]", kw
    assert sweep(T=0, adj=None, lev=None, out=None, entry=entry)[0] == OK        # an empty batch touches nothing
    rc, msg = sweep(p=E.CodeParams(9, 18, 4, 8, 16), entry=entry)
    assert rc == TOO_LARGE and "dv <= 8" in msg
    huge = E.make_params(3, 6, 64, 1 << 15)                              # two VN bitmaps of 64 K words: beyond one CU's LDS
    rc, msg = sweep(p=huge, entry=entry)
    assert rc == TOO_LARGE and msg.startswith(entry) and "do not fit 160 KiB of LDS" in msg
    big = E.make_params(4, 8, 50, 5000)                                  # the words go to the workspace: none given
    rc, msg = sweep(p=big, T=2, entry=entry)
    assert rc == BAD_ARG and "workspace" in msg


def test_the_workspace_query_answers_without_a_device():
    lib = _lib.lib()
    q = lambda p, T, a16: lib.scldpc_peel_sweep_eps_workspace_query(C.byref(p), T, a16)
    small, bench, big = E.make_params(4, 8, 12, 32), E.make_params(4, 8, 50, 1000), E.make_params(4, 8, 50, 5000)
    for T in (0, 1, 77):
        for a16 in (0, 1):
            assert q(small, T, a16) == 0 and q(bench, T, a16) == 0       # the words stay in LDS
            assert q(big, T, a16) == T * 4 * big.nk                      # 32-bit words in the workspace, one slice per trial
    assert E.peel_sweep_eps_workspace_bytes(big, 3, True) == 3 * 4 * 132500
    # int32 rows, (4,8), L = 50: the smallest M (multiples of 2) whose words leave the LDS; the GPU tests use it
    m = next(M for M in range(1000, 3000, 2) if q(E.make_params(4, 8, 50, M), 1, 0))
    assert m == WORKSPACE_M and q(E.make_params(4, 8, 50, m - 2), 4, 0) == 0
    assert q(E.make_params(4, 8, 50, m), 4, 0) == 4 * 4 * E.make_params(4, 8, 50, m).nk
    assert q(E.CodeParams(3, 6, 10, 64, 127), 1, 0) == BAD_ARG and "must equal" in err()
    huge = E.make_params(3, 6, 64, 1 << 15)
    assert q(huge, 1, 0) == TOO_LARGE and "do not fit 160 KiB of LDS" in err()
    with pytest.raises(E.ScldpcError, match="LDS"):
        E.peel_sweep_eps_workspace_bytes(huge, 1, False)


WORKSPACE_M = 1324               # found by the test above (the query needs no device)


def test_the_queue_cap_is_read_per_call_and_changes_no_answer(monkeypatch):
    p = E.make_params(4, 8, 12, 32)
    for v in ("8", "0", "-5", "100000"):
        monkeypatch.setenv(QCAP, v)
        assert _lib.lib().scldpc_peel_sweep_eps_workspace_query(C.byref(p), 3, 1) == 0
        assert sweep(K=0)[0] == BAD_ARG


# ---- the host logic of the curve simulator over an engine fake ---------------------------------------------------------------
def test_curve_stages_sorts_merges_and_remembers_the_order():
    twin = float(np.nextafter(0.46, 0.0))                                # another eps with 0.46's threshold
    assert E.erasure_threshold(twin) == E.erasure_threshold(0.46)
    stage_eps, stage_of = PD.curve_stages([0.44, 0.50, twin, 0.44, 0.46, 0.42])
    assert stage_eps == [0.50, twin, 0.44, 0.42] and stage_of == [2, 0, 1, 2, 1, 3]
    th = [E.erasure_threshold(e) for e in stage_eps]
    assert all(a > b for a, b in zip(th, th[1:]))
    assert PD.curve_stages([0.3]) == ([0.3], [0])
    assert PD.curve_stages(np.array([0.1, 0.2])) == ([0.2, 0.1], [1, 0])


def fake_lost(trial, e):
    """A trial's row at eps e: fails where a hash of the trial falls below a share that grows with e."""
    h = (trial * 2654435761 + 12345) % 1000
    bad = h < int(2000 * (e - 0.38))
    return [3 + trial % 5, trial % 4, 1 + trial % 2] if bad else [0, 0, 0]


def reference_tuple(e, geo, num_repeats, max_fuckups):
    """simulate_sc_ldpc's bookkeeping and stop rule, trial by trial (PD:668-699)."""
    t = dict.fromkeys(("trials", "fuckups", "lost", "fuckups_exp", "lost_exp", "blocks_exp"), 0)
    for trial in range(num_repeats):
        lost, lost_exp, blocks = fake_lost(trial, e)
        t["trials"] += 1
        t["fuckups"] += lost >= 1
        t["lost"] += lost
        t["fuckups_exp"] += lost_exp > 0
        t["lost_exp"] += lost_exp
        t["blocks_exp"] += blocks
        if t["fuckups"] >= max_fuckups:
            break
    o1 = t["trials"]
    tg, tb = o1 * geo.generated, o1 * geo.blocks
    return (t["fuckups"] / o1, t["fuckups_exp"] / o1, t["lost"] / tg, t["lost_exp"] / tg, t["fuckups_exp"], o1, t["lost_exp"], tg,
            np.zeros(num_repeats), np.zeros(num_repeats), t["blocks_exp"], tb, t["blocks_exp"] / tb)


class FakeEngine:
    """Stands in for the five engine calls of simulate_sc_ldpc_curve on CPU tensors and records them."""

    def __init__(self, monkeypatch):
        self.rounds = []                                                 # (trial0, ntrials, eps of the sampler, es of the levels)
        self.state = None
        for name in ("sample_philox", "channel_levels", "peel_sweep_eps", "accumulate_peel", "peel_sweep_eps_workspace_bytes"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def peel_sweep_eps_workspace_bytes(self, p, T, adj16):
        return 0

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device="cpu", adj16=False, ensemble="olmos"):
        assert self.state is None, "one sampler call per round"
        self.state = [trial0, ntrials, eps, None, (seed, tuple(doped), adj16, ensemble)]
        return torch.zeros((ntrials, 1, 1), dtype=torch.int16), None

    def channel_levels(self, p, seed, trial0, ntrials, es_desc, doped=(), device="cpu"):
        assert self.state[:2] == [trial0, ntrials] and self.state[4][:2] == (seed, tuple(doped))
        th = [E.erasure_threshold(e) for e in es_desc]
        assert all(a > b for a, b in zip(th, th[1:])) and 1 <= len(th) <= 64
        self.state[3] = list(es_desc)
        return torch.zeros((ntrials, p.n), dtype=torch.uint8)

    def peel_sweep_eps(self, p, d_adj, d_lev, npoints, total_size, lost_lo=0, lost_hi=None, want_lost=False):
        trial0, ntrials, eps, es, _ = self.state
        assert npoints == len(es) and d_adj.shape[0] == ntrials == d_lev.shape[0]
        self.rounds.append((trial0, ntrials, eps, es))
        self.state = None
        out = torch.zeros((npoints, ntrials, 8), dtype=torch.int32)
        for k, e in enumerate(es):
            for t in range(ntrials):
                out[k, t, :3] = torch.tensor(fake_lost(trial0 + t, e), dtype=torch.int32)
        return {"out": out, "lost": None}

    def accumulate_peel(self, d_out, d_run, max_fuckups=0):
        """scldpc_accumulate_peel_device: in trial order, the trial at which the fuckups reach max_fuckups is the last."""
        assert d_out.is_contiguous() and d_out.shape[1] == 8
        for row in d_out.tolist():
            if max_fuckups > 0 and int(d_run[1]) >= max_fuckups:
                break
            d_run[0] += 1
            d_run[1] += row[0] >= 1
            d_run[2] += row[0]
            d_run[3] += row[1] > 0
            d_run[4] += row[1]
            d_run[5] += row[2]
        return d_run


def same_tuples(a, b):
    return len(a) == len(b) and all(len(x) == 13 == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


def test_the_curve_simulator_over_a_fake_engine(monkeypatch):
    fake = FakeEngine(monkeypatch)
    twin = float(np.nextafter(0.46, 0.0))
    es = [0.44, 0.50, twin, 0.40, 0.46, 0.44, 0.48]                      # unsorted, a duplicate, two eps with one threshold
    args = (4, 8, 12, 32, True, False, True, False)
    geo = PD._Geometry(4, 8, 12, 32, True, True, [])
    got = PD.simulate_sc_ldpc_curve(es, *args, num_repeats=500, max_fuckups=30, doping_points=[], seed=9, batch=64, device="cpu")
    want = [reference_tuple(e, geo, 500, 30) for e in es]
    assert same_tuples(got, want)
    stops = [t[5] for t in want]
    assert len(set(stops)) >= 4 and stops[3] == 500 and stops[1] < 200    # the points stop at different trials; 0.40 runs out
    # one sampler call per round at max(es), the rounds of simulate_sc_ldpc (batch 64 from trial 0), descending live points
    assert [r[0] for r in fake.rounds] == list(range(0, 500, 64)) and all(r[2] == 0.50 for r in fake.rounds)
    assert fake.rounds[0][3] == [0.50, 0.48, twin, 0.44, 0.40] and fake.rounds[-1][1] == 500 - 448
    for (_, _, _, before), (t0, _, _, after) in zip(fake.rounds, fake.rounds[1:]):
        assert set(after) <= set(before)                                 # a point that left does not come back
        for e in before:                                                 # ... and leaves exactly when its run has stopped
            assert (e in after) == (reference_tuple(e, geo, 500, 30)[5] > t0)
    assert fake.rounds[-1][3] == [0.40]
    # every point stopped: the loop ends before num_repeats
    fake.rounds.clear()
    got = PD.simulate_sc_ldpc_curve([0.50, 0.48], *args, num_repeats=5000, max_fuckups=5, seed=9, batch=64, device="cpu")
    assert same_tuples(got, [reference_tuple(e, geo, 5000, 5) for e in (0.50, 0.48)]) and len(fake.rounds) <= 2
    assert PD.simulate_sc_ldpc_curve([], *args, device="cpu") == []
    # hard doping goes to both calls, soft doping to neither: its VNs are zeroed on the [T, n] view
    seen = []
    monkeypatch.setattr(E, "channel_levels", lambda p, seed, t0, T, es_desc, doped=(), device="cpu":
                        (seen.append(tuple(doped)), fake.channel_levels(p, seed, t0, T, es_desc, doped, device))[1])
    PD.simulate_sc_ldpc_curve([0.45], 4, 8, 13, 32, True, False, True, False, 64, 5, [3], seed=9, batch=64, device="cpu")
    PD.simulate_sc_ldpc_curve([0.45], 4, 8, 13, 32, True, False, True, False, 64, 5, {3: 0.5}, seed=9, batch=64, device="cpu")
    assert seen == [(3,), ()]


def test_the_curve_simulator_refuses_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("sample_philox", "channel_levels", "peel_sweep_eps", "accumulate_peel", "local_device", "_require_gpu"):
        monkeypatch.setattr(E, name, no_device)
    f = lambda es=ES, bounded=True, shape=(4, 8, 12, 32), **kw: PD.simulate_sc_ldpc_curve(es, *shape, True, False, bounded, False, 10, 5, **kw)
    with pytest.raises(ValueError, match=r"^eps_fused: rng='numpy' draws a fresh stream of codes and channels for every eps"):
        f(rng="numpy")
    with pytest.raises(ValueError, match=r"^eps_fused: an unbounded chain sweeps from CN position 10 \(sweep_start > 0\)"):
        f(bounded=False)
    for sw in ("small", "wide"):
        with pytest.raises(ValueError, match=r"^eps_fused: sweep='%s' chooses the 4-bit sweep decoder" % sw):
            f(sweep=sw)
    with pytest.raises(ValueError, match=r"^eps_fused: local_tables=True chooses the tables of the 4-bit sweep decoder"):
        f(local_tables=True)
    with pytest.raises(ValueError, match=r"^eps_fused: at most 64 distinct eps points in one run \(got 65\)"):
        f(es=list(np.linspace(0.3, 0.5, 65)))
    with pytest.raises(ValueError, match=r"^eps_fused: .*do not fit 160 KiB of LDS"):
        f(shape=(3, 6, 64, 1 << 15))
    with pytest.raises(NotImplementedError, match="protograph \\+ tail-biting"):
        PD.simulate_sc_ldpc_curve(ES, 4, 8, 12, 32, True, True, True, True, 10, 5)
    assert PD.EPS_FUSED_BY_DEFAULT is False


# ---- the command line ----------------------------------------------------------------------------------------------------
ARGV = ["4", "8", "12", "32", "[0.44, 0.5, 0.46]", "T", "U", "B", "NTB", "300", "20", "[]"]


def t13(e, reps):
    return (e, 0.25, 0.1, 0.05, 3, 12, 7, 3072, np.zeros(reps), np.zeros(reps), 2, 96, 2 / 96)


def test_eps_fused_on_the_command_line(monkeypatch, tmp_path):
    curve, single = [], []

    def fake_curve(es, l, r, L, M, term, proto, bounded, tb, reps, fu, doping, **kw):
        curve.append((list(es), (l, r, L, M, term, proto, bounded, tb, reps, fu, doping), kw))
        return [t13(e, reps) for e in es]

    def fake_single(e, l, r, L, M, term, proto, bounded, tb, reps, fu, doping, **kw):
        single.append((e, kw))
        return t13(e, reps)
    monkeypatch.setattr(PD, "simulate_sc_ldpc_curve", fake_curve)
    monkeypatch.setattr(PD, "simulate_sc_ldpc", fake_single)
    a, b, c, d = (str(tmp_path / n) for n in "abcd")
    PD.main_simulate_sc_ldpc([a] + ARGV + ["--rng", "philox", "--seed", "5", "--eps-fused", "on", "--batch", "64", "--device", "cpu"])
    assert curve == [([0.44, 0.5, 0.46], (4, 8, 12, 32, True, False, True, False, 300, 20, []),
                      dict(rng="philox", seed=5, batch=64, device="cpu"))] and not single
    PD.main_simulate_sc_ldpc([b] + ARGV + ["--rng", "philox", "--seed", "5", "--batch", "64", "--device", "cpu"])
    PD.main_simulate_sc_ldpc([c] + ARGV + ["--rng", "philox", "--seed", "5", "--eps-fused", "off", "--batch", "64", "--device", "cpu"])
    PD.main_simulate_sc_ldpc([d] + ARGV + ["--rng", "philox", "--seed", "5", "--eps-fused", "auto", "--batch", "64", "--device", "cpu"])
    assert len(curve) == 1 and [s[0] for s in single] == [0.44, 0.5, 0.46] * 3      # auto is off (EPS_FUSED_BY_DEFAULT)
    assert all(s[1] == dict(rng="philox", seed=5, batch=64, device="cpu") for s in single)     # the calls are what they were
    texts = [open(x).read() for x in (a, b, c, d)]
    assert texts[0] == texts[1] == texts[2] == texts[3] and len(texts[0].splitlines()) == 4
    assert texts[0].splitlines()[2].split()[:2] == ["0.5", "0.5"]
    # the options the fused path refuses reach the simulator, which names them
    PD.main_simulate_sc_ldpc([a] + ARGV + ["--rng", "philox", "--eps-fused", "on", "--sweep", "small", "--local-tables", "on", "--device", "cpu"])
    assert curve[-1][2] == dict(rng="philox", sweep="small", local_tables=True, device="cpu")
    PD.main_simulate_sc_ldpc([a] + ARGV + ["--eps-fused", "on", "--device", "cpu"])
    assert curve[-1][2] == dict(device="cpu")
    monkeypatch.undo()
    with pytest.raises(ValueError, match="^eps_fused: rng='numpy'"):
        PD.main_simulate_sc_ldpc([a] + ARGV + ["--eps-fused", "on", "--rng", "numpy", "--device", "cpu"])


def test_eps_fused_goes_where_it_belongs(monkeypatch, tmp_path):
    for name in ("simulate_sc_ldpc_spectrum", "simulate_sc_ldpc", "simulate_sc_ldpc_curve", "simulate_peeling_decoder_ldpc",
                 "simulate_pd_covariance"):
        monkeypatch.setattr(PD, name, lambda *a, **k: pytest.fail("ran"))
    out = str(tmp_path / "o.txt")
    with pytest.raises(SystemExit, match=r"--eps-fused takes on, off or auto \(got 'yes'\)"):
        PD.main_simulate_sc_ldpc([out] + ARGV + ["--eps-fused", "yes"])
    with pytest.raises(SystemExit, match="--eps-fused walks ber_sim's eps grid on one sampled code .*stopping_sets takes no such option "
                                         r"\(the spectrum pass reads the lost bits"):
        PD.main_stopping_sets([out] + ARGV + ["--eps-fused", "on", "--rng", "philox"])
    with pytest.raises(SystemExit, match="--eps-fused walks .*simulate_variance takes no such option"):
        PD.main_simulate_variance([out, "4", "8", "12", "32", "0.45", "T", "U", "10", "10", "x.npy", "--eps-fused", "on"])
    with pytest.raises(SystemExit, match="--eps-fused walks .*simulate_covariance takes no such option"):
        PD.main_simulate_covariance([out, "4", "8", "12", "32", "0.45", "T", "U", "10", "4", "--eps-fused", "off"])
    assert not os.path.exists(out)


# ---- the identity itself ----------------------------------------------------------------------------------------------------
def oracle_stages(l, r, L, M, terminated, sweep_pos, seed):
    """One code and one nested channel: [(direct residual, incremental residual) per point of ES]."""
    from oracle import pd_oracle as P
    rng = np.random.RandomState(seed)
    cpp = l * M // r
    D = L + l - 1
    cn = np.stack([i * cpp + rng.permutation(l * M).reshape(l, M) // r for i in range(D)])
    tr = np.empty((L, M, l), dtype=np.int64)
    for d in range(l):
        tr[:, :, d] = cn[d:d + L, d, :]
    tr = tr.reshape(L * M, l)
    u = rng.rand(L * M)
    total = cpp * (D if terminated else L)
    out, R = [], None
    for e in ES:
        Ek = u <= e
        direct = P.peel_closure(tr, Ek, total, sweep_pos * cpp)
        R = P.peel_closure(tr, Ek if R is None else (R & Ek), total, sweep_pos * cpp)
        out.append((direct, R))
    return out


@pytest.mark.parametrize("l,r,L,M,terminated", [(4, 8, 12, 32, True), (3, 6, 10, 40, False)], ids=["4-8-terminated", "3-6-open"])
def test_the_residual_of_a_lower_eps_is_the_residual_of_the_residual(l, r, L, M, terminated):
    """200 codes, six points each: R_k = residual(R_{k-1} ∩ E_k) with the sweep starting at CN 0, without an exception."""
    mismatches = fails_first = fails_last = 0
    for seed in range(200):
        st = oracle_stages(l, r, L, M, terminated, 0, seed)
        mismatches += sum(not np.array_equal(a, b) for a, b in st)
        fails_first += bool(st[0][0].any())
        fails_last += bool(st[-1][0].any())
    assert mismatches == 0
    if terminated:
        assert fails_first >= 100 and fails_last <= 50                   # the grid crosses the threshold: both branches are met
    else:
        assert fails_first == fails_last == 200                          # the truncated tail holds its VNs at every point


def test_with_a_sweep_start_above_zero_the_identity_is_false():
    """Why simulate_sc_ldpc_curve refuses unbounded chains: one pinned code of (4,8), L = 14, M = 32 with the sweep starting at
    position 3, where peeling on from the residual of the point before leaves another set than peeling the point itself."""
    st = oracle_stages(4, 8, 14, 32, True, 3, PINNED_SEED)
    assert any(not np.array_equal(a, b) for a, b in st)
    assert all(np.array_equal(a, b) for a, b in oracle_stages(4, 8, 14, 32, True, 0, PINNED_SEED))


PINNED_SEED = 0
