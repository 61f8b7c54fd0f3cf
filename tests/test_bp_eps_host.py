"""Unlimited full BP over an eps grid from one code, on the CPU: the symbols of the extension header include/scldpc_bp_eps.h,
every check its entries decide before any device work (placeholder pointers that are never dereferenced, as
tests/test_eps_host.py), the workspace query, bp_decoding.eps_fused_reason and the command line's exits, the host logic of
bp_decoding.run_grid_fused over an engine fake (one sampler call per round at the key of point 0, live points that only shrink,
the caller's order, every run against a trial-by-trial restatement of plr_computation + willIstop), and the identity the decoder
rests on, fixpoint(E_k) = fixpoint(R_{k-1} ∩ E_k), on the oracle's decodeBP."""
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
from test_eps_host import ES, QCAP, WORKSPACE_M

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_bp_eps.h")
BPE, BPE16 = "scldpc_full_bp_eps_device", "scldpc_full_bp_eps_device_adj16"


def err():
    return _lib.lib().scldpc_last_error().decode()


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_BP_EPS) and len(declared) == 3
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
              | set(_lib.EXPORTS_COV) | set(_lib.EXPORTS_SS) | set(_lib.EXPORTS_RUNS) | set(_lib.EXPORTS_EPS))
    assert not declared & others                                         # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc_eps.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_bp_eps.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    assert "_lib.EXPORTS_BP_EPS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_bp_eps.h"\nint main(void){'
                   'int (*g)(const scldpc_code_params *, int32_t, const int32_t *, const uint8_t *, int32_t, int32_t,'
                   ' int32_t *, uint32_t *, void *, uint64_t, void *) = scldpc_full_bp_eps_device;'
                   'int (*h)(const scldpc_code_params *, int32_t, const uint16_t *, const uint8_t *, int32_t, int32_t,'
                   ' int32_t *, uint32_t *, void *, uint64_t, void *) = scldpc_full_bp_eps_device_adj16;'
                   'int64_t (*w)(const scldpc_code_params *, int32_t, int32_t) = scldpc_full_bp_eps_workspace_query;'
                   'return (g==0)+(h==0)+(w==0)+SCLDPC_EPS_MAX_POINTS-64+SCLDPC_NCOUNTERS-8;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the checks decided before any device work ----------------------------------------------------------------------------
def entry_call(p=None, T=1, adj=ONE, lev=ONE, K=6, is_term=1, out=ONE, erased=None, ws=None, wsb=0, entry=BPE16):
    p = E.make_params(4, 8, 12, 32) if p is None else p
    rc = getattr(_lib.lib(), entry)(C.byref(p), T, adj, lev, K, is_term, out, erased, ws, wsb, None)
    return rc, err()


@pytest.mark.parametrize("entry", [BPE, BPE16])
def test_the_entries_refuse_with_a_text_and_no_device(entry):
    """peel_sweep_eps's order and wording: the parameters, null buffers, npoints, the empty batch, the limits, the LDS, the
    workspace.  Each call below is wrong in one thing only, except where the order itself is shown."""
    rc, msg = entry_call(p=E.CodeParams(3, 6, 10, 64, 127), entry=entry)
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = entry_call(p=E.CodeParams(3, 6, 10, 64, 127), T=-1, K=0, entry=entry)     # the parameters come first
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = entry_call(T=-1, entry=entry)
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for kw in (dict(adj=None), dict(lev=None), dict(out=None)):
        rc, msg = entry_call(entry=entry, **kw)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials", kw
    rc, msg = entry_call(out=None, K=0, entry=entry)                     # the buffers before npoints
    assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
    for K in (0, 65, -3):
        rc, msg = entry_call(K=K, entry=entry)
        assert rc == BAD_ARG and msg == "%s: 1 <= npoints <= 64 (got npoints = %d)" % (entry, K)
    rc, msg = entry_call(K=65, T=0, adj=None, lev=None, out=None, entry=entry)          # npoints before the empty batch
    assert rc == BAD_ARG and msg == "%s: 1 <= npoints <= 64 (got npoints = 65)" % entry
    for K in (1, 64):
        assert entry_call(K=K, T=0, adj=None, lev=None, out=None, entry=entry)[0] == OK  # an empty batch touches nothing
    assert entry_call(p=E.CodeParams(9, 18, 4, 8, 16), T=0, entry=entry)[0] == OK        # ... and is judged no further
    for is_term in (0, 1):
        rc, msg = entry_call(p=E.CodeParams(9, 18, 4, 8, 16), is_term=is_term, entry=entry)
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
    q = lambda p, T, a16: lib.scldpc_full_bp_eps_workspace_query(C.byref(p), T, a16)
    small, bench, big = E.make_params(4, 8, 12, 32), E.make_params(4, 8, 50, 1000), E.make_params(4, 8, 50, 5000)
    for T in (0, 1, 77):
        for a16 in (0, 1):
            assert q(small, T, a16) == 0 and q(bench, T, a16) == 0       # the words stay in LDS
            assert q(big, T, a16) == T * 4 * big.nk                      # 32-bit words in the workspace, one slice per trial
    assert E.full_bp_eps_workspace_bytes(big, 3, True) == 3 * 4 * 132500
    for pair in ((3, 6), (5, 10)):
        assert q(E.make_params(*pair, 50, 1000), 5, 1) == 0
    # int32 rows, (4,8), L = 50: the smallest N (multiples of 2) whose words leave the LDS — one step below peel_sweep_eps's
    # (two [L] position arrays where that kernel has one [L + dv]); the GPU tests use that entry's N, in the workspace here too
    m = next(M for M in range(1000, 3000, 2) if q(E.make_params(4, 8, 50, M), 1, 0))
    assert m == WORKSPACE_M - 2 and q(E.make_params(4, 8, 50, m - 2), 4, 0) == 0
    for M in (m, WORKSPACE_M):
        assert q(E.make_params(4, 8, 50, M), 4, 0) == 4 * 4 * E.make_params(4, 8, 50, M).nk
    assert q(E.CodeParams(3, 6, 10, 64, 127), 1, 0) == BAD_ARG and "must equal" in err()
    huge = E.make_params(3, 6, 64, 1 << 15)
    assert q(huge, 1, 0) == TOO_LARGE and "do not fit 160 KiB of LDS" in err()
    with pytest.raises(E.ScldpcError, match="LDS"):
        E.full_bp_eps_workspace_bytes(huge, 1, False)


def test_the_queue_cap_is_read_per_call_and_changes_no_answer(monkeypatch):
    p = E.make_params(4, 8, 12, 32)
    for v in ("8", "0", "-5", "100000"):
        monkeypatch.setenv(QCAP, v)
        assert _lib.lib().scldpc_full_bp_eps_workspace_query(C.byref(p), 3, 1) == 0
        assert entry_call(K=0)[0] == BAD_ARG


# ---- eps_fused_reason and the command line ----------------------------------------------------------------------------------
SMALL = E.make_params(4, 8, 12, 16)
GRID6 = [0.48 - 0.02 * k for k in range(6)]


def test_eps_fused_reason_one_case_per_refusal():
    ok = dict(schedule="fixpoint", max_it=1000000, caps=None, window="off", rng="philox", shard="auto")
    f = lambda prog="bp_lim_iter", p=SMALL, es=GRID6, **kw: BP.eps_fused_reason(prog, p, es, **dict(ok, **kw))
    assert f() is None and f(max_it=0) is None and f(max_it=2000000) is None and f(shard="frames") is None
    assert f(es=list(np.linspace(0.6, 0.2, 64))) is None
    assert f(p=E.make_params(4, 8, 50, 5000)) is None and f(p=E.make_params(3, 6, 10, 20)) is None
    for prog in ("sw_lim_iter", "bp_traj"):
        assert f(prog=prog).endswith("%s takes no such path" % prog)
    assert f(schedule="flooding").startswith("--schedule flooding counts flooding iterations")
    for cap in (1, 250, 999999):
        assert f(max_it=cap).startswith("MAX_IT = %d binds" % cap)
    assert f(caps=[100, 200]).startswith("--caps asks for capped results")
    assert f(window="classical", schedule="flooding").startswith("--schedule flooding")     # the stated order
    assert f(window="classical").startswith("--window classical decodes window by window")
    assert f(rng="glibc").startswith("--rng glibc replays one sequential random() stream")
    assert f(shard="points").startswith("--shard points gives every rank")
    assert f(es=list(np.linspace(0.6, 0.2, 65))) == "at most 64 distinct ε points in one run (got 65)"
    twin = float(np.nextafter(0.3, 0.0))                                 # 65 eps, 64 thresholds: fine
    assert E.erasure_threshold(twin) == E.erasure_threshold(0.3)
    assert f(es=list(np.linspace(0.6, 0.2, 63)) + [0.3, twin]) is None
    assert "do not fit 160 KiB of LDS" in f(p=E.make_params(3, 6, 64, 1 << 15))
    assert BP.BP_EPS_FUSED_BY_DEFAULT is False


FUSED_ARGV = ["0", "0", "0", "1000000", "--schedule", "fixpoint", "--eps-fused", "on", "--N", "16", "--L", "12", "--num-points", "6",
              "--eps-delta", "0.02", "--seed", "5", "--quiet"]


def test_the_command_line_exits_before_any_device_work(monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("device work before the command line was checked")
    for name in ("sample_philox", "channel_levels", "full_bp_eps", "accumulate_run", "local_device", "_require_gpu",
                 "init_distributed", "new_run"):
        monkeypatch.setattr(E, name, no_device)
    monkeypatch.setattr(BP, "Simulator", no_device)
    out = ["--outdir", str(tmp_path / "o")]

    def refused(prog, argv, text):
        with pytest.raises(SystemExit) as e:
            BP.main(prog, argv + out)
        code = str(e.value.code)
        assert code.startswith("--eps-fused on: ") and text in code[:len("--eps-fused on: ") + 80], code
    base = FUSED_ARGV[4:]
    refused("sw_lim_iter", ["0", "5", "0", "1000000", "0", "--eps-fused", "on"], "the ε walk is unlimited full BP")
    refused("bp_traj", ["0", "0", "0", "1000000", "1", "--eps-fused", "on", "--schedule", "fixpoint"], "the ε walk is unlimited")
    refused("bp_lim_iter", ["0", "0", "0", "1000000", "--eps-fused", "on"], "--schedule flooding counts")
    refused("bp_lim_iter", ["0", "0", "0", "250"] + base, "MAX_IT = 250 binds")
    refused("bp_lim_iter", ["0", "0", "0", "0"] + base, "MAX_IT = 1 binds")             # MAX_IT = 0 runs one iteration (BPF:1065)
    refused("bp_lim_iter", FUSED_ARGV + ["--caps", "100,200"], "--caps asks for capped results")
    refused("bp_lim_iter", ["0", "4", "0", "1000000", "--eps-fused", "on", "--window", "classical"], "--schedule flooding counts")
    refused("bp_lim_iter", FUSED_ARGV + ["--rng", "glibc"], "--rng glibc replays")
    refused("bp_lim_iter", FUSED_ARGV + ["--shard", "points"], "--shard points gives every rank")
    refused("bp_lim_iter", FUSED_ARGV + ["--num-points", "65", "--eps-delta", "0.005"], "at most 64 distinct ε points in one run (got 65)")
    refused("bp_lim_iter", ["0", "0", "0", "1000000"] + base + ["--dv", "3", "--dc", "6", "--L", "64", "--N", "32768"],
            "scldpc_full_bp_eps_workspace_query: ")
    assert not os.path.exists(str(tmp_path / "o"))
    # --shard frames and auto pass the check: the run itself is the next thing that happens
    for shard in ([], ["--shard", "frames"], ["--shard", "auto"]):
        with pytest.raises(AssertionError, match="device work"):
            BP.main("bp_lim_iter", FUSED_ARGV + shard + out)
    assert "every point decodes the codes of point 0" in " ".join(BP._parser("bp_lim_iter").format_help().split())


def test_off_and_auto_take_the_unfused_program(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(BP, "run_grid_fused", lambda *a, **k: pytest.fail("the fused path ran"))
    monkeypatch.setattr(E, "init_distributed", lambda: False)

    class Sim:
        def __init__(self, p, **kw):
            seen.append(kw["schedule"])
            raise KeyboardInterrupt                                      # far enough: the unfused program builds its Simulator
    monkeypatch.setattr(BP, "Simulator", Sim)
    for mode in (["--eps-fused", "off"], ["--eps-fused", "auto"], []):
        argv = [a for a in FUSED_ARGV if a not in ("--eps-fused", "on")] + mode + ["--outdir", str(tmp_path)]
        with pytest.raises(KeyboardInterrupt):
            BP.main("bp_lim_iter", argv)
    assert seen == ["fixpoint"] * 3


# ---- the host logic of run_grid_fused over an engine fake ---------------------------------------------------------------------
def fake_row(frame, e):
    """A frame's counters at eps e: it fails where a hash of the frame falls below a share that grows with e (so the failing
    frames of a lower eps are among those of a higher one, as on one code)."""
    h = (frame * 2654435761 + 12345) % 1000
    if h >= int(2500 * (e - 0.38)):
        return [0, 0, 0, 0, 0, 2, 0, 40 + frame % 7]
    exp = frame % 3
    return [5 + frame % 4, 1 + frame % 2, exp, int(exp > 0), 0, 3, 0, 40 + frame % 7]


def reference_run(e, min_frame_err, max_frames):
    """plr_computation (BPF:1506-1519) and willIstop (BPF:2143-2144), frame by frame."""
    r = dict.fromkeys(BP.RUN_NAMES, 0)
    for frame in range(max_frames):
        c = fake_row(frame, e)
        if c[0] > 0:
            r["users_err"] += c[0]
            r["frame_err"] += 1
            r["block_err"] += c[1]
        if c[2] > 0:
            r["users_err_exp"] += c[2]
            r["frame_err_exp"] += 1
            r["block_err_exp"] += c[3]
        r["frames"] += 1
        r["iterations"] += c[5]
        if r["frame_err"] >= min_frame_err > 0:
            break
    return r


class FakeEngine:
    """Stands in for the engine calls of run_grid_fused on CPU tensors and records them."""

    def __init__(self, monkeypatch, index, seed):
        self.rounds, self.state, self.index, self.seed = [], None, index, seed
        for name in ("sample_philox", "channel_levels", "full_bp_eps", "accumulate_run", "full_bp_eps_workspace_bytes", "chain_runs"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def full_bp_eps_workspace_bytes(self, p, T, adj16):
        return 0

    def chain_runs(self, *a, **k):
        raise AssertionError("no runs were asked for")

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device="cpu", out=None, adj16=False, ensemble="olmos"):
        assert self.state is None, "one sampler call per round"
        assert seed == self.seed and out is not None and out[0].dtype == torch.int16 and out[0].shape == (ntrials, p.n, p.dv)
        frame0 = trial0 - BP.trial_key(self.index, 0, 0)
        assert 0 <= frame0 < BP.POINT_STRIDE and trial0 == BP.trial_key(self.index, 0, frame0)     # the key of point 0
        self.state = [frame0, ntrials, eps, None, tuple(doped)]
        return out

    def channel_levels(self, p, seed, trial0, ntrials, es_desc, doped=(), device="cpu", out=None):
        assert trial0 == BP.trial_key(self.index, 0, self.state[0]) and ntrials == self.state[1] and tuple(doped) == self.state[4]
        th = [E.erasure_threshold(e) for e in es_desc]
        assert all(a > b for a, b in zip(th, th[1:])) and 1 <= len(th) <= 64
        self.state[3] = list(es_desc)
        return out

    def full_bp_eps(self, p, d_adj, d_lev, npoints, is_term=True, want_erased=False, counters=None):
        frame0, ntrials, eps, es, _ = self.state
        assert npoints == len(es) and d_adj.shape[0] == ntrials == d_lev.shape[0] and not want_erased and is_term
        assert counters.shape == (npoints, ntrials, 8) and counters.is_contiguous()
        self.rounds.append((frame0, ntrials, eps, es))
        self.state = None
        for k, e in enumerate(es):
            for t in range(ntrials):
                counters[k, t] = torch.tensor(fake_row(frame0 + t, e), dtype=torch.int32)
        return {"counters": counters, "erased": None}

    def accumulate_run(self, d_counters, d_run, stop_frame_err=0):
        """scldpc_accumulate_run_device: in frame order, the frame at which frame_err reaches stop_frame_err is the last."""
        assert d_counters.is_contiguous() and d_counters.shape[1] == 8 and d_run.shape == (9,)
        for c in d_counters.tolist():
            if stop_frame_err > 0 and int(d_run[1]) >= stop_frame_err:
                break
            if c[0] > 0:
                d_run[0] += c[0]; d_run[1] += 1; d_run[3] += c[1]
            if c[2] > 0:
                d_run[4] += c[2]; d_run[5] += 1; d_run[6] += c[3]
            d_run[2] += c[4] > 0
            d_run[7] += 1
            d_run[8] += c[5]
        return d_run


def test_the_grid_over_a_fake_engine(monkeypatch):
    fake = FakeEngine(monkeypatch, index=3, seed=9)
    twin = float(np.nextafter(0.46, 0.0))
    es = [0.44, 0.50, twin, 0.40, 0.46, 0.44, 0.48]                      # unsorted, a duplicate, two eps with one threshold
    p = E.make_params(4, 8, 12, 16)
    pts = BP.run_grid_fused(p, es, 30, 500, seed=9, index=3, batch=64, device="cpu")
    assert [pt.eps for pt in pts] == es and all((pt.n, pt.L) == (p.n, 12) and not pt.bad and pt.runs is None for pt in pts)
    want = [reference_run(e, 30, 500) for e in es]
    assert [pt.run for pt in pts] == want
    stops = [r["frames"] for r in want]
    print("stop frames by point:", stops)
    assert len(set(stops)) >= 4 and stops[3] == 500 and want[3]["frame_err"] < 30 and stops[1] < 200   # 0.40 runs out of frames
    # one sampler call per round at max(es) with the key of point 0, the rounds of run_point (batch 64 from frame 0)
    assert [r[0] for r in fake.rounds] == list(range(0, 500, 64)) and all(r[2] == 0.50 for r in fake.rounds)
    assert fake.rounds[0][3] == [0.50, 0.48, twin, 0.44, 0.40] and fake.rounds[-1][1] == 500 - 448
    for (_, _, _, before), (f0, _, _, after) in zip(fake.rounds, fake.rounds[1:]):
        assert set(after) <= set(before)                                 # a point that left does not come back
        for e in before:                                                 # ... and leaves exactly when its run has stopped
            assert (e in after) == (reference_run(e, 30, 500)["frames"] > f0)
    assert fake.rounds[-1][3] == [0.40]
    # every point stopped: the loop ends long before max_frames
    fake.rounds.clear()
    pts = BP.run_grid_fused(p, [0.50, 0.48], 5, 5000, seed=9, index=3, batch=64, device="cpu")
    assert [pt.run for pt in pts] == [reference_run(e, 5, 5000) for e in (0.50, 0.48)] and len(fake.rounds) <= 2
    # no stop rule: every point takes every frame, and nobody reads the counters back in between
    fake.rounds.clear()
    pts = BP.run_grid_fused(p, [0.46, 0.50], 0, 130, seed=9, index=3, batch=64, device="cpu")
    assert [pt.run for pt in pts] == [reference_run(e, 0, 130) for e in (0.46, 0.50)]
    assert [r[:2] for r in fake.rounds] == [(0, 64), (64, 64), (128, 2)]
    assert BP.run_grid_fused(p, [], 30, 500, seed=9, device="cpu") == []
    with pytest.raises(ValueError, match=r"^eps_fused: at most 64 distinct ε points in one run \(got 65\)"):
        BP.run_grid_fused(p, list(np.linspace(0.3, 0.5, 65)), 30, 500, seed=9, device="cpu")


def test_a_broken_invariant_aborts_as_run_point_does(monkeypatch, capsys):
    fake = FakeEngine(monkeypatch, index=0, seed=1)
    real = fake.full_bp_eps

    def broken(p, d_adj, d_lev, npoints, **kw):
        res = real(p, d_adj, d_lev, npoints, **kw)
        res["counters"][1, 5, 6] = 1                                     # status != 0 in frame 5 of the second point
        return res
    monkeypatch.setattr(E, "full_bp_eps", broken)
    p = E.make_params(4, 8, 12, 16)
    pts = BP.run_grid_fused(p, [0.50, 0.48, 0.46], 0, 64, seed=1, batch=64, device="cpu", defer_abort=True)
    assert [pt.bad for pt in pts] == [False, True, False]
    with pytest.raises(SystemExit) as e:
        BP.run_grid_fused(p, [0.50, 0.48, 0.46], 0, 64, seed=1, batch=64, device="cpu")
    assert e.value.code == -1 and "ARGH! RECOVERED MORE VNs THAN deg-1 CNs!" in capsys.readouterr().out


# ---- the identity itself ----------------------------------------------------------------------------------------------------
def numpy_code(l, r, L, N, rng):
    """One code of the Olmos chain, numpy-sampled: VN -> CN table int32 [L * N, l] (as tests/test_eps_host.oracle_stages)."""
    cpp = l * N // r
    D = L + l - 1
    cn = np.stack([i * cpp + rng.permutation(l * N).reshape(l, N) // r for i in range(D)])
    tr = np.empty((L, N, l), dtype=np.int64)
    for d in range(l):
        tr[:, :, d] = cn[d:d + L, d, :]
    return tr.reshape(L * N, l).astype(np.int32)


FOUR = ("num_erasures", "num_blocks_err", "num_erasures_exp", "num_blocks_err_exp")


@pytest.mark.parametrize("l,r,L,N,is_term", [(4, 8, 12, 16, 1), (3, 6, 10, 20, 1), (3, 6, 10, 20, 0)],
                         ids=["4-8-terminated", "3-6-terminated", "3-6-truncated"])
def test_the_fixpoint_of_a_lower_eps_is_the_fixpoint_of_the_residual(l, r, L, N, is_term):
    """100 codes, six nested channels each: decodeBP on R_{k-1} ∩ E_k leaves the erased set and the four counters decodeBP leaves
    on E_k — BPF's expurgation included, which reads the residual's graph alone."""
    from oracle import oracle as O
    po = O.Params(l, r, L, l * N // r, N)
    fails = np.zeros(len(ES), dtype=int)
    size2_only = several_blocks = 0
    for seed in range(100):
        rng = np.random.RandomState(seed)
        g = O.Graph.from_vn_adj(po, numpy_code(l, r, L, N, rng))
        u = rng.rand(L * N)
        R = None
        for k, e in enumerate(ES):
            Ek = (u <= e).astype(np.uint8)
            direct, erased, _ = O.decode_bp(g, Ek, is_term=is_term, literal=False)
            walk, R, _ = O.decode_bp(g, Ek if R is None else (R & Ek), is_term=is_term, literal=False)
            assert np.array_equal(erased, R), (seed, k)
            assert [walk[c] for c in FOUR] == [direct[c] for c in FOUR], (seed, k, walk, direct)
            assert direct["num_erasures"] == int(erased.sum()) and direct["status"] == 0
            fails[k] += direct["num_erasures"] > 0
            size2_only += direct["num_erasures"] > 0 and direct["num_erasures_exp"] == 0
            several_blocks += direct["num_blocks_err"] >= 2
    print("failing codes per point:", fails.tolist(), "size-2-only residuals:", size2_only, "with >= 2 blocks:", several_blocks)
    assert several_blocks >= 1                                           # the first-position rule is met
    if is_term:
        assert size2_only >= 1                                           # ... and residuals the expurgation removes whole
        assert fails[0] >= 50 and fails[-1] <= 50                        # the grid crosses the threshold
    else:
        assert fails.min() >= 90                                         # the truncated tail holds VNs at every point, nearly always
