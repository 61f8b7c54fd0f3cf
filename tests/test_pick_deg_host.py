"""Random-pick peeling for the pairs (3,6), (4,8), (5,10) (scldpc_peel_pick_device_adj16_deg: cn_build.hip's ring of dv CN
positions + peel_pick_multi_kernel) on the CPU: its three symbols, the shape rule behind scldpc_peel_pick_deg_supported
recomputed from the documented formula, the workspace formula, the refusals decided before any device work (placeholder
pointers that are never dereferenced, as tests/test_sweep_wide_host.py), the pure selector of simulate_peeling_decoder_ldpc, the
command line, and simulate_peeling_decoder_ldpc's calls with stand-ins for the engine."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ENTRY = "scldpc_peel_pick_device_adj16_deg"
NAMES = ("scldpc_peel_pick_deg_supported", "scldpc_peel_pick_deg_workspace_bytes", ENTRY)
ONE = C.c_void_p(16)                                                    # non-null placeholder (not 256-byte aligned)
ALIGNED = C.c_void_p(256)
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024


def last_error():
    return _lib.lib().scldpc_last_error().decode()


def test_the_three_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint(64_t)? %s\(" % name, header)
    assert L.scldpc_abi_version() == 2                                   # additions only
    assert L.scldpc_peel_pick_deg_workspace_bytes.restype is C.c_int64
    assert len(L.scldpc_peel_pick_device_adj16_deg.argtypes) == 13       # no MT state, no moments
    assert hasattr(E, "peel_pick_deg") and hasattr(E, "peel_pick_deg_supported")


def rule(p, total_size):
    """The documented rule, limit by limit in its order; None, or the name of the first limit that refuses."""
    if (p.dv, p.dc) not in ((3, 6), (4, 8), (5, 10)):
        return "pairs"
    if p.cns_pos > 65536:
        return "cns_pos"
    if not 0 <= total_size <= p.nk:
        return "total_size"
    if (total_size + 63) // 64 + 1 > 4096:
        return "bitmap"
    if p.dc * p.n >= 1 << 24:
        return "dc * n"
    magic = (1 << 32) // p.vns_pos + 1
    if any((x * magic) >> 32 != x // p.vns_pos for q in range(p.L + 1) for x in (q * p.vns_pos, max(q * p.vns_pos - 1, 0))):
        return "reciprocal"
    if p.dv * 4 * p.cns_pos > LDS:
        return "LDS"
    return None


TEXT = {"pairs": "the pairs (3,6), (4,8), (5,10) only: no instance for dv = 4, dc = 6", "total_size": "outside [0,",
        "bitmap": "the degree-1 bitmap takes 4220 words, at most 4096", "LDS": "LDS: the ring of 5 CN positions takes 200000 B",
        "dc * n": "needs dc * n < 2^24", "cns_pos": "exceeds 65536"}


@pytest.mark.parametrize("p,total_size,why", [
    (E.make_params(3, 6, 50, 10000), 250000, None), (E.make_params(3, 6, 50, 10000), 260000, None),
    (E.make_params(5, 10, 50, 10000), 250000, None), (E.make_params(5, 10, 50, 10000), 270000, "bitmap"),
    (E.make_params(4, 8, 50, 10000), 250000, None), (P(4, 6, 50, 800, 1200), 1000, "pairs"),
    (E.make_params(5, 10, 10, 20000), 0, "LDS"), (E.make_params(5, 10, 10, 16384), 0, None),
    (E.make_params(3, 6, 50, 10000), 260001, "total_size"), (E.make_params(3, 6, 50, 10000), -1, "total_size"),
    (E.make_params(3, 6, 1, 50), 75, None), (E.make_params(3, 6, 1, 50), 25, None), (E.make_params(5, 10, 3, 50), 0, None),
    (E.make_params(4, 8, 200, 10500), 100000, "dc * n"), (P(3, 6, 1, 70000, 140000), 0, "cns_pos"),
], ids=lambda v: "-".join(map(str, v.key())) if isinstance(v, P) else str(v))
def test_supported_follows_the_documented_rule(p, total_size, why):
    assert rule(p, total_size) == why
    assert E.peel_pick_deg_supported(p, total_size) is (why is None)
    if why is not None:
        assert last_error().startswith(ENTRY + ": ") and TEXT[why] in last_error(), last_error()
    # the entry refuses the same shapes with the same text, even for an empty batch, before it looks at any buffer
    if why is not None:
        said = last_error()
        for ntrials in (0, 1):
            rc = _lib.lib().scldpc_peel_pick_device_adj16_deg(C.byref(p), ntrials, None, None, total_size, 10, 0, 0, None, None, None, 0, None)
            assert rc == TOO_LARGE and last_error() == said
        assert _lib.lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), 8, total_size) == TOO_LARGE


def test_invalid_parameters_are_refused_first():
    bad = P(3, 6, 50, 500, 999)
    assert E.peel_pick_deg_supported(bad, 0) is False and "must equal" in last_error()
    assert _lib.lib().scldpc_peel_pick_device_adj16_deg(C.byref(bad), 0, None, None, 0, 0, 0, 0, None, None, None, 0, None) == BAD_ARG
    assert _lib.lib().scldpc_peel_pick_device_adj16_deg(None, 0, None, None, 0, 0, 0, 0, None, None, None, 0, None) == BAD_ARG


@pytest.mark.parametrize("shape,total_size,T", [((3, 6, 50, 10000), 250000, 8), ((5, 10, 50, 10000), 250000, 4096),
                                                ((3, 6, 1, 50), 75, 5), ((5, 10, 3, 50), 75, 1), ((4, 8, 7, 30), 0, 3),
                                                ((3, 6, 50, 10000), 260000, 0)])
def test_workspace_bytes_equals_the_formula(shape, total_size, T):
    p = E.make_params(*shape)
    want = ((T * p.nk * 4 + 255) & ~255) + T * ((total_size + 63) // 64 + 1) * 8
    assert _lib.lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), T, total_size) == want
    assert _lib.lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), -1, total_size) == BAD_ARG


def call(p, ntrials=1, a=ONE, ch=ONE, out=ONE, r1=None, total=None, steps=10, ws=ALIGNED, wsb=None):
    total = p.nk if total is None else total
    if wsb is None:
        wsb = max(_lib.lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), max(ntrials, 0), total), 0)
    rc = _lib.lib().scldpc_peel_pick_device_adj16_deg(C.byref(p), ntrials, a, ch, total, steps, 7, 0, r1, out, ws, wsb, None)
    return rc, last_error()


def test_argument_checks_before_any_device_work():
    p = E.make_params(3, 6, 7, 86)
    need = _lib.lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), 1, p.nk)
    assert call(p, ntrials=0, a=None, ch=None, out=None, ws=None, wsb=0)[0] == OK        # the empty batch
    for kw in (dict(ntrials=-1), dict(steps=-1), dict(ntrials=0, steps=-1)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": negative ntrials or num_steps", kw
    for kw in (dict(a=None), dict(ch=None), dict(out=None)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer", kw
    for kw, passed in ((dict(wsb=need - 1), need - 1), (dict(ws=None), 0), (dict(wsb=0), 0)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + (": needs %d bytes of device workspace (scldpc_peel_pick_deg_workspace_bytes), "
                                                 "the caller passed %d" % (need, passed)), (kw, msg)
    rc, msg = call(p, ws=ONE)
    assert rc == BAD_ARG and msg == ENTRY + ": the workspace must be 256-byte aligned"
    # the shape before the buffers, the parameters before the shape
    rc, msg = call(E.make_params(5, 10, 50, 10000), a=None, ws=None, wsb=0)
    assert rc == TOO_LARGE and "4220 words" in msg


def test_the_existing_workspace_answers_are_unchanged():
    ws = _lib.lib().scldpc_workspace_bytes
    p48, p36 = E.make_params(4, 8, 50, 10000), E.make_params(3, 6, 50, 10000)
    assert ws(E.WS_PEEL_PICK, C.byref(p48), 8, 250000, 0) == 8 * 265000 * 4 + 8 * 3908 * 8 == 8730112
    assert ws(E.WS_PEEL_PICK, C.byref(p36), 8, 250000, 0) == 8 * 260000 * 4 + 8 * 3908 * 8 == 8570112
    assert ws(E.WS_PEEL_PICK, C.byref(E.make_params(3, 6, 10, 20)), 8, 100, 0) == 0       # within the LDS: no workspace
    assert ws(5, C.byref(p36), 8, 250000, 0) == BAD_ARG                                   # no new operation
    # at these sizes the existing entry keeps words and bitmap in the workspace too: the function of its own says the same
    for p in (p48, p36):
        assert _lib.lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), 8, 250000) == ws(E.WS_PEEL_PICK, C.byref(p), 8, 250000, 0)


# ---- the selector ------------------------------------------------------------------------------------------------------
RNG_TEXT = "rng='numpy' replays the MT19937 stream, which is sequential: the multi-trial pick kernel draws from Philox"
PROTO_TEXT = "the protograph tables hold global CN ids in 4-byte rows: the multi-trial pick kernel reads position-local 2-byte rows"
KERNEL_TEXT = "moments_from='kernel': the multi-trial pick kernel has no in-chain moments (use 'rows')"
SHAPE_TEXT = ("the multi-trial pick kernel takes the pairs (3,6), (4,8), (5,10) with cns_pos <= 65536, at most 4096 words of degree-1 "
              "bitmap and a ring of dv CN positions within the LDS (dv = 5, dc = 10, L = 50, M = 10000, total_size = 270000)")


def expected(rng, ens, mf, ok, pick, default):
    if pick == "first":
        return "first", "pick='first'"
    if pick == "auto" and not default:
        return "first", "pick='auto' is 'first' (PICK_DEG_BY_DEFAULT)"
    if rng != "philox":
        return "first", RNG_TEXT
    if ens == "protograph":
        return "first", PROTO_TEXT
    if mf == "kernel":
        return "first", KERNEL_TEXT
    if not ok:
        return "first", SHAPE_TEXT
    return "multi", "cn_build ring + peel_pick_multi"


def test_select_pick_over_its_whole_grid(monkeypatch):
    assert PD.PICK_DEG_BY_DEFAULT is False
    p = E.make_params(5, 10, 50, 10000)
    for default in (False, True):
        monkeypatch.setattr(PD, "PICK_DEG_BY_DEFAULT", default)
        for rng in ("philox", "numpy"):
            for ens in ("olmos", "protograph"):
                for mf in ("auto", "rows", "kernel"):
                    for ok in (True, False):
                        for pick in ("auto", "first", "multi"):
                            got = PD.select_pick(p, 270000, rng, ens, mf, ok, pick)
                            assert got == expected(rng, ens, mf, ok, pick, default), (default, rng, ens, mf, ok, pick)
                        assert PD.select_pick(p, 270000, rng, ens, mf, ok) == PD.select_pick(p, 270000, rng, ens, mf, ok, "auto")
    with pytest.raises(ValueError, match="^pick must be 'auto', 'first' or 'multi'$"):
        PD.select_pick(p, 0, "philox", "olmos", "rows", True, "fast")


# ---- the command line --------------------------------------------------------------------------------------------------
def test_cli_parses_pick():
    pos, kw = PD._cli_options([None, "out.pkl", "3", "--pick", "multi", "6", "--rng", "philox"], {})
    assert pos == [None, "out.pkl", "3", "6"] and kw == {"pick": "multi", "rng": "philox"}
    for v in ("first", "multi", "auto"):
        assert PD._cli_options([None, "--pick", v], {})[1] == {"pick": v}
    with pytest.raises(SystemExit, match="--pick takes first, multi or auto"):
        PD._cli_options([None, "--pick", "fast"], {})


def test_ber_sim_takes_no_pick(tmp_path):
    with pytest.raises(SystemExit, match="ber_sim"):
        PD.main_simulate_sc_ldpc([str(tmp_path / "o.dat"), "4", "8", "10", "20", "[0.5]", "T", "U", "B", "NTB", "6", "2000", "[]",
                                  "--pick", "multi"])
    assert not (tmp_path / "o.dat").exists()


def test_simulate_variance_passes_pick_on(monkeypatch, tmp_path):
    seen = []

    def fake(e, l, r, L, M, term, proto, num, **kw):
        seen.append(kw)
        return None, np.zeros((3, 5), dtype=np.int64), np.zeros(num)

    monkeypatch.setattr(PD, "simulate_peeling_decoder_ldpc", fake)
    monkeypatch.setattr(PD, "load_theory", lambda path: np.ones(5))
    monkeypatch.setattr(PD, "nu_chunk_from_moments", lambda mom, th, M: (np.zeros(5), np.zeros(5)))
    monkeypatch.setattr(PD, "_join_job", lambda kw: False)
    PD.main_simulate_variance([str(tmp_path / "o.pkl"), "3", "6", "10", "20", "0.4", "T", "U", "4", "2", "none.npy", "--rng", "philox",
                               "--pick", "multi"])
    assert len(seen) == 2 and all(kw["pick"] == "multi" and kw["want_moments"] for kw in seen)


# ---- simulate_peeling_decoder_ldpc's calls, with stand-ins for the engine ----------------------------------------------
class Recorder:
    """Stand-ins for the engine calls of simulate_peeling_decoder_ldpc: they record their arguments and hand back CPU tensors."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("sample_philox", "peel_pick", "peel_pick_deg", "peel_pick_deg_supported", "r1_moments"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None, adj16=False, ensemble="olmos"):
        self.calls.append(("sample_philox", trial0, ntrials, tuple(doped), adj16, ensemble))
        return (torch.zeros((ntrials, p.n, p.dv), dtype=torch.int16 if adj16 else torch.int32),
                torch.zeros((ntrials, p.nw), dtype=torch.int32))

    def _res(self, T, steps, trial0, want_r1):
        out = torch.zeros((T, 4), dtype=torch.int32)
        out[:, 0] = 7 + torch.arange(T, dtype=torch.int32) + trial0
        r1 = (torch.arange(T, dtype=torch.int32)[:, None] + trial0 + 1).repeat(1, steps + 1) if want_r1 else None
        return {"out": out, "r1": r1, "moments": None}

    def peel_pick(self, p, d_adj, d_chan, total_size, num_steps, mt_state=None, seed=0, trial0=0, want_r1=True, moments=None):
        self.calls.append(("peel_pick", d_adj.shape[0], total_size, num_steps, seed, trial0, want_r1, moments is not None))
        return self._res(d_adj.shape[0], num_steps, trial0, want_r1)

    def peel_pick_deg(self, p, d_adj, d_chan, total_size, num_steps, seed=0, trial0=0, want_r1=True):
        assert d_adj.dtype == torch.int16
        self.calls.append(("peel_pick_deg", d_adj.shape[0], total_size, num_steps, seed, trial0, want_r1))
        return self._res(d_adj.shape[0], num_steps, trial0, want_r1)

    def peel_pick_deg_supported(self, p, total_size):
        self.calls.append(("peel_pick_deg_supported", p.key(), total_size))
        return _lib.lib().scldpc_peel_pick_deg_supported(C.byref(p), total_size) == 1

    def r1_moments(self, d_r1, moments=None):
        self.calls.append(("r1_moments", d_r1.shape[0]))
        r = d_r1.to(torch.int64)
        moments += torch.stack([(r != 0).sum(0), r.sum(0), (r * r).sum(0)])
        return moments


GEO = dict(L=7, M=86, e=0.42)
TS, STEPS = 7 * 43, int(86 * 7 * (0.42 + 0.1))                            # non-terminated (3,6): 43 CNs per position


def run(pick, **kw):
    return PD.simulate_peeling_decoder_ldpc(GEO["e"], 3, 6, GEO["L"], GEO["M"], False, False, 10, [3], rng="philox", seed=9, batch=4,
                                            device="cpu", pick=pick, **kw)


def test_pick_multi_calls_peel_pick_deg_with_the_right_trial0_per_batch(monkeypatch, capfd):
    rec = Recorder(monkeypatch)
    _, r1, plrs = run("multi")
    p = E.make_params(3, 6, 7, 86)
    assert rec.calls == [("peel_pick_deg_supported", p.key(), TS)] + [
        c for t0, nb in ((0, 4), (4, 4), (8, 2)) for c in (("sample_philox", t0, nb, (3,), True, "olmos"),
                                                           ("peel_pick_deg", nb, TS, STEPS, 9, t0, True))]
    assert (r1[:, 0] == np.arange(10) + 1).all() and (plrs == (np.arange(10) + 7) / (6 * 86)).all()
    err = capfd.readouterr().err
    assert err.count("[scldpc] kernels: ") == 1 and "cn_build ring + peel_pick_multi" in err
    # the moments come from the rows: "auto" resolves to "rows"
    rec = Recorder(monkeypatch)
    _, mom, plrs2 = run("multi", want_moments=True)
    assert [c[0] for c in rec.calls] == ["peel_pick_deg_supported"] + ["sample_philox", "peel_pick_deg", "r1_moments"] * 3
    assert all(c[-1] is True for c in rec.calls if c[0] == "peel_pick_deg")
    assert (mom[1] == (np.arange(10) + 1).sum()).all() and (plrs2 == plrs).all()


def test_pick_multi_on_a_rank_share_uses_global_trial_indices(monkeypatch, capfd):
    rec = Recorder(monkeypatch)
    fake_dist = types.SimpleNamespace(all_reduce=lambda t: t)
    monkeypatch.setattr(PD, "_dist", lambda: (fake_dist, 1, 2))            # rank 1 of 2: trials 5 .. 9
    _, r1, plrs = run("multi")
    assert [c for c in rec.calls if c[0] == "peel_pick_deg"] == [("peel_pick_deg", 4, TS, STEPS, 9, 5, True),
                                                                 ("peel_pick_deg", 1, TS, STEPS, 9, 9, True)]
    assert (r1[:5] == 0).all() and (r1[5:, 0] == np.arange(5, 10) + 1).all()


def test_pick_auto_and_first_call_nothing_new(monkeypatch, capfd):
    for kw in (dict(), dict(pick="auto"), dict(pick="first")):
        rec = Recorder(monkeypatch)
        PD.simulate_peeling_decoder_ldpc(GEO["e"], 3, 6, GEO["L"], GEO["M"], False, False, 10, [3], rng="philox", seed=9, batch=4,
                                         device="cpu", **kw)
        assert rec.calls == [c for t0, nb in ((0, 4), (4, 4), (8, 2)) for c in (("sample_philox", t0, nb, (3,), True, "olmos"),
                                                                                ("peel_pick", nb, TS, STEPS, 9, t0, True, False))], kw
        err = capfd.readouterr().err
        assert ("[scldpc] kernels: sampler (first generation) + peel_pick: pick='first'" in err) == (kw.get("pick") == "first")
        assert "peel_pick_multi" not in err


def test_pick_multi_raises_where_the_selector_refuses(monkeypatch):
    rec = Recorder(monkeypatch)
    base = dict(num_repeats=2, device="cpu", pick="multi")
    with pytest.raises(ValueError, match="^pick='multi': rng='numpy' replays the MT19937 stream"):
        PD.simulate_peeling_decoder_ldpc(0.4, 3, 6, 7, 86, True, False, rng="numpy", **base)
    with pytest.raises(ValueError, match="^pick='multi': the protograph tables hold global CN ids"):
        PD.simulate_peeling_decoder_ldpc(0.4, 3, 6, 7, 86, True, True, rng="philox", **base)
    with pytest.raises(ValueError, match="^pick='multi': moments_from='kernel'"):
        PD.simulate_peeling_decoder_ldpc(0.4, 3, 6, 7, 86, True, False, rng="philox", want_moments=True, moments_from="kernel", **base)
    with pytest.raises(ValueError, match=r"^pick='multi': the multi-trial pick kernel takes the pairs .* total_size = 270000\)$"):
        PD.simulate_peeling_decoder_ldpc(0.4, 5, 10, 50, 10000, True, False, rng="philox", **base)
    with pytest.raises(ValueError, match="^pick must be"):
        PD.simulate_peeling_decoder_ldpc(0.4, 3, 6, 7, 86, True, False, rng="philox", num_repeats=2, device="cpu", pick="fast")
    assert [c[0] for c in rec.calls if c[0] != "peel_pick_deg_supported"] == []       # refused before any engine work
