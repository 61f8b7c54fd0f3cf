"""The 4-bit sweep decoder (peel_sweep_small.hip) on the CPU: its two symbols, the shape rule behind
scldpc_peel_sweep_sock16_supported, the refusals decided before any device work (placeholder pointers that are never
dereferenced, as tests/test_deg_host.py), the pure selector of simulate_sc_ldpc, the command line, and simulate_sc_ldpc's calls
with stand-ins for the engine.

One refusal of the entry point has no case here because no valid shape reaches it: "the bitmap of sweep_start CNs leaves no
room for the queues" — with 16-bit sockets and at most 65536 CNs the counts (32 KiB), the VN bits (16 KiB) and the bitmap
(8 KiB) always leave a queue in one CU's 160 KiB."""
import ctypes as C
import os
import re

import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ENTRY = "scldpc_peel_sweep_device_sock16"
ONE = C.c_void_p(16)                                                    # non-null placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    for name in ("scldpc_peel_sweep_sock16_supported", ENTRY):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert L.scldpc_abi_version() == 2                                   # additions only


@pytest.mark.parametrize("p,want", [
    (E.make_params(4, 8, 50, 1000), True),
    (E.make_params(3, 6, 10, 40), True),
    (E.make_params(5, 10, 12, 40), True),
    (E.make_params(4, 8, 100, 1000), True),                             # 51 500 CNs
    (E.make_params(4, 8, 90, 1000), True),                              # the non-terminated, unbounded chain of L = 50
    (E.make_params(4, 8, 50, 5000), False),                             # 132 500 CNs
    (P(4, 6, 50, 800, 1200), False),                                    # no instance for (4,6)
    (P(3, 6, 2, 10923, 21846), False),                                  # 65 538 sockets per position
    (P(3, 6, 50, 500, 999), False),                                     # invalid parameters
], ids=lambda v: "-".join(map(str, v.key())) if isinstance(v, P) else str(v))
def test_supported_follows_the_shape_rule(p, want):
    assert E.peel_sweep_sock16_supported(p) == want
    assert E.peel_sweep_sock16_supported(p) == E.full_bp_deg_supported(p)       # the shapes of the _deg forms
    if p.key() == (4, 8, 50, 2500, 5000):
        assert p.nk == 132500


def call(p, ntrials=1, a=ONE, cn=ONE, ch=ONE, out=ONE, total=None, start=0, lo=0, hi=None):
    nk = p.nk if p is not None else 0
    total = nk if total is None else total
    rc = _lib.lib().scldpc_peel_sweep_device_sock16(C.byref(p) if p is not None else None, ntrials, a, cn, ch, total, start, lo,
                                                    total if hi is None else hi, out, None, None)
    return rc, _lib.lib().scldpc_last_error().decode()


def test_cn_ranges_are_checked_against_nk():
    p = E.make_params(4, 8, 50, 1000)
    for kw in (dict(total=p.nk + 1), dict(total=-1), dict(start=-1), dict(lo=-1), dict(hi=p.nk + 1)):
        for ntrials in (1, 0):
            rc, msg = call(p, ntrials=ntrials, **kw)
            assert rc == BAD_ARG and msg == ENTRY + ": CN ranges outside [0,%d]" % p.nk, (kw, msg)
    # any sweep_start at or beyond total_size is a valid (if idle) sweep, and total_size may be anything in [0, nk]
    for kw in (dict(start=p.nk), dict(start=p.nk + 5000), dict(total=0), dict(total=p.L * p.cns_pos, start=5000)):
        assert call(p, ntrials=0, **kw)[0] == OK, kw


def test_buffers_and_ntrials():
    p = E.make_params(3, 6, 10, 40)
    assert call(p, ntrials=0, a=None, cn=None, ch=None, out=None)[0] == OK     # a supported shape, an empty batch
    rc, msg = call(p, ntrials=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials"
    for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(out=None)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials", kw


@pytest.mark.parametrize("p,part", [
    (E.make_params(4, 8, 50, 5000), "at most 65536 CNs per trial"),
    (P(4, 6, 50, 800, 1200), "no instance for dv = 4, dc = 6"),
    (P(3, 6, 2, 10923, 21846), "sockets: vns_pos * dv must fit 16 bits"),
    (P(4, 16, 50, 250, 1000), "dc must be at most 15"),
], ids=["too_many_cns", "pair", "sockets", "dc"])
def test_an_unsupported_shape_is_refused_even_for_an_empty_batch(p, part):
    for ntrials in (0, 1):
        rc, msg = call(p, ntrials=ntrials, a=None if ntrials == 0 else ONE)
        assert rc == TOO_LARGE and msg.startswith(ENTRY + ": ") and part in msg, msg


def test_the_checks_come_in_their_fixed_order():
    bad_shape = E.make_params(4, 8, 50, 5000)
    rc, msg = call(bad_shape, total=bad_shape.nk + 1, a=None)          # ranges before the shape
    assert rc == BAD_ARG and "CN ranges" in msg
    rc, msg = call(bad_shape, a=None)                                   # the shape before the buffers
    assert rc == TOO_LARGE and "65536 CNs" in msg
    rc, msg = call(P(3, 6, 50, 500, 999), total=0)                      # the parameters first
    assert rc == BAD_ARG and "must equal" in msg
    assert call(None, total=0)[0] == BAD_ARG


# ---- the selector ------------------------------------------------------------------------------------------------------
def test_selector_defaults_to_the_first_generation():
    assert PD.SWEEP_SMALL_BY_DEFAULT is False
    p = E.make_params(4, 8, 50, 1000)
    for sweep in ("auto", "first"):
        kind, why = PD.select_sweep(p, "philox", "olmos", True, True, True, sweep)
        assert kind == "first" and why
    assert PD.select_sweep(p, "philox", "olmos", True, True, True)[0] == "first"
    with pytest.raises(ValueError):
        PD.select_sweep(p, "philox", "olmos", True, True, True, "fast")


def test_selector_picks_the_sampler_of_the_pair(monkeypatch):
    sel = PD.select_sweep
    assert sel(E.make_params(4, 8, 50, 1000), "philox", "olmos", True, True, False, "small") == ("small", "sample_philox_sock16")
    for dv, dc in ((3, 6), (5, 10)):
        assert sel(E.make_params(dv, dc, 50, 1000), "philox", "olmos", True, False, True, "small") == ("small", "sample_philox_deg_sock16")
        # the pair's own sampler does not take the ensemble: the first-generation sampler and the cn_sockets pass
        assert sel(E.make_params(dv, dc, 50, 1000), "philox", "olmos", True, True, False, "small") == ("small", "sample_philox+cn_sockets")
    assert sel(E.make_params(4, 8, 20, 4000), "philox", "olmos", True, False, True, "small") == ("small", "sample_philox+cn_sockets")
    monkeypatch.setattr(PD, "SWEEP_SMALL_BY_DEFAULT", True)             # "auto" then follows the same rule, without raising
    assert sel(E.make_params(4, 8, 50, 1000), "philox", "olmos", True, True, False) == ("small", "sample_philox_sock16")
    assert sel(E.make_params(4, 8, 50, 1000), "numpy", "olmos", True, True, False)[0] == "first"
    assert sel(E.make_params(4, 8, 50, 1000), "philox", "olmos", True, True, False, "first")[0] == "first"
    # with the library's own answers
    for (dv, dc, L, N), want in (((4, 8, 50, 1000), "sample_philox_sock16"), ((3, 6, 50, 1000), "sample_philox_deg_sock16"),
                                 ((5, 10, 50, 1000), "sample_philox_deg_sock16"), ((4, 8, 20, 4000), "sample_philox+cn_sockets")):
        p = E.make_params(dv, dc, L, N)
        assert sel(p, "philox", "olmos", E.peel_sweep_sock16_supported(p), E.sock16_supported(p), E.deg_sock16_supported(p),
                   "small") == ("small", want)


def test_selector_refuses_with_a_reason():
    p = E.make_params(4, 8, 50, 1000)
    for args, part in ((("philox", "tail_biting", True, True, True), "tail_biting tables hold global CN ids"),
                       (("philox", "protograph", True, True, True), "protograph tables hold global CN ids"),
                       (("numpy", "olmos", True, True, True), "rng='numpy' draws the codes on the host"),
                       (("philox", "olmos", False, True, True), "at most 65536 CNs per trial")):
        kind, why = PD.select_sweep(p, *args, "small")
        assert kind == "first" and part in why, why


# ---- the command line --------------------------------------------------------------------------------------------------
def test_cli_parses_sweep():
    pos, kw = PD._cli_options([None, "out.dat", "4", "--sweep", "small", "8", "--rng", "philox"], {})
    assert pos == [None, "out.dat", "4", "8"] and kw == {"sweep": "small", "rng": "philox"}
    assert PD._cli_options([None, "--sweep", "auto"], {})[1] == {"sweep": "auto"}
    with pytest.raises(SystemExit):
        PD._cli_options([None, "--sweep", "fast"], {})


def test_simulate_variance_takes_no_sweep(tmp_path):
    with pytest.raises(SystemExit, match="simulate_variance"):
        PD.main_simulate_variance([str(tmp_path / "o.pkl"), "4", "8", "10", "20", "0.45", "T", "U", "2", "2", "none.npy", "--sweep", "small"])
    assert not (tmp_path / "o.pkl").exists()


# ---- simulate_sc_ldpc's calls, with stand-ins for the engine --------------------------------------------------------------
class Recorder:
    """Stand-ins for the engine calls of simulate_sc_ldpc: they record their arguments and hand back CPU tensors."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("sample_philox", "sample_philox_sock16", "sample_philox_deg_sock16", "cn_sockets", "peel_sweep",
                     "peel_sweep_sock16", "accumulate_peel", "clear_channel_range"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def _tables(self, p, T, cn):
        adj = torch.zeros((T, p.n, p.dv), dtype=torch.int16)
        ch = torch.zeros((T, p.nw), dtype=torch.int32)
        return (adj, torch.zeros((T, p.nk, p.dc), dtype=torch.int16), ch) if cn else (adj, ch)

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None, adj16=False, ensemble="olmos"):
        self.calls.append(("sample_philox", trial0, ntrials, tuple(doped), adj16, ensemble))
        return self._tables(p, ntrials, False)

    def sample_philox_sock16(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None):
        self.calls.append(("sample_philox_sock16", trial0, ntrials, tuple(doped)))
        return self._tables(p, ntrials, True)

    def sample_philox_deg_sock16(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None):
        self.calls.append(("sample_philox_deg_sock16", trial0, ntrials, tuple(doped)))
        return self._tables(p, ntrials, True)

    def cn_sockets(self, p, d_adj16, out=None):
        self.calls.append(("cn_sockets", d_adj16.shape[0]))
        return torch.zeros((d_adj16.shape[0], p.nk, p.dc), dtype=torch.int16)

    def clear_channel_range(self, p, d_ch, lo, hi):
        self.calls.append(("clear_channel_range", lo, hi))
        return d_ch

    def peel_sweep(self, p, d_adj, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
        self.calls.append(("peel_sweep", d_adj.shape[0], total_size, sweep_start, lost_lo, lost_hi))
        return {"out": torch.zeros((d_adj.shape[0], 8), dtype=torch.int32), "lost": None}

    def peel_sweep_sock16(self, p, d_adj, d_cn, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
        assert tuple(d_cn.shape) == (d_adj.shape[0], p.nk, p.dc)
        self.calls.append(("peel_sweep_sock16", d_adj.shape[0], total_size, sweep_start, lost_lo, lost_hi))
        return {"out": torch.zeros((d_adj.shape[0], 8), dtype=torch.int32), "lost": None}

    def accumulate_peel(self, d_out, run, max_fuckups=0):
        run[E.PEELRUN_NAMES.index("trials")] += d_out.shape[0]
        return run

    def names(self):
        return [c[0] for c in self.calls]


@pytest.mark.parametrize("l,r,term,bounded,sampler", [(4, 8, True, True, "sample_philox_sock16"),
                                                      (4, 8, False, False, "sample_philox_sock16"),
                                                      (3, 6, True, False, "sample_philox_deg_sock16"),
                                                      (5, 10, False, True, "sample_philox_deg_sock16")])
def test_simulate_sc_ldpc_small_calls_the_selected_sampler_and_decoder(monkeypatch, capfd, l, r, term, bounded, sampler):
    rec = Recorder(monkeypatch)
    L, M, T = 12, 40, 10
    g = PD._Geometry(l, r, L, M, term, bounded, [4])
    t13 = PD.simulate_sc_ldpc(0.4, l, r, L, M, term, False, bounded, False, num_repeats=T, doping_points=[4], rng="philox",
                              seed=3, batch=4, device="cpu", sweep="small")
    assert t13[5] == T
    geo = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    assert rec.calls == [c for t0, nb in ((0, 4), (4, 4), (8, 2)) for c in ((sampler, t0, nb, (4,)), ("peel_sweep_sock16", nb) + geo)]
    assert sampler.replace("+", " + ") + " + peel_sweep_small" in capfd.readouterr().err


def test_simulate_sc_ldpc_small_without_a_second_generation_sampler_and_with_soft_doping(monkeypatch):
    rec = Recorder(monkeypatch)
    monkeypatch.setattr(E, "sock16_supported", lambda p: False)
    g = PD._Geometry(4, 8, 12, 40, True, True, {3: 0.5})
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, num_repeats=3, doping_points={3: 0.5}, rng="philox", device="cpu",
                        sweep="small")
    assert rec.calls == [("sample_philox", 0, 3, (), True, "olmos"), ("cn_sockets", 3), ("clear_channel_range", 120, 140),
                         ("peel_sweep_sock16", 3, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)]


def test_simulate_sc_ldpc_first_and_auto_call_what_they_called(monkeypatch, capfd):
    g = PD._Geometry(4, 8, 12, 40, False, False, [])
    for kw in (dict(), dict(sweep="auto"), dict(sweep="first")):
        rec = Recorder(monkeypatch)
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, False, False, False, False, num_repeats=5, rng="philox", batch=5, device="cpu", **kw)
        assert rec.calls == [("sample_philox", 0, 5, (), True, "olmos"),
                             ("peel_sweep", 5, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)], kw
        err = capfd.readouterr().err
        assert ("peel_sweep (16- or 32-bit CN words)" in err) == (kw.get("sweep") == "first") and "peel_sweep_small" not in err
    rec = Recorder(monkeypatch)                                          # the other ensembles keep their int32 tables
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", device="cpu")
    assert rec.calls[0] == ("sample_philox", 0, 2, (), False, "tail_biting") and rec.names()[1] == "peel_sweep"


def test_simulate_sc_ldpc_small_raises_where_the_selector_refuses(monkeypatch):
    rec = Recorder(monkeypatch)
    base = dict(num_repeats=2, device="cpu", sweep="small")
    with pytest.raises(ValueError, match="tail_biting tables hold global CN ids"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, rng="philox", **base)
    with pytest.raises(ValueError, match="protograph tables hold global CN ids"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, True, True, False, rng="philox", **base)
    with pytest.raises(ValueError, match="rng='numpy'"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, rng="numpy", **base)
    with pytest.raises(ValueError, match="at most 65536 CNs per trial"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 50, 5000, True, False, True, False, rng="philox", **base)
    with pytest.raises(ValueError, match="sweep must be"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, rng="philox", num_repeats=2, device="cpu", sweep="fast")
    assert rec.calls == []                                               # refused before any engine call
