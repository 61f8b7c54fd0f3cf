"""The wide 4-bit sweep decoder (peel_sweep_small.hip, WIDE instances) on the CPU: its two symbols, the shape rule behind
scldpc_peel_sweep_wide_supported recomputed from the documented formula, the refusals decided before any device work
(placeholder pointers that are never dereferenced, as tests/test_sweep_small_host.py), the pure selector of simulate_sc_ldpc,
the command line, and simulate_sc_ldpc's calls with stand-ins for the engine.

A sweep_start that only a launch can judge exists in this form: (4,8), L = 90, M = 4000 has 186 000 CNs; at sweep_start = 0 its
state is 138 448 B and a queue holds 3108 entries, at sweep_start = total_size = nk the frozen bitmap takes 23 250 B more and a
queue would hold 200."""
import ctypes as C
import os
import re

import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ENTRY = "scldpc_peel_sweep_device_sock16_wide"
ONE = C.c_void_p(16)                                                    # non-null placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_TEXT = "leave fewer than 1024 entries per queue"


def test_the_two_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    for name in ("scldpc_peel_sweep_wide_supported", ENTRY):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert L.scldpc_abi_version() == 2                                   # additions only
    assert L.scldpc_peel_sweep_device_sock16_wide.argtypes == L.scldpc_peel_sweep_device_sock16.argtypes


def queue_entries(p, fz_lim=0):
    """The documented carve: of 160 KiB - 512 B, count words, VN words, frozen bytes, L position flags and 16 scalars, each
    region rounded up to 16 bytes (4 words); two queues of 32-bit entries share the rest evenly, in multiples of 4."""
    r4 = lambda words: (words + 3) & ~3
    state = r4((p.nk + 7) // 8) + r4((p.n + 31) // 32) + r4(((fz_lim + 7) // 8 + 3) // 4) + r4(p.L) + r4(16)
    return (((160 * 1024 - 512) // 4 - state) // 2) & ~3


@pytest.mark.parametrize("shape,want", [((4, 8, 50, 5000), True), ((4, 8, 90, 4000), True), ((4, 8, 90, 5000), False),
                                        ((4, 8, 12, 40), True), ((3, 6, 660, 200), True), ((5, 10, 70, 2500), True)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_supported_follows_the_documented_formula(shape, want):
    p = E.make_params(*shape)
    assert p.vns_pos * p.dv <= 65535 and p.cns_pos <= 65536             # the other limits do not bind on these six
    assert (queue_entries(p) >= 1024) == want
    assert E.peel_sweep_wide_supported(p) == want
    if shape == (4, 8, 90, 4000):
        assert queue_entries(p) == 3108                                  # 138 448 B of state
    if shape == (4, 8, 90, 5000):
        assert p.nk // 2 + p.n // 8 == 172500


@pytest.mark.parametrize("p", [P(4, 6, 50, 800, 1200), P(3, 6, 2, 10923, 21846), P(3, 6, 50, 500, 999)], ids=["pair", "sockets", "invalid"])
def test_supported_refuses_other_pairs_wide_sockets_and_invalid_parameters(p):
    assert E.peel_sweep_wide_supported(p) is False


def test_the_narrow_answers_are_unchanged():
    assert E.peel_sweep_sock16_supported(E.make_params(4, 8, 50, 1000)) and not E.peel_sweep_sock16_supported(E.make_params(4, 8, 50, 5000))


def call(p, ntrials=1, a=ONE, cn=ONE, ch=ONE, out=ONE, total=None, start=0, lo=0, hi=None):
    nk = p.nk if p is not None else 0
    total = nk if total is None else total
    rc = _lib.lib().scldpc_peel_sweep_device_sock16_wide(C.byref(p) if p is not None else None, ntrials, a, cn, ch, total, start, lo,
                                                         total if hi is None else hi, out, None, None)
    return rc, _lib.lib().scldpc_last_error().decode()


def test_cn_ranges_are_checked_against_nk():
    p = E.make_params(4, 8, 50, 5000)
    for kw in (dict(total=p.nk + 1), dict(total=-1), dict(start=-1), dict(lo=-1), dict(hi=p.nk + 1)):
        for ntrials in (1, 0):
            rc, msg = call(p, ntrials=ntrials, **kw)
            assert rc == BAD_ARG and msg == ENTRY + ": CN ranges outside [0,%d]" % p.nk, (kw, msg)
    for kw in (dict(start=p.nk), dict(start=p.nk + 5000), dict(total=0), dict(total=p.L * p.cns_pos, start=5000)):
        assert call(p, ntrials=0, **kw)[0] == OK, kw


def test_buffers_and_ntrials():
    p = E.make_params(3, 6, 660, 200)
    assert call(p, ntrials=0, a=None, cn=None, ch=None, out=None)[0] == OK     # a supported shape, an empty batch
    rc, msg = call(p, ntrials=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials"
    for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(out=None)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials", kw


@pytest.mark.parametrize("p,part", [
    (E.make_params(4, 8, 90, 5000), LDS_TEXT),
    (P(4, 6, 50, 800, 1200), "no instance for dv = 4, dc = 6"),
    (P(3, 6, 2, 10923, 21846), "sockets: vns_pos * dv must fit 16 bits"),
    (P(4, 16, 50, 250, 1000), "dc must be at most 15"),
], ids=["lds", "pair", "sockets", "dc"])
def test_an_unsupported_shape_is_refused_even_for_an_empty_batch(p, part):
    for ntrials in (0, 1):
        rc, msg = call(p, ntrials=ntrials, a=None if ntrials == 0 else ONE)
        assert rc == TOO_LARGE and msg.startswith(ENTRY + ": ") and part in msg, msg


def test_the_checks_come_in_their_fixed_order():
    bad_shape = E.make_params(4, 8, 90, 5000)
    rc, msg = call(bad_shape, total=bad_shape.nk + 1, a=None)          # ranges before the shape
    assert rc == BAD_ARG and "CN ranges" in msg
    rc, msg = call(bad_shape, a=None)                                   # the shape before the buffers
    assert rc == TOO_LARGE and LDS_TEXT in msg
    rc, msg = call(P(3, 6, 50, 500, 999), total=0)                      # the parameters first
    assert rc == BAD_ARG and "must equal" in msg
    assert call(None, total=0)[0] == BAD_ARG


def test_a_sweep_start_only_a_launch_can_judge():
    p = E.make_params(4, 8, 90, 4000)
    assert E.peel_sweep_wide_supported(p) and queue_entries(p) >= 1024 and queue_entries(p, p.nk) < 1024
    first_bad = next(s for s in range(0, p.nk + 1, 8) if queue_entries(p, s) < 1024)
    for ntrials in (0, 1):
        assert call(p, ntrials=0, start=first_bad - 8)[0] == OK
        for start, total in ((p.nk, None), (first_bad, None), (p.nk + 7, p.nk)):
            rc, msg = call(p, ntrials=ntrials, start=start, total=total)
            assert rc == TOO_LARGE and msg.startswith(ENTRY + ": LDS: ") and LDS_TEXT in msg, (start, msg)
        assert call(p, ntrials=0, start=p.nk, total=first_bad - 8)[0] == OK     # fz_lim = min(sweep_start, total_size)


# ---- the selector ------------------------------------------------------------------------------------------------------
def test_the_existing_modes_return_what_they_returned(monkeypatch):
    sel = PD.select_sweep
    assert PD.SWEEP_SMALL_BY_DEFAULT is False and PD.SWEEP_WIDE_BY_DEFAULT is False
    p, big = E.make_params(4, 8, 50, 1000), E.make_params(4, 8, 50, 5000)
    small_refusal = ("the 4-bit sweep decoder takes the pairs (3,6), (4,8), (5,10) with vns_pos * dv <= 65535 and at most "
                     "65536 CNs per trial (dv = 4, dc = 8, L = 50, M = 5000: 132500 CNs)")
    for extra in (dict(), dict(wide_ok=True, wide_sock16_ok=True)):     # the new keywords change nothing for these modes
        for flags in ((True, True, True), (False, False, False), (True, False, True)):
            assert sel(p, "philox", "olmos", *flags, **extra) == ("first", "sweep='auto' is 'first' (SWEEP_SMALL_BY_DEFAULT)")
            assert sel(p, "philox", "olmos", *flags, "auto", **extra) == ("first", "sweep='auto' is 'first' (SWEEP_SMALL_BY_DEFAULT)")
            assert sel(p, "numpy", "tail_biting", *flags, "first", **extra) == ("first", "sweep='first'")
        assert sel(p, "philox", "olmos", True, True, False, "small", **extra) == ("small", "sample_philox_sock16")
        assert sel(p, "philox", "olmos", True, False, True, "small", **extra) == ("small", "sample_philox+cn_sockets")
        assert sel(E.make_params(3, 6, 50, 1000), "philox", "olmos", True, False, True, "small", **extra) == ("small", "sample_philox_deg_sock16")
        assert sel(E.make_params(5, 10, 50, 1000), "philox", "olmos", True, True, False, "small", **extra) == ("small", "sample_philox+cn_sockets")
        assert sel(big, "philox", "olmos", False, True, True, "small", **extra) == ("first", small_refusal)
        assert sel(p, "numpy", "olmos", True, True, True, "small", **extra) == \
            ("first", "rng='numpy' draws the codes on the host: the 4-bit sweep decoder reads the device samplers' tables")
        assert sel(p, "philox", "tail_biting", True, True, True, "small", **extra) == \
            ("first", "the tail_biting tables hold global CN ids: the 4-bit sweep decoder reads position-local 2-byte rows")
    with pytest.raises(ValueError, match="^sweep must be"):
        sel(p, "philox", "olmos", True, True, True, "fast")
    assert not E.peel_sweep_sock16_supported(big)
    assert sel(big, "philox", "olmos", E.peel_sweep_sock16_supported(big), E.sock16_supported(big), E.deg_sock16_supported(big),
               "small") == ("first", small_refusal)
    monkeypatch.setattr(PD, "SWEEP_SMALL_BY_DEFAULT", True)
    assert sel(p, "philox", "olmos", True, True, False) == ("small", "sample_philox_sock16")
    assert sel(big, "philox", "olmos", False, True, False, wide_ok=True, wide_sock16_ok=True) == ("first", small_refusal)


def test_wide_picks_the_sampler_in_the_stated_order():
    sel = lambda p, s, d, w, ws: PD.select_sweep(p, "philox", "olmos", False, s, d, "wide", wide_ok=w, wide_sock16_ok=ws)
    p48, p36, p510 = E.make_params(4, 8, 50, 2600), E.make_params(3, 6, 50, 1000), E.make_params(5, 10, 50, 1000)
    assert sel(p48, True, True, True, True) == ("wide", "sample_philox_sock16")
    assert sel(p48, False, True, True, True) == ("wide", "sample_philox_wide_sock16")      # deg_sock16 is not the (4,8) sampler
    assert sel(p48, False, True, True, False) == ("wide", "sample_philox+cn_sockets")
    for p in (p36, p510):
        assert sel(p, True, True, True, True) == ("wide", "sample_philox_deg_sock16")
        assert sel(p, True, False, True, True) == ("wide", "sample_philox_wide_sock16")    # sock16 is not this pair's sampler
        assert sel(p, True, False, True, False) == ("wide", "sample_philox+cn_sockets")
    # the narrow decoder's answer is not consulted
    assert PD.select_sweep(p48, "philox", "olmos", True, True, False, "wide", wide_ok=True) == ("wide", "sample_philox_sock16")
    # with the library's own answers
    for shape, want in (((4, 8, 90, 1500), "sample_philox_sock16"), ((4, 8, 50, 2600), "sample_philox_wide_sock16"),
                        ((3, 6, 660, 200), "sample_philox_deg_sock16"), ((5, 10, 70, 2500), "sample_philox_wide_sock16"),
                        ((5, 10, 50, 5000), "sample_philox+cn_sockets")):
        p = E.make_params(*shape)
        assert E.peel_sweep_wide_supported(p), shape
        assert sel(p, E.sock16_supported(p), E.deg_sock16_supported(p), E.peel_sweep_wide_supported(p),
                   E.wide_sock16_supported(p)) == ("wide", want), shape


def test_wide_refuses_with_a_reason():
    p = E.make_params(4, 8, 90, 5000)
    for (rng, ens, wide_ok), part in ((("philox", "tail_biting", True), "the tail_biting tables hold global CN ids: the 4-bit sweep decoder"),
                                      (("philox", "protograph", True), "the protograph tables hold global CN ids: the 4-bit sweep decoder"),
                                      (("numpy", "olmos", True), "rng='numpy' draws the codes on the host"),
                                      (("philox", "olmos", False), "(3,6), (4,8), (5,10)"),
                                      (("philox", "olmos", False), "vns_pos * dv <= 65535"),
                                      (("philox", "olmos", False), "1024 entries in one CU's LDS"),
                                      (("philox", "olmos", False), "(dv = 4, dc = 8, L = 90, M = 5000: 232500 CNs)")):
        kind, why = PD.select_sweep(p, rng, ens, True, True, True, "wide", wide_ok=wide_ok, wide_sock16_ok=True)
        assert kind == "first" and part in why, why
    # without the keywords the wide mode has no decoder
    assert PD.select_sweep(p, "philox", "olmos", True, True, True, "wide")[0] == "first"
    # the order: rng, then the ensemble, then the decoder
    assert "rng=" in PD.select_sweep(p, "numpy", "tail_biting", True, True, True, "wide")[1]
    assert "tail_biting" in PD.select_sweep(p, "philox", "tail_biting", True, True, True, "wide")[1]


def test_auto_consults_the_wide_flag_after_the_small_rule(monkeypatch):
    sel = PD.select_sweep
    p, big = E.make_params(4, 8, 50, 1000), E.make_params(4, 8, 50, 5000)
    both_ok = dict(wide_ok=True, wide_sock16_ok=True)
    monkeypatch.setattr(PD, "SWEEP_WIDE_BY_DEFAULT", True)              # wide alone
    assert sel(p, "philox", "olmos", True, True, False, **both_ok) == ("wide", "sample_philox_sock16")
    assert sel(big, "philox", "olmos", False, False, False, **both_ok) == ("wide", "sample_philox_wide_sock16")
    assert sel(big, "numpy", "olmos", False, False, False, **both_ok)[0] == "first"
    assert sel(big, "philox", "olmos", False, False, False)[0] == "first" and "one CU's LDS" in sel(big, "philox", "olmos", False, False, False)[1]
    assert sel(p, "philox", "olmos", True, True, False, "first", **both_ok) == ("first", "sweep='first'")
    monkeypatch.setattr(PD, "SWEEP_SMALL_BY_DEFAULT", True)             # both: small where it applies, wide where small declines
    assert sel(p, "philox", "olmos", True, True, False, **both_ok) == ("small", "sample_philox_sock16")
    assert sel(big, "philox", "olmos", False, False, False, **both_ok) == ("wide", "sample_philox_wide_sock16")
    kind, why = sel(big, "philox", "olmos", False, False, False)        # both decline: the small rule's reason
    assert kind == "first" and "at most 65536 CNs per trial" in why
    monkeypatch.setattr(PD, "SWEEP_WIDE_BY_DEFAULT", False)             # small alone: as before
    assert sel(big, "philox", "olmos", False, False, False, **both_ok)[0] == "first"


# ---- the command line --------------------------------------------------------------------------------------------------
def test_cli_parses_sweep_wide():
    pos, kw = PD._cli_options([None, "out.dat", "4", "--sweep", "wide", "8", "--rng", "philox"], {})
    assert pos == [None, "out.dat", "4", "8"] and kw == {"sweep": "wide", "rng": "philox"}
    for v in ("first", "small", "auto"):
        assert PD._cli_options([None, "--sweep", v], {})[1] == {"sweep": v}
    with pytest.raises(SystemExit):
        PD._cli_options([None, "--sweep", "fast"], {})


def test_simulate_variance_takes_no_sweep(tmp_path):
    with pytest.raises(SystemExit, match="simulate_variance"):
        PD.main_simulate_variance([str(tmp_path / "o.pkl"), "4", "8", "10", "20", "0.45", "T", "U", "2", "2", "none.npy", "--sweep", "wide"])
    assert not (tmp_path / "o.pkl").exists()


# ---- simulate_sc_ldpc's calls, with stand-ins for the engine --------------------------------------------------------------
class Recorder:
    """Stand-ins for the engine calls of simulate_sc_ldpc: they record their arguments and hand back CPU tensors."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("sample_philox", "sample_philox_sock16", "sample_philox_deg_sock16", "sample_philox_wide_sock16", "cn_sockets",
                     "peel_sweep", "peel_sweep_sock16", "peel_sweep_sock16_wide", "accumulate_peel", "clear_channel_range"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def _tables(self, p, T, cn):
        adj = torch.zeros((T, p.n, p.dv), dtype=torch.int16)
        ch = torch.zeros((T, p.nw), dtype=torch.int32)
        return (adj, torch.zeros((T, p.nk, p.dc), dtype=torch.int16), ch) if cn else (adj, ch)

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None, adj16=False, ensemble="olmos"):
        self.calls.append(("sample_philox", trial0, ntrials, tuple(doped), adj16, ensemble))
        return self._tables(p, ntrials, False)

    def _second(name):
        def f(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None):
            self.calls.append((name, trial0, ntrials, tuple(doped)))
            return self._tables(p, ntrials, True)
        return f

    sample_philox_sock16 = _second("sample_philox_sock16")
    sample_philox_deg_sock16 = _second("sample_philox_deg_sock16")
    sample_philox_wide_sock16 = _second("sample_philox_wide_sock16")

    def cn_sockets(self, p, d_adj16, out=None):
        self.calls.append(("cn_sockets", d_adj16.shape[0]))
        return torch.zeros((d_adj16.shape[0], p.nk, p.dc), dtype=torch.int16)

    def clear_channel_range(self, p, d_ch, lo, hi):
        self.calls.append(("clear_channel_range", lo, hi))
        return d_ch

    def peel_sweep(self, p, d_adj, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
        self.calls.append(("peel_sweep", d_adj.shape[0], total_size, sweep_start, lost_lo, lost_hi))
        return {"out": torch.zeros((d_adj.shape[0], 8), dtype=torch.int32), "lost": None}

    def _tables_decoder(name):
        def f(self, p, d_adj, d_cn, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
            assert tuple(d_cn.shape) == (d_adj.shape[0], p.nk, p.dc)
            self.calls.append((name, d_adj.shape[0], total_size, sweep_start, lost_lo, lost_hi))
            return {"out": torch.zeros((d_adj.shape[0], 8), dtype=torch.int32), "lost": None}
        return f

    peel_sweep_sock16 = _tables_decoder("peel_sweep_sock16")
    peel_sweep_sock16_wide = _tables_decoder("peel_sweep_sock16_wide")

    def accumulate_peel(self, d_out, run, max_fuckups=0):
        run[E.PEELRUN_NAMES.index("trials")] += d_out.shape[0]
        return run

    def names(self):
        return [c[0] for c in self.calls]


@pytest.mark.parametrize("l,r,L,M,term,bounded,sampler", [(4, 8, 12, 40, True, True, "sample_philox_sock16"),
                                                          (4, 8, 12, 40, False, False, "sample_philox_sock16"),
                                                          (3, 6, 12, 40, True, False, "sample_philox_deg_sock16"),
                                                          (5, 10, 12, 40, False, True, "sample_philox_deg_sock16"),
                                                          (4, 8, 12, 2600, True, True, "sample_philox_wide_sock16")])
def test_simulate_sc_ldpc_wide_calls_the_selected_sampler_and_decoder(monkeypatch, capfd, l, r, L, M, term, bounded, sampler):
    rec = Recorder(monkeypatch)
    T = 10
    g = PD._Geometry(l, r, L, M, term, bounded, [4])
    t13 = PD.simulate_sc_ldpc(0.4, l, r, L, M, term, False, bounded, False, num_repeats=T, doping_points=[4], rng="philox",
                              seed=3, batch=4, device="cpu", sweep="wide")
    assert t13[5] == T
    geo = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    assert rec.calls == [c for t0, nb in ((0, 4), (4, 4), (8, 2)) for c in ((sampler, t0, nb, (4,)), ("peel_sweep_sock16_wide", nb) + geo)]
    assert sampler + " + peel_sweep_wide (4-bit CN counts, 32-bit queues)" in capfd.readouterr().err


def test_simulate_sc_ldpc_wide_without_a_second_generation_sampler_and_with_soft_doping(monkeypatch, capfd):
    rec = Recorder(monkeypatch)
    monkeypatch.setattr(E, "sock16_supported", lambda p: False)
    monkeypatch.setattr(E, "wide_sock16_supported", lambda p: False)
    g = PD._Geometry(4, 8, 12, 40, True, True, {3: 0.5})
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, num_repeats=3, doping_points={3: 0.5}, rng="philox", device="cpu",
                        sweep="wide")
    assert rec.calls == [("sample_philox", 0, 3, (), True, "olmos"), ("cn_sockets", 3), ("clear_channel_range", 120, 140),
                         ("peel_sweep_sock16_wide", 3, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)]
    assert "sample_philox + cn_sockets + peel_sweep_wide (4-bit CN counts, 32-bit queues)" in capfd.readouterr().err


def test_simulate_sc_ldpc_first_auto_and_small_call_what_they_called(monkeypatch, capfd):
    g = PD._Geometry(4, 8, 12, 40, False, False, [])
    asked = []
    for name in ("peel_sweep_wide_supported", "wide_sock16_supported"):
        monkeypatch.setattr(E, name, lambda p, name=name: asked.append(name) or True)
    for kw in (dict(), dict(sweep="auto"), dict(sweep="first")):
        rec = Recorder(monkeypatch)
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, False, False, False, False, num_repeats=5, rng="philox", batch=5, device="cpu", **kw)
        assert rec.calls == [("sample_philox", 0, 5, (), True, "olmos"),
                             ("peel_sweep", 5, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)], kw
        err = capfd.readouterr().err
        assert ("peel_sweep (16- or 32-bit CN words)" in err) == (kw.get("sweep") == "first") and "peel_sweep_wide" not in err
    rec = Recorder(monkeypatch)
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, False, False, False, False, num_repeats=5, rng="philox", batch=5, device="cpu", sweep="small")
    assert rec.calls == [("sample_philox_sock16", 0, 5, ()), ("peel_sweep_sock16", 5, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)]
    assert "sample_philox_sock16 + peel_sweep_small (4-bit CN counts)" in capfd.readouterr().err
    assert asked == []                                                   # none of these modes asks the library anything new


def test_simulate_sc_ldpc_wide_raises_where_the_selector_refuses(monkeypatch):
    rec = Recorder(monkeypatch)
    base = dict(num_repeats=2, device="cpu", sweep="wide")
    with pytest.raises(ValueError, match="sweep='wide': the tail_biting tables hold global CN ids"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, rng="philox", **base)
    with pytest.raises(ValueError, match="sweep='wide': the protograph tables hold global CN ids"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, True, True, False, rng="philox", **base)
    with pytest.raises(ValueError, match="sweep='wide': rng='numpy'"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, rng="numpy", **base)
    with pytest.raises(ValueError, match=r"1024 entries in one CU's LDS \(dv = 4, dc = 8, L = 90, M = 5000: 232500 CNs\)"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 50, 5000, False, False, False, False, rng="philox", **base)    # widened to L = 90
    with pytest.raises(ValueError, match="sweep must be"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, rng="philox", num_repeats=2, device="cpu", sweep="fast")
    assert rec.calls == []                                               # refused before any engine call
