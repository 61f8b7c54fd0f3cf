"""The 4-bit sweep decoder for the tail-biting and protograph ensembles on the CPU: the symbols of the extension header
include/scldpc_ensembles.h, the shape rules of its entries (decided before any device work: placeholder pointers that are never
dereferenced, as tests/test_sweep_small_host.py), the pure selector with local_tables, simulate_sc_ldpc's calls with stand-ins
for the engine, the command line, and the rule that every device entry of the header is in the case table of
tests/test_gpu_buffer_contracts_ens.py."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ONE = C.c_void_p(16)                                                    # non-null placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_ensembles.h")
OLMOS, TB, PG = 0, 1, 2
SAMPLER = "scldpc_sample_philox_ensemble_device_adj16_sock"
DECODERS = ("scldpc_peel_sweep_device_sock16_tb", "scldpc_peel_sweep_device_sock16_tb_wide")
GLOBAL_IDS = "the %s tables hold global CN ids: the 4-bit sweep decoder reads position-local 2-byte rows"


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_ENSEMBLES) and len(declared) == 6
    assert not declared & set(_lib.EXPORTS)                              # scldpc.h and its coverage rule are as they were
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc.h"' in text and L.scldpc_abi_version() == 2
    for name in DECODERS:
        assert getattr(L, name).argtypes == L.scldpc_peel_sweep_device_sock16.argtypes


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_ensembles.h"\nint main(void){scldpc_code_params p={4,8,12,20,40};return (int)sizeof(p)-20;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")],
                   check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def header_device_entries(path):
    """tests/test_buffer_contracts_host.py's header_device_entries, on another header: {scldpc_* function: its non-const d_*
    pointer parameters}."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(scldpc_\w+)\s*\(([^;{]*?)\)\s*;", text):
        params = [a.strip() for a in m.group(2).split(",")]
        outs = [a.split("*")[-1].strip() for a in params if re.search(r"\*\s*d_\w+$", a) and not a.startswith("const")]
        if outs:
            out[m.group(1)] = outs
    return out


def test_every_device_entry_of_the_header_is_in_the_buffer_contract_table():
    import test_gpu_buffer_contracts_ens as G
    entries = header_device_entries(HEADER)
    assert entries == {SAMPLER: ["d_vn_adj16", "d_cn_sock16", "d_chan_bits"], DECODERS[0]: ["d_out", "d_lost_bits"],
                       DECODERS[1]: ["d_out", "d_lost_bits"]}
    assert G.covered_symbols() == set(entries)
    assert len(G.SHAPES) == 2
    for sym, (ensembles, run, expect) in G.CASES.items():
        assert ensembles and callable(run) and callable(expect), sym
    import test_buffer_contracts_host as H                               # the same expression, on the other header: unchanged
    assert not set(entries) & set(H.header_device_entries())


# ---- shape rules: the sampler ------------------------------------------------------------------------------------------------
def sample(p, ens, ntrials=0, a=None, cn=None, ch=None):
    rc = _lib.lib().scldpc_sample_philox_ensemble_device_adj16_sock(C.byref(p), ens, 1, 0, ntrials, 0.5, 0, None, a, cn, ch, None)
    return rc, _lib.lib().scldpc_last_error().decode()


def test_sampler_takes_the_two_ensembles_and_names_the_olmos_entry():
    p = E.make_params(4, 8, 12, 40)
    assert E.ens_sock16_supported(p, "tail_biting") and E.ens_sock16_supported(p, "protograph")
    assert not E.ens_sock16_supported(p, "olmos")
    rc, msg = sample(p, OLMOS)
    assert rc == BAD_ARG and msg.startswith(SAMPLER + ": ") and "scldpc_sample_philox_device_adj16_sock" in msg.split(": ", 1)[1]
    assert sample(p, 3)[0] == BAD_ARG and "unknown ensemble" in sample(p, 3)[1]
    assert sample(p, TB)[0] == OK and sample(p, PG)[0] == OK             # an empty batch of a shape it takes
    for kw in (dict(a=None, cn=ONE, ch=ONE), dict(a=ONE, cn=None, ch=ONE), dict(a=ONE, cn=ONE, ch=None)):
        rc, msg = sample(p, TB, ntrials=1, **kw)
        assert rc == BAD_ARG and msg == SAMPLER + ": null buffer or negative ntrials", kw
    assert sample(p, TB, ntrials=-1, a=ONE, cn=ONE, ch=ONE)[0] == BAD_ARG
    with pytest.raises(KeyError):
        E.ens_sock16_supported(p, "ring")


@pytest.mark.parametrize("p,ens,code,part", [
    (P(4, 8, 3, 20, 40), TB, BAD_ARG, "tail-biting needs L >= dv"),                  # L = dv - 1
    (P(3, 6, 2, 10, 20), TB, BAD_ARG, "tail-biting needs L >= dv"),
    (P(4, 8, 12, 1025, 2050), TB, TOO_LARGE, "at most 8192 sockets per position"),   # 8200 sockets
    (P(4, 8, 12, 1025, 2050), PG, TOO_LARGE, "at most 8192 sockets per position"),
    (P(1, 3, 12, 2731, 8193), TB, TOO_LARGE, "at most 8192 sockets per position"),   # 8193 sockets
    (P(4, 6, 12, 800, 1200), PG, BAD_ARG, "dv | dc"),
    (P(4, 8, 12, 8192, 16384), TB, TOO_LARGE, "vns_pos * dv must fit 16 bits"),      # vns_pos * dv = 65536
    (P(4, 8, 12, 8192, 16384), PG, TOO_LARGE, "vns_pos * dv must fit 16 bits"),
    (P(3, 6, 12, 500, 999), TB, BAD_ARG, "must equal"),                              # invalid parameters
], ids=["L3-dv4", "L2-dv3", "8200-tb", "8200-proto", "8193", "dv-not-dc", "65536-tb", "65536-proto", "invalid"])
def test_sampler_refusals_are_judged_even_for_an_empty_batch(p, ens, code, part):
    assert _lib.lib().scldpc_sample_philox_ensemble_adj16_sock_supported(C.byref(p), ens) == 0
    for ntrials in (0, 1):
        rc, msg = sample(p, ens, ntrials=ntrials, a=None if ntrials == 0 else ONE, cn=ONE, ch=ONE)
        assert rc == code and part in msg, (ntrials, rc, msg)
        if part != "must equal":
            assert msg.startswith(SAMPLER + ": "), msg


def test_sampler_limits_are_taken_at_the_limit():
    S = lambda p, ens: _lib.lib().scldpc_sample_philox_ensemble_adj16_sock_supported(C.byref(p), ens)
    assert S(P(4, 8, 4, 20, 40), TB) == 1 and S(P(3, 6, 3, 10, 20), TB) == 1 and S(P(5, 10, 5, 20, 40), TB) == 1      # L = dv
    assert S(P(4, 8, 3, 20, 40), PG) == 1                                # a chain may be shorter than dv
    assert S(P(4, 8, 12, 1024, 2048), TB) == 1 and S(P(4, 8, 12, 1024, 2048), PG) == 1                               # 8192 sockets
    assert S(P(4, 6, 12, 800, 1200), TB) == 1                            # the ring needs no dv | dc
    assert S(P(4, 8, 12, 20, 40), OLMOS) == 0


# ---- shape rules: the decoders ---------------------------------------------------------------------------------------------
def decode(entry, p, ntrials=1, a=ONE, cn=ONE, ch=ONE, out=ONE, total=None, start=0, lo=0, hi=None):
    total = p.nk if total is None else total
    rc = getattr(_lib.lib(), entry)(C.byref(p), ntrials, a, cn, ch, total, start, lo, total if hi is None else hi, out, None, None)
    return rc, _lib.lib().scldpc_last_error().decode()


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_decoder_shape_rule_is_the_chains_plus_L_at_least_dv(wide):
    entry = DECODERS[wide]
    chain = E.peel_sweep_wide_supported if wide else E.peel_sweep_sock16_supported
    for p, want in ((E.make_params(4, 8, 12, 40), True), (E.make_params(4, 8, 50, 1000), True), (P(4, 8, 4, 20, 40), True),
                    (P(3, 6, 3, 10, 20), True), (P(5, 10, 5, 20, 40), True), (P(4, 8, 3, 20, 40), False), (P(5, 10, 4, 20, 40), False),
                    (P(4, 6, 50, 800, 1200), False), (P(3, 6, 2, 10923, 21846), False), (P(3, 6, 50, 500, 999), False)):
        assert E.peel_sweep_tb_supported(p, wide=wide) == want, p.key()
        assert E.peel_sweep_tb_supported(p, wide=wide) == (chain(p) and p.L >= p.dv), p.key()
    assert E.peel_sweep_tb_supported(E.make_params(4, 8, 50, 5000), wide=True) and not E.peel_sweep_tb_supported(E.make_params(4, 8, 50, 5000))
    for ntrials in (0, 1):
        rc, msg = decode(entry, P(4, 8, 3, 20, 40), ntrials=ntrials, a=None if ntrials == 0 else ONE)      # L = dv - 1
        assert rc == BAD_ARG and msg.startswith(entry + ": tail-biting needs L >= dv"), msg
        assert decode(entry, P(4, 8, 4, 20, 40), ntrials=0, a=None, cn=None, ch=None, out=None)[0] == OK  # L = dv
        for p, part in ((P(4, 6, 50, 800, 1200), "no instance for dv = 4, dc = 6"), (P(4, 16, 50, 250, 1000), "dc must be at most 15"),
                        (P(3, 6, 2, 10923, 21846), "sockets: vns_pos * dv must fit 16 bits")):
            rc, msg = decode(entry, p, ntrials=ntrials, a=None if ntrials == 0 else ONE)
            assert rc == TOO_LARGE and msg.startswith(entry + ": ") and part in msg, msg


@pytest.mark.parametrize("entry", DECODERS)
def test_decoder_checks_come_in_the_chains_order(entry):
    p = E.make_params(4, 8, 12, 40)
    for kw in (dict(total=p.nk + 1), dict(total=-1), dict(start=-1), dict(lo=-1), dict(hi=p.nk + 1)):
        for ntrials in (1, 0):
            rc, msg = decode(entry, p, ntrials=ntrials, **kw)
            assert rc == BAD_ARG and msg == entry + ": CN ranges outside [0,%d]" % p.nk, (kw, msg)
    # the terminated flag passes total_size = cns_pos * (L + dv - 1) = nk: legal, the CNs above L * cns_pos count zero
    for kw in (dict(total=p.nk), dict(total=p.L * p.cns_pos), dict(total=0), dict(start=p.nk + 5000)):
        assert decode(entry, p, ntrials=0, **kw)[0] == OK, kw
    rc, msg = decode(entry, P(4, 8, 3, 20, 40), total=10 ** 6, a=None)   # ranges before the shape
    assert rc == BAD_ARG and "CN ranges" in msg
    rc, msg = decode(entry, P(4, 8, 3, 20, 40), a=None)                  # the shape before the buffers
    assert rc == BAD_ARG and "L >= dv" in msg
    rc, msg = decode(entry, P(3, 6, 50, 500, 999), total=0)              # the parameters first
    assert rc == BAD_ARG and "must equal" in msg
    for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(out=None), dict(ntrials=-1)):
        rc, msg = decode(entry, p, **kw)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials", kw


def test_engine_keyword_picks_the_entry():
    assert E._sweep_entry("olmos", False) == "scldpc_peel_sweep_device_sock16"
    assert E._sweep_entry("protograph", False) == "scldpc_peel_sweep_device_sock16"
    assert E._sweep_entry("protograph", True) == "scldpc_peel_sweep_device_sock16_wide"
    assert E._sweep_entry("tail_biting", False) == DECODERS[0] and E._sweep_entry("tail_biting", True) == DECODERS[1]
    with pytest.raises(ValueError, match="ensemble must be one of"):
        E._sweep_entry("ring", False)


# ---- the selector ----------------------------------------------------------------------------------------------------------
def test_without_the_switch_every_answer_is_todays():
    sel = PD.select_sweep
    assert PD.LOCAL_TABLES_BY_DEFAULT is False and PD.SWEEP_SMALL_BY_DEFAULT is False and PD.SWEEP_WIDE_BY_DEFAULT is False
    p, big = E.make_params(4, 8, 50, 1000), E.make_params(4, 8, 50, 5000)
    auto = ("first", "sweep='auto' is 'first' (SWEEP_SMALL_BY_DEFAULT)")
    for extra in (dict(), dict(local_tables=False), dict(local_tables=False, ens_sock16_ok=True, tb_ok=True)):
        assert sel(p, "philox", "olmos", True, True, True, **extra) == auto
        assert sel(p, "numpy", "tail_biting", True, True, True, "first", **extra) == ("first", "sweep='first'")
        assert sel(p, "philox", "olmos", True, True, False, "small", **extra) == ("small", "sample_philox_sock16")
        assert sel(p, "philox", "olmos", True, False, True, "small", **extra) == ("small", "sample_philox+cn_sockets")
        assert sel(E.make_params(3, 6, 50, 1000), "philox", "olmos", True, False, True, "small", **extra) == ("small", "sample_philox_deg_sock16")
        for ens in ("tail_biting", "protograph"):
            assert sel(p, "philox", ens, True, True, True, "small", **extra) == ("first", GLOBAL_IDS % ens)
            assert sel(p, "philox", ens, True, True, True, "wide", wide_ok=True, wide_sock16_ok=True, **extra) == ("first", GLOBAL_IDS % ens)
        assert sel(p, "numpy", "olmos", True, True, True, "small", **extra) == \
            ("first", "rng='numpy' draws the codes on the host: the 4-bit sweep decoder reads the device samplers' tables")
        assert sel(big, "philox", "olmos", False, True, True, "small", **extra) == \
            ("first", "the 4-bit sweep decoder takes the pairs (3,6), (4,8), (5,10) with vns_pos * dv <= 65535 and at most "
                      "65536 CNs per trial (dv = 4, dc = 8, L = 50, M = 5000: 132500 CNs)")
        assert sel(big, "philox", "olmos", False, False, False, "wide", wide_ok=True, wide_sock16_ok=True, **extra) == ("wide", "sample_philox_wide_sock16")
    assert PD.SWEEP_SAMPLERS[:3] == ("sample_philox_sock16", "sample_philox_deg_sock16", "sample_philox+cn_sockets")
    assert PD.SWEEP_WIDE_SAMPLERS[:4] == ("sample_philox_sock16", "sample_philox_deg_sock16", "sample_philox_wide_sock16",
                                          "sample_philox+cn_sockets")
    assert PD.SWEEP_SAMPLERS[3:] == ("sample_philox_ens_sock16",) and PD.SWEEP_WIDE_SAMPLERS[4:] == ("sample_philox_ens_sock16",)


@pytest.mark.parametrize("form", ["small", "wide"])
@pytest.mark.parametrize("ens", ["olmos", "tail_biting", "protograph"])
def test_the_switch_over_ensembles_forms_and_capability_flags(ens, form):
    p = E.make_params(4, 8, 12, 40)
    for chain_ok in (False, True):
        for ens_ok in (False, True):
            for tb_ok in (False, True):
                flags = dict(local_tables=True, ens_sock16_ok=ens_ok, tb_ok=tb_ok)
                if form == "small":
                    got = PD.select_sweep(p, "philox", ens, chain_ok, True, True, "small", **flags)
                    old = PD.select_sweep(p, "philox", ens, chain_ok, True, True, "small")
                else:
                    got = PD.select_sweep(p, "philox", ens, False, True, True, "wide", wide_ok=chain_ok, wide_sock16_ok=True, **flags)
                    old = PD.select_sweep(p, "philox", ens, False, True, True, "wide", wide_ok=chain_ok, wide_sock16_ok=True)
                if ens == "olmos":
                    assert got == old                                    # the switch is not read for the Olmos chain
                    continue
                decoder_ok = tb_ok if ens == "tail_biting" else chain_ok
                if decoder_ok and ens_ok:
                    assert got == (form, "sample_philox_ens_sock16")
                    continue
                kind, why = got
                assert kind == "first" and "global CN ids" not in why and "(dv = 4, dc = 8, L = 12, M = 40: 300 CNs)" in why
                if not decoder_ok:                                       # the decoder's limit is named first
                    assert ("1024 entries in one CU's LDS" in why) == (form == "wide") and "(3,6), (4,8), (5,10)" in why
                    assert ("L >= dv" in why) == (ens == "tail_biting")
                else:
                    assert why.startswith("sample_philox_ens_sock16 takes at most 8192 sockets per position")
        assert got[0] in ("first", form)


def test_the_switch_keeps_the_order_rng_then_ensemble_and_the_other_modes():
    p = E.make_params(4, 8, 12, 40)
    on = dict(local_tables=True, ens_sock16_ok=True, tb_ok=True)
    for sweep in ("small", "wide"):
        kind, why = PD.select_sweep(p, "numpy", "tail_biting", True, True, True, sweep, wide_ok=True, **on)
        assert kind == "first" and why.startswith("rng='numpy' draws the codes on the host")
    assert PD.select_sweep(p, "philox", "tail_biting", True, True, True, "first", **on) == ("first", "sweep='first'")
    assert PD.select_sweep(p, "philox", "tail_biting", True, True, True, "auto", **on) == ("first", "sweep='auto' is 'first' (SWEEP_SMALL_BY_DEFAULT)")
    with pytest.raises(ValueError, match="^sweep must be"):
        PD.select_sweep(p, "philox", "tail_biting", True, True, True, "fast", **on)


def test_auto_reaches_the_switch_through_the_flags(monkeypatch):
    p = E.make_params(4, 8, 12, 40)
    on = dict(local_tables=True, ens_sock16_ok=True, tb_ok=True)
    monkeypatch.setattr(PD, "SWEEP_SMALL_BY_DEFAULT", True)
    assert PD.select_sweep(p, "philox", "protograph", True, False, False, **on) == ("small", "sample_philox_ens_sock16")
    assert PD.select_sweep(p, "philox", "protograph", True, False, False) == ("first", GLOBAL_IDS % "protograph")
    monkeypatch.setattr(PD, "SWEEP_WIDE_BY_DEFAULT", True)
    assert PD.select_sweep(p, "philox", "tail_biting", False, False, False, wide_ok=True, **on) == ("small", "sample_philox_ens_sock16")
    assert PD.select_sweep(p, "philox", "protograph", False, False, False, wide_ok=True, **on) == ("wide", "sample_philox_ens_sock16")


# ---- simulate_sc_ldpc's calls, with stand-ins for the engine ------------------------------------------------------------------
class Recorder:
    """Stand-ins for the engine calls of simulate_sc_ldpc: they record their arguments and hand back CPU tensors."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("sample_philox", "sample_philox_ens_sock16", "sample_philox_sock16", "cn_sockets", "peel_sweep",
                     "peel_sweep_sock16", "peel_sweep_sock16_wide", "accumulate_peel", "clear_channel_range"):
            monkeypatch.setattr(E, name, getattr(self, name))

    def _tables(self, p, T, cn):
        adj = torch.zeros((T, p.n, p.dv), dtype=torch.int16)
        ch = torch.zeros((T, p.nw), dtype=torch.int32)
        return (adj, torch.zeros((T, p.nk, p.dc), dtype=torch.int16), ch) if cn else (adj, ch)

    def sample_philox(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None, adj16=False, ensemble="olmos"):
        self.calls.append(("sample_philox", trial0, ntrials, tuple(doped), adj16, ensemble))
        return self._tables(p, ntrials, False)

    def sample_philox_ens_sock16(self, p, ensemble, seed, trial0, ntrials, eps, doped=(), device=None, out=None):
        self.calls.append(("sample_philox_ens_sock16", ensemble, seed, trial0, ntrials, tuple(doped)))
        return self._tables(p, ntrials, True)

    def sample_philox_sock16(self, p, seed, trial0, ntrials, eps, doped=(), device=None, out=None):
        self.calls.append(("sample_philox_sock16", trial0, ntrials, tuple(doped)))
        return self._tables(p, ntrials, True)

    def cn_sockets(self, p, d_adj16, out=None):
        raise AssertionError("the cn_sockets pass is not part of these runs")

    def clear_channel_range(self, p, d_ch, lo, hi):
        self.calls.append(("clear_channel_range", lo, hi))
        return d_ch

    def peel_sweep(self, p, d_adj, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
        self.calls.append(("peel_sweep", d_adj.shape[0], total_size, sweep_start, lost_lo, lost_hi))
        return {"out": torch.zeros((d_adj.shape[0], 8), dtype=torch.int32), "lost": None}

    def _tables_decoder(name):
        def f(self, p, d_adj, d_cn, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False, **kw):
            assert tuple(d_cn.shape) == (d_adj.shape[0], p.nk, p.dc)
            self.calls.append((name, d_adj.shape[0], total_size, sweep_start, lost_lo, lost_hi, kw))
            return {"out": torch.zeros((d_adj.shape[0], 8), dtype=torch.int32), "lost": None}
        return f

    peel_sweep_sock16 = _tables_decoder("peel_sweep_sock16")
    peel_sweep_sock16_wide = _tables_decoder("peel_sweep_sock16_wide")

    def accumulate_peel(self, d_out, run, max_fuckups=0):
        run[E.PEELRUN_NAMES.index("trials")] += d_out.shape[0]
        return run


@pytest.mark.parametrize("sweep", ["small", "wide"])
@pytest.mark.parametrize("ens,term,bounded", [("tail_biting", True, True), ("tail_biting", False, False), ("protograph", True, False)])
def test_simulate_sc_ldpc_calls_the_sampler_and_the_decoder_with_the_ensemble(monkeypatch, capfd, ens, term, bounded, sweep):
    rec = Recorder(monkeypatch)
    T = 10
    g = PD._Geometry(4, 8, 12, 40, term, bounded, [4])
    t13 = PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, term, ens == "protograph", bounded, ens == "tail_biting", num_repeats=T,
                              doping_points=[4], rng="philox", seed=3, batch=4, device="cpu", sweep=sweep, local_tables=True)
    assert t13[5] == T
    geo = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    decoder = "peel_sweep_sock16" + ("_wide" if sweep == "wide" else "")
    assert rec.calls == [c for t0, nb in ((0, 4), (4, 4), (8, 2))
                         for c in (("sample_philox_ens_sock16", ens, 3, t0, nb, (4,)), (decoder, nb) + geo + ({"ensemble": ens},))]
    line = capfd.readouterr().err
    what = "peel_sweep_small (4-bit CN counts" if sweep == "small" else "peel_sweep_wide (4-bit CN counts, 32-bit queues"
    assert "[scldpc] kernels: sample_philox_ens_sock16 + " + what + (", tail-biting)" if ens == "tail_biting" else ")") in line


def test_simulate_sc_ldpc_soft_doping_on_the_ring(monkeypatch):
    rec = Recorder(monkeypatch)
    g = PD._Geometry(4, 8, 12, 40, True, True, {3: 0.5})
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=3, doping_points={3: 0.5}, rng="philox", device="cpu",
                        sweep="small", local_tables=True)
    assert rec.calls == [("sample_philox_ens_sock16", "tail_biting", 0, 0, 3, ()), ("clear_channel_range", 120, 140),
                         ("peel_sweep_sock16", 3, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi, {"ensemble": "tail_biting"})]


def test_simulate_sc_ldpc_without_the_switch_calls_what_it_called(monkeypatch):
    asked = []
    for name in ("ens_sock16_supported", "peel_sweep_tb_supported"):
        monkeypatch.setattr(E, name, lambda *a, name=name, **k: asked.append(name) or True)
    g = PD._Geometry(4, 8, 12, 40, True, True, [])
    for kw in (dict(), dict(local_tables=None), dict(local_tables=False), dict(sweep="first", local_tables=False)):
        rec = Recorder(monkeypatch)
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=5, rng="philox", batch=5, device="cpu", **kw)
        assert rec.calls == [("sample_philox", 0, 5, (), False, "tail_biting"),
                             ("peel_sweep", 5, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)], kw
    rec = Recorder(monkeypatch)                                          # the Olmos chain under sweep='small': no ensemble keyword
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, num_repeats=5, rng="philox", batch=5, device="cpu", sweep="small")
    assert rec.calls == [("sample_philox_sock16", 0, 5, ()), ("peel_sweep_sock16", 5, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi, {})]
    for sweep in ("small", "wide"):
        with pytest.raises(ValueError, match="^sweep='%s': the tail_biting tables hold global CN ids" % sweep):
            PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", device="cpu", sweep=sweep)
    assert asked == []                                                   # none of these asks the library anything new


def test_simulate_sc_ldpc_local_tables_raises_with_the_reason(monkeypatch):
    rec = Recorder(monkeypatch)
    base = dict(num_repeats=2, device="cpu", local_tables=True)
    with pytest.raises(ValueError, match="^local_tables=True: the Olmos chain's tables are position-local already"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, rng="philox", sweep="small", **base)
    with pytest.raises(ValueError, match="^local_tables=True: sweep='first'$"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, rng="philox", sweep="first", **base)
    with pytest.raises(ValueError, match=r"^local_tables=True: sweep='auto' is 'first' \(SWEEP_SMALL_BY_DEFAULT\)$"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, True, True, False, rng="philox", **base)
    with pytest.raises(ValueError, match="^local_tables=True: rng='numpy' draws the codes on the host"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, rng="numpy", sweep="small", **base)
    with pytest.raises(ValueError, match=r"^local_tables=True: .*tail-biting with L >= dv \(dv = 4, dc = 8, L = 3, M = 40: 120 CNs\)"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 3, 40, True, False, True, True, rng="philox", sweep="small", **base)      # a ring of 3 < dv
    with pytest.raises(ValueError, match=r"^local_tables=True: sample_philox_ens_sock16 takes at most 8192 sockets per position"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 2600, True, True, True, False, rng="philox", sweep="wide", **base)   # 10400 sockets
    with pytest.raises(ValueError, match="^sweep must be"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, rng="philox", sweep="fast", **base)
    assert rec.calls == []                                               # refused before any engine call


def test_the_default_follows_the_constant_and_never_raises(monkeypatch):
    monkeypatch.setattr(PD, "LOCAL_TABLES_BY_DEFAULT", True)
    rec = Recorder(monkeypatch)
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", device="cpu", sweep="small")
    assert [c[0] for c in rec.calls] == ["sample_philox_ens_sock16", "peel_sweep_sock16"]
    rec = Recorder(monkeypatch)                                          # the Olmos chain, and sweep='first': no error from a default
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, False, num_repeats=2, rng="philox", device="cpu", sweep="small")
    PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", device="cpu", sweep="first")
    assert [c[0] for c in rec.calls] == ["sample_philox_sock16", "peel_sweep_sock16", "sample_philox", "peel_sweep"]


def test_local_tables_false_beats_the_constant(monkeypatch):
    monkeypatch.setattr(PD, "LOCAL_TABLES_BY_DEFAULT", True)
    Recorder(monkeypatch)
    with pytest.raises(ValueError, match="^sweep='small': the tail_biting tables hold global CN ids"):
        PD.simulate_sc_ldpc(0.4, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", device="cpu", sweep="small",
                            local_tables=False)


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_cli_parses_local_tables():
    pos, kw = PD._cli_options([None, "out.dat", "4", "--sweep", "small", "8", "--local-tables", "on", "--rng", "philox"], {})
    assert pos == [None, "out.dat", "4", "8"] and kw == {"sweep": "small", "local_tables": True, "rng": "philox"}
    assert PD._cli_options([None, "--local-tables", "off"], {})[1] == {"local_tables": False}
    assert PD._cli_options([None, "--local-tables", "auto"], {})[1] == {"local_tables": None}
    with pytest.raises(SystemExit, match="--local-tables takes on, off or auto"):
        PD._cli_options([None, "--local-tables", "yes"], {})
    assert PD._cli_options([None, "--sweep", "wide"], {})[1] == {"sweep": "wide"}      # the other options as before


def test_ber_sim_passes_the_switch_on(monkeypatch, tmp_path):
    rec = Recorder(monkeypatch)
    out = tmp_path / "ber.dat"
    PD.main_simulate_sc_ldpc([str(out), "4", "8", "10", "20", "[0.4]", "T", "U", "B", "TB", "3", "2000", "[]", "--rng", "philox",
                              "--device", "cpu", "--sweep", "small", "--local-tables", "on"])
    assert [c[0] for c in rec.calls] == ["sample_philox_ens_sock16", "peel_sweep_sock16"] and rec.calls[0][1] == "tail_biting"
    assert open(out).read().startswith("# SC-LDPC (4,8,L=10,M=20)")


def test_simulate_variance_takes_no_local_tables(tmp_path):
    with pytest.raises(SystemExit, match="simulate_variance"):
        PD.main_simulate_variance([str(tmp_path / "o.pkl"), "4", "8", "10", "20", "0.45", "T", "U", "2", "2", "none.npy",
                                   "--local-tables", "on"])
    assert not (tmp_path / "o.pkl").exists()
