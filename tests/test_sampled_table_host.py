"""The CN -> socket table from the first-generation sampler's own launch, on the CPU: the two symbols, the shape rule behind
scldpc_sample_philox_adj16_sock_supported, the argument checks decided before any device work (placeholder pointers that are
never dereferenced, as tests/test_deg_host.py), the Simulator's choice of the path for the seven configurations that run the
cn_sockets pass (or leave the table to engine.sw_bp) today, and the command line."""
import ctypes as C
import os
import re

import pytest
import torch

from fakes import SelectOnly
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

ENTRY, PRED = "scldpc_sample_philox_device_adj16_sock", "scldpc_sample_philox_adj16_sock_supported"
ONE = C.c_void_p(256)                                                   # non-null placeholder
BAD_ARG, TOO_LARGE = -1, -2
P = _lib.CodeParams
NEW = "sampler (first generation, CN->socket table)"


def test_library_exports_and_header_declares_both_symbols():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "scldpc.h")).read()
    for name in (ENTRY, PRED):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert L.scldpc_abi_version() == 2                                   # additions only


YES = [(3, 6, 8, 50), (5, 10, 12, 200), (3, 9, 7, 60), (4, 8, 50, 5000), (4, 8, 50, 10000), (4, 8, 5, 2048), (4, 8, 5, 2050),
       (4, 8, 2, 16382)]


@pytest.mark.parametrize("shape", YES)
def test_supported_says_yes(shape):
    assert E.sample_philox_sock_supported(E.make_params(*shape))


def test_supported_says_no():
    fn = getattr(_lib.lib(), PRED)
    assert not E.sample_philox_sock_supported(E.make_params(4, 8, 5, 16384))      # vns_pos * dv = 65536
    assert fn(C.byref(P(2, 1, 4, 65538, 32769))) == 0                    # cns_pos > 65536 (and sockets beyond 16 bits)
    assert fn(C.byref(P(1, 1, 4, 65537, 65537))) == 0                    # cns_pos > 65536
    assert fn(C.byref(P(2, 1, 4, 40000, 20000))) == 0                    # beyond 8192 sockets per position: cns_pos > 32768
    assert fn(C.byref(P(9, 18, 10, 100, 200))) == 0                      # dv > 8: scldpc_sample_philox_device_adj16 refuses it
    assert fn(C.byref(P(3, 6, 50, 500, 999))) == 0                       # invalid parameters
    assert fn(None) == 0


def call(p, ntrials=1, eps=0.45, doped=(), a=ONE, cn=ONE, ch=ONE):
    arr = (C.c_int32 * max(1, len(doped)))(*doped)
    rc = getattr(_lib.lib(), ENTRY)(C.byref(p) if p is not None else None, 2, 40, ntrials, eps, len(doped), arr if doped else None,
                                    a, cn, ch, None, 0, None)
    return rc, _lib.lib().scldpc_last_error().decode()


def call_adj16(p, ntrials=1, eps=0.45, doped=(), a=ONE, ch=ONE):
    arr = (C.c_int32 * max(1, len(doped)))(*doped)
    return _lib.lib().scldpc_sample_philox_device_adj16(C.byref(p), 2, 40, ntrials, eps, len(doped), arr if doped else None,
                                                        a, ch, None, 0, None)


@pytest.mark.parametrize("shape", [(3, 6, 8, 50), (4, 8, 50, 5000)])
def test_argument_checks_come_before_any_launch(shape):
    p = E.make_params(*shape)
    assert call(p, ntrials=0, a=None, cn=None, ch=None)[0] == 0          # empty batch, null buffers
    rc, msg = call(p, cn=None)                                           # null table
    assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials"
    for kw in (dict(a=None), dict(ch=None), dict(ntrials=-1), dict(eps=1.5), dict(eps=-0.1), dict(eps=float("nan")),
               dict(doped=(shape[2],)), dict(doped=(-1,)), dict(ntrials=0, eps=2.0)):
        rc, msg = call(p, **kw)
        kw16 = {k: v for k, v in kw.items() if k != "cn"}
        assert rc == BAD_ARG and rc == call_adj16(p, **kw16), (kw, rc, msg)     # the codes of the _adj16 entry point
        if "doped" not in kw:
            assert msg.startswith(ENTRY + ": "), msg


def test_refusal_names_the_limit_and_the_entry_point():
    for p, part in ((E.make_params(4, 8, 5, 16384), "vns_pos * dv must fit 16 bits"),
                    (P(1, 1, 4, 65537, 65537), "vns_pos * dv must fit 16 bits"),
                    (P(2, 1, 4, 40000, 20000), "at most 32768 CNs per position")):
        for ntrials in (1, 0):
            rc, msg = call(p, ntrials=ntrials)
            assert rc == TOO_LARGE and msg.startswith(ENTRY + ": ") and part in msg, msg
    assert call(P(3, 6, 50, 500, 999))[0] == BAD_ARG and call(None)[0] == BAD_ARG


def test_the_older_predicates_answer_as_before():
    L = _lib.lib()
    for shape in YES + [(4, 8, 5, 16384), (4, 8, 6, 600), (4, 8, 50, 1000), (4, 8, 100, 1000)]:
        p = E.make_params(*shape)
        dv, dc, _, N = shape
        v2 = (dv, dc) == (4, 8) and N * dv <= 8192
        assert bool(L.scldpc_sample_philox_sock16_supported(C.byref(p))) == v2, shape
        assert bool(L.scldpc_sample_philox_cn16_supported(C.byref(p))) == (v2 and p.n < 65535), shape
    # the table-less entry point still takes what the table mode refuses
    assert call_adj16(E.make_params(4, 8, 5, 16384), ntrials=0) == 0


# ---- the Simulator's choice ------------------------------------------------------------------------------------------------
def _sim(dv, dc, L, N, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), device="cpu", **kw)


# the six configurations whose path ends in cn_pass=True, and the (4,8) ring above 8192 sockets whose table E.sw_bp builds
SEVEN = [
    ("ring_deg", (3, 6, 100, 2000), dict(decoder="sw", W=10, max_it=20, ring=True)),
    ("classical_ring", (5, 10, 50, 1000), dict(decoder="swc", W=10, max_it=20, ring=True)),
    ("caps_wide", (4, 8, 50, 5000), dict(caps=[175, 200, 250], fused_caps=True)),
    ("caps_deg", (3, 6, 50, 1000), dict(caps=[175, 200, 250], fused_caps=True)),
    ("deg16", (5, 10, 50, 1000), dict(deg=True, max_it=500)),
    ("wide_rows", (4, 8, 50, 5000), dict(wide=True, max_it=500, rows_cap=4096, is_term=False)),
    ("ring_4_8", (4, 8, 100, 2500), dict(decoder="sw", W=10, max_it=20)),
]


def test_the_constant_stays_off():
    assert B.SAMPLED_TABLE_BY_DEFAULT is False


@pytest.mark.parametrize("case", SEVEN, ids=lambda c: c[0])
def test_simulator_takes_the_sampled_table_where_a_pass_builds_it_today(case, monkeypatch):
    name, shape, kw = case
    today = _sim(*shape, **kw)
    assert today.path.sampler == "first" and (today.path.cn_pass or name == "ring_4_8")
    assert today.path.cn_pass == ("cn_sockets pass" in today.kernel_choice().replace("sw_ring + cn_sockets pass", "")), today.kernel_choice()
    s = _sim(*shape, sampled_table=True, **kw)
    assert s.path == today.path._replace(sampler="first_sock", cn_table="sock", cn_pass=False)
    assert s.path.sampler == "first_sock" and s.path.cn_pass is False and s.path.cn_table == "sock"
    assert s.kernel_choice().startswith(NEW + " + ") and "cn_sockets" not in s.kernel_choice()
    assert s.kernel_choice().split(" + ", 1)[1].startswith(("sw_ring", "full_bp_small "))
    assert s.sampled_table_reason is None
    # the decoder's own flags stay where they were (the _deg ring entry points, the wide form, the pair's instances)
    assert (s.ring_deg, s.wide, s.deg, s.lvl2, s.gen2) == (today.ring_deg, today.wide, today.deg, today.lvl2, today.gen2)
    # unset or off: exactly today's path and line
    for want in (None, False):
        off = _sim(*shape, sampled_table=want, **kw)
        assert off.path == today.path and off.kernel_choice() == today.kernel_choice()
        assert (off.ring_deg, off.ring2, off.wide, off.wide_sock, off.deg) == (today.ring_deg, today.ring2, today.wide, today.wide_sock, today.deg)
        assert off.sampled_table_reason == "switched off"
    # the measured default decides for None; the library's rule decides
    monkeypatch.setattr(B, "SAMPLED_TABLE_BY_DEFAULT", True)
    assert _sim(*shape, **kw).path.sampler == "first_sock" and _sim(*shape, sampled_table=False, **kw).path == today.path
    monkeypatch.setattr(E, "sample_philox_sock_supported", lambda p: False)
    s = _sim(*shape, sampled_table=True, **kw)
    assert s.path == today.path and s.kernel_choice() == today.kernel_choice() and "vns_pos * dv <= 65535" in s.sampled_table_reason


def test_kernel_choice_lines_of_the_new_path():
    lines = {name: _sim(*shape, sampled_table=True, **kw).kernel_choice() for name, shape, kw in SEVEN}
    assert lines["ring_deg"] == NEW + " + sw_ring (window state in LDS, dv = 3, dc = 6)"
    assert lines["ring_4_8"] == NEW + " + sw_ring (window state in LDS)"
    assert lines["classical_ring"] == NEW + " + sw_ring classical window (window state in LDS, dv = 5, dc = 10)"
    assert lines["deg16"] == NEW + " + full_bp_small level-synchronous (4-bit CN counts, dv = 5, dc = 10)"
    assert lines["wide_rows"] == NEW + " + full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries, trajectory rows)"
    assert lines["caps_wide"] == NEW + (" + full_bp_small wide level-synchronous with 3 cap checkpoints per decode (4-bit CN counts, "
                                        "32-bit queue entries)")


def test_shapes_of_the_second_generation_sampler_never_select_it():
    for shape, kw in (((4, 8, 50, 1000), dict(max_it=500)), ((4, 8, 100, 1000), dict(max_it=500)),
                      ((4, 8, 100, 2000), dict(decoder="sw", W=10, max_it=20)), ((4, 8, 100, 2000), dict(wide=True, max_it=500)),
                      ((4, 8, 50, 2000), dict(decoder="swc", W=10, max_it=20, ring=True)),
                      ((4, 8, 100, 2000), dict(caps=[100, 200], fused_caps=True))):
        today = _sim(*shape, **kw)
        assert today.path.sampler in ("cn16", "sock16")
        s = _sim(*shape, sampled_table=True, **kw)
        assert s.path == today.path and s.kernel_choice() == today.kernel_choice()
        assert "second-generation sampler" in s.sampled_table_reason


def test_glibc_and_table_less_decoders_never_select_it():
    for name, shape, kw in SEVEN:
        if "caps" in kw:
            continue                                                     # (caps take Philox sampling only)
        today = _sim(*shape, rng="glibc", **kw)
        s = _sim(*shape, rng="glibc", sampled_table=True, **kw)
        assert s.path == today.path and s.path.sampler == "glibc" and s.kernel_choice() == today.kernel_choice()
        assert s.sampled_table_reason == "--rng glibc samples the code on the host"
    for shape, kw in (((3, 6, 50, 1000), dict(max_it=500)), ((3, 6, 100, 2000), dict(decoder="sw", W=10, max_it=20)),
                      ((4, 8, 50, 5000), dict(wide=False, max_it=500)), ((5, 10, 50, 1000), dict(decoder="swc", W=10, max_it=20))):
        today = _sim(*shape, **kw)
        s = _sim(*shape, sampled_table=True, **kw)
        assert s.path == today.path and s.path.cn_table is None and s.kernel_choice() == today.kernel_choice()
        assert "reads no CN -> socket table" in s.sampled_table_reason


# ---- the command line --------------------------------------------------------------------------------------------------------
def _argv(prog, *more):
    return ["0", "10", "0", "6"] + (["60"] if prog == "sw_lim_iter" else ["0"] if prog == "bp_traj" else []) + list(more)


def test_the_three_parsers_accept_the_switch():
    for prog in ("bp_lim_iter", "bp_traj", "sw_lim_iter"):
        ap = B._parser(prog)
        assert ap.parse_args(_argv(prog)).sampled_table == "auto"
        for v in ("auto", "on", "off"):
            assert ap.parse_args(_argv(prog, "--sampled-table", v)).sampled_table == v
        with pytest.raises(SystemExit):
            ap.parse_args(_argv(prog, "--sampled-table", "maybe"))
    assert B._parser("bp_lim_iter").parse_args(_argv("bp_lim_iter", "--window", "classical", "--ring", "on", "--sampled-table",
                                                     "on")).sampled_table == "on"


class Seen(Exception):
    pass


def _run(monkeypatch, prog, *more):
    """run_program up to the Simulator it builds (no device): the Simulator's keyword, or the SystemExit of the check."""
    class Probe(SelectOnly):
        def __init__(self, p, **kw):
            kw.pop("device", None)
            super().__init__(p, device="cpu", **kw)

        def run_point(self, *a, **k):
            raise Seen(self)

        def run_point_caps(self, *a, **k):
            raise Seen(self)
    monkeypatch.setattr(B, "Simulator", Probe)
    opts = B._parser(prog).parse_args(_argv(prog, "--quiet", "--seed", "1", "--num-points", "1", "--max-frames", "2", *more))
    extra = getattr(opts, "INIT_IT", None) if prog == "sw_lim_iter" else getattr(opts, "IS_TERM", None)
    with pytest.raises(Seen) as e:
        B.run_program(prog, opts.INDEX, opts.W, opts.NUM_DOPED, opts.MAX_IT, extra, opts)
    return e.value.args[0]


def test_the_switch_reaches_the_simulator(monkeypatch, tmp_path):
    out = ["--outdir", str(tmp_path)]
    s = _run(monkeypatch, "bp_lim_iter", "--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "on", "--sampled-table", "on", *out)
    assert s.want_sampled_table is True and s.path.sampler == "first_sock" and s.path.decoder == "deg16"
    s = _run(monkeypatch, "bp_lim_iter", "--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "on", "--sampled-table", "off", *out)
    assert s.want_sampled_table is False and s.path.sampler == "first" and s.path.cn_pass
    s = _run(monkeypatch, "bp_lim_iter", "--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "on", *out)
    assert s.want_sampled_table is None and s.path.sampler == "first"
    s = _run(monkeypatch, "bp_traj", "--N", "5000", "--wide", "on", "--sampled-table", "on", *out)
    assert s.path.sampler == "first_sock" and s.path.decoder == "wide"
    s = _run(monkeypatch, "sw_lim_iter", "--dv", "5", "--dc", "10", "--N", "200", "--L", "16", "--ring", "on", "--sampled-table", "on", *out)
    assert s.path.sampler == "first_sock" and s.ring_deg
    s = _run(monkeypatch, "sw_lim_iter", "--N", "2500", "--L", "100", "--sampled-table", "on", *out)
    assert s.path == B.Path(torch.int16, "first_sock", "sock", False, "sw_ring", None) and not s.ring_deg
    s = _run(monkeypatch, "bp_lim_iter", "--window", "classical", "--ring", "on", "--N", "2500", "--L", "16", "--sampled-table", "on", *out)
    assert s.path.sampler == "first_sock" and s.path.decoder == "swc_ring"
    s = _run(monkeypatch, "bp_lim_iter", "--N", "5000", "--caps", "3,4", "--caps-fused", "on", "--sampled-table", "on", *out)
    assert s.path.sampler == "first_sock" and s.path.decoder == "wide" and tuple(s.caps) == (3, 4, 6)


def test_on_where_it_cannot_apply_exits_with_the_reason(monkeypatch, tmp_path):
    out = ["--outdir", str(tmp_path)]
    for prog, more, part in (
            ("bp_lim_iter", ["--N", "1000"], "the second-generation sampler takes this ensemble"),
            ("bp_lim_iter", ["--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "off"], "reads no CN -> socket table"),
            ("bp_traj", ["--N", "5000", "--wide", "on", "--rng", "glibc"], "--rng glibc samples the code on the host"),
            ("sw_lim_iter", ["--dv", "3", "--dc", "6", "--N", "200", "--L", "16", "--ring", "off"], "reads no CN -> socket table"),
            ("bp_lim_iter", ["--window", "classical", "--N", "2500", "--L", "16", "--ring", "off"], "reads no CN -> socket table")):
        with pytest.raises(SystemExit) as e:
            _run(monkeypatch, prog, "--sampled-table", "on", *more, *out)
        assert str(e.value).startswith("--sampled-table on: ") and part in str(e.value), (prog, more, str(e.value))
        _run(monkeypatch, prog, "--sampled-table", "auto", *more, *out)                           # auto and off run as before
        _run(monkeypatch, prog, "--sampled-table", "off", *more, *out)
