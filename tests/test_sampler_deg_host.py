"""The second-generation sampler of the pairs (3,6) and (5,10), on the CPU: the two symbols, the shape rule behind
scldpc_sample_philox_deg_sock16_supported, the refusal and the argument checks decided before any device work (placeholder
pointers that are never dereferenced, as tests/test_sampled_table_host.py), the Simulator's choice of the path with the sampler2
switch set, unset and off, and the command line."""
import ctypes as C
import os
import re

import pytest

from fakes import SelectOnly
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

ENTRY, PRED = "scldpc_sample_philox_device_deg_sock16", "scldpc_sample_philox_deg_sock16_supported"
ONE = C.c_void_p(256)                                                   # non-null placeholder
BAD_ARG, TOO_LARGE = -1, -2
P = _lib.CodeParams

# the shapes tests/test_gpu_sampler_deg.py launches
YES = [(3, 6, 8, 52), (3, 6, 8, 50), (5, 10, 7, 50), (5, 10, 12, 200), (5, 10, 5, 818), (5, 10, 5, 820), (3, 6, 6, 1400),
       (3, 6, 5, 2730), (5, 10, 7, 1638), (3, 6, 3, 64), (5, 10, 5, 64), (3, 6, 50, 1000), (5, 10, 50, 1000)]
NO = [(4, 8, 50, 1000),         # has entry points of its own
      (3, 9, 7, 60),            # another pair
      (3, 6, 5, 2734),          # S = 8202
      (5, 10, 5, 1640)]         # S = 8200


def test_library_exports_and_header_declares_both_symbols():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "scldpc.h")).read()
    for name in (ENTRY, PRED):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert L.scldpc_abi_version() == 2                                   # additions only
    assert callable(E.deg_sock16_supported) and callable(E.sample_philox_deg_sock16)


@pytest.mark.parametrize("shape", YES)
def test_supported_says_yes(shape):
    p = E.make_params(*shape)
    assert p.cns_pos * p.dc <= 8192 and E.deg_sock16_supported(p)


@pytest.mark.parametrize("shape", NO)
def test_supported_says_no(shape):
    assert not E.deg_sock16_supported(E.make_params(*shape))


def test_supported_refuses_invalid_parameters():
    fn = getattr(_lib.lib(), PRED)
    assert fn(C.byref(P(3, 6, 50, 500, 999))) == 0 and fn(None) == 0


def call(p, ntrials=1, eps=0.45, doped=(), ndoped=None, a=ONE, cn=ONE, ch=ONE):
    arr = (C.c_int32 * max(1, len(doped)))(*doped)
    rc = getattr(_lib.lib(), ENTRY)(C.byref(p) if p is not None else None, 2, 40, ntrials, eps,
                                    len(doped) if ndoped is None else ndoped, arr if doped else None, a, cn, ch, None)
    return rc, _lib.lib().scldpc_last_error().decode()


@pytest.mark.parametrize("shape", NO)
def test_refusal_names_the_limits_and_what_it_got(shape):
    p = E.make_params(*shape)
    for ntrials in (1, 0):
        rc, msg = call(p, ntrials=ntrials)
        assert rc == TOO_LARGE and msg.startswith(ENTRY + ": "), msg
        assert "dv = 3, dc = 6 or dv = 5, dc = 10" in msg and "at most 8192 sockets per position" in msg, msg
        assert "dv=%d dc=%d cns_pos=%d: %d sockets" % (p.dv, p.dc, p.cns_pos, p.cns_pos * p.dc) in msg, msg


@pytest.mark.parametrize("shape", [(3, 6, 8, 50), (5, 10, 50, 1000)])
def test_argument_checks_come_before_any_launch(shape):
    p = E.make_params(*shape)
    assert call(p, ntrials=0, a=None, cn=None, ch=None)[0] == 0          # empty batch, null buffers
    for kw in (dict(a=None), dict(ch=None), dict(ntrials=-1)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials", (kw, rc, msg)
    for kw in (dict(eps=1.5), dict(eps=-0.1), dict(eps=float("nan")), dict(ntrials=0, eps=2.0)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg.startswith(ENTRY + ": eps="), (kw, rc, msg)
    for kw in (dict(doped=tuple(range(33))), dict(ndoped=33, doped=(1,)), dict(ndoped=-1), dict(ndoped=1)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": 0 <= ndoped <= 32", (kw, rc, msg)
    for kw in (dict(doped=(shape[2],)), dict(doped=(-1,))):
        assert call(p, **kw)[0] == BAD_ARG, kw
    assert call(P(3, 6, 50, 500, 999))[0] == BAD_ARG and call(None)[0] == BAD_ARG


# ---- the Simulator's choice ------------------------------------------------------------------------------------------------
def _sim(dv, dc, L, N, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), device="cpu", **kw)


# the configurations of the pairs (3,6) and (5,10) whose path ends in the cn_sockets pass today
CASES = [
    ("deg16", (5, 10, 50, 1000), dict(deg=True, max_it=500)),
    ("deg16_fixpoint", (3, 6, 50, 1000), dict(deg=True, schedule="fixpoint")),
    ("deg16_rows", (3, 6, 50, 1000), dict(deg=True, max_it=500, rows_cap=64)),
    ("degwide", (3, 6, 100, 2000), dict(deg=True, max_it=500)),
    ("caps_deg", (3, 6, 50, 1000), dict(caps=[175, 200, 250], fused_caps=True)),
    ("caps_degwide", (3, 6, 100, 2000), dict(caps=[175, 200, 250], fused_caps=True)),
    ("ring_deg", (3, 6, 100, 2000), dict(decoder="sw", W=10, max_it=20, ring=True)),
    ("classical_ring", (5, 10, 50, 1000), dict(decoder="swc", W=10, max_it=20, ring=True)),
]
DECODERS = {"deg16": "deg16", "deg16_fixpoint": "deg16", "deg16_rows": "deg16", "degwide": "degwide", "caps_deg": "deg16",
            "caps_degwide": "degwide", "ring_deg": "sw_ring", "classical_ring": "swc_ring"}


def test_the_constant_is_a_bool():
    assert B.SAMPLER2_DEG_BY_DEFAULT in (True, False)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_simulator_takes_the_second_generation_sampler_where_a_pass_builds_the_table_today(case, monkeypatch):
    name, shape, kw = case
    monkeypatch.setattr(B, "SAMPLER2_DEG_BY_DEFAULT", False)
    today = _sim(*shape, sampler2=False, **kw)
    assert today.path.sampler == "first" and today.path.cn_pass and today.path.decoder == DECODERS[name]
    assert "sampler (first generation) + cn_sockets pass + " in today.kernel_choice()
    s = _sim(*shape, sampler2=True, **kw)
    assert s.path == today.path._replace(sampler="deg_sock16", cn_table="sock", cn_pass=False)
    assert s.path.sampler == "deg_sock16" and s.path.cn_pass is False
    assert s.sampler2_deg_reason is None
    new = "sampler_v2 (dv = %d, dc = %d, CN->socket table)" % shape[:2]
    assert s.kernel_choice() == today.kernel_choice().replace("sampler (first generation) + cn_sockets pass", new)
    # the decoder's own flags stay where they were
    assert (s.ring_deg, s.wide, s.deg, s.lvl2, s.gen2, s.ring2) == (today.ring_deg, today.wide, today.deg, today.lvl2, today.gen2,
                                                                   today.ring2)
    # unset or off: the path and the line without the switch
    for want in (None, False):
        off = _sim(*shape, sampler2=want, **kw)
        assert off.path == today.path and off.kernel_choice() == today.kernel_choice()
        assert off.sampler2_deg_reason == "switched off"
    plain = SelectOnly(E.make_params(*shape), device="cpu", **kw)       # the keyword not given at all
    assert plain.path == today.path and plain.kernel_choice() == today.kernel_choice()
    # the measured default decides for None
    monkeypatch.setattr(B, "SAMPLER2_DEG_BY_DEFAULT", True)
    assert _sim(*shape, **kw).path.sampler == "deg_sock16" and _sim(*shape, sampler2=False, **kw).path == today.path
    # both switches on: the first-generation sampler no longer runs, so it cannot write the table
    both = _sim(*shape, sampler2=True, sampled_table=True, **kw)
    assert both.path == s.path and "second-generation sampler" in both.sampled_table_reason


def test_kernel_choice_lines_of_the_new_path():
    lines = {name: _sim(*shape, sampler2=True, **kw).kernel_choice() for name, shape, kw in CASES}
    assert lines["deg16"] == "sampler_v2 (dv = 5, dc = 10, CN->socket table) + full_bp_small level-synchronous (4-bit CN counts, dv = 5, dc = 10)"
    assert lines["ring_deg"] == "sampler_v2 (dv = 3, dc = 6, CN->socket table) + sw_ring (window state in LDS, dv = 3, dc = 6)"
    assert lines["classical_ring"] == ("sampler_v2 (dv = 5, dc = 10, CN->socket table) + sw_ring classical window (window state in LDS, "
                                       "dv = 5, dc = 10)")
    assert lines["degwide"].startswith("sampler_v2 (dv = 3, dc = 6, CN->socket table) + full_bp_small wide level-synchronous (")


REFUSED = [
    ((5, 10, 50, 1000), dict(deg=True, max_it=500, rng="glibc"), "--rng glibc samples the code on the host"),
    ((4, 8, 50, 1000), dict(max_it=500), "dv = 4, dc = 8 has a second-generation sampler of its own"),
    ((4, 8, 50, 5000), dict(wide=True, max_it=500), "dv = 4, dc = 8 has a second-generation sampler of its own"),
    ((3, 6, 50, 5000), dict(deg=True, max_it=500), "at most 8192 sockets per position (dv = 3, dc = 6, N = 5000: 15000 sockets)"),
    ((3, 6, 50, 1000), dict(max_it=500), "reads no CN -> socket table"),                        # full_bp: --deg not on
    ((3, 6, 100, 2000), dict(decoder="sw", W=10, max_it=20), "reads no CN -> socket table"),    # the whole-chain window kernel
    ((5, 10, 50, 1000), dict(decoder="swc", W=10, max_it=20), "reads no CN -> socket table"),
]


@pytest.mark.parametrize("shape,kw,part", REFUSED)
def test_where_it_does_not_apply_the_path_stays_and_the_reason_says_why(shape, kw, part, monkeypatch):
    monkeypatch.setattr(B, "SAMPLER2_DEG_BY_DEFAULT", False)
    today = _sim(*shape, **kw)
    s = _sim(*shape, sampler2=True, **kw)
    assert s.path == today.path and s.kernel_choice() == today.kernel_choice()
    assert part in s.sampler2_deg_reason, s.sampler2_deg_reason


# ---- the command line --------------------------------------------------------------------------------------------------------
def _argv(prog, *more):
    return ["0", "10", "0", "6"] + (["60"] if prog == "sw_lim_iter" else ["0"] if prog == "bp_traj" else []) + list(more)


def test_the_three_parsers_accept_the_switch():
    for prog in ("bp_lim_iter", "bp_traj", "sw_lim_iter"):
        ap = B._parser(prog)
        assert ap.parse_args(_argv(prog)).sampler2 == "auto"
        for v in ("auto", "on", "off"):
            assert ap.parse_args(_argv(prog, "--sampler2", v)).sampler2 == v
        with pytest.raises(SystemExit):
            ap.parse_args(_argv(prog, "--sampler2", "maybe"))


class Seen(Exception):
    pass


def _run(monkeypatch, prog, *more):
    """run_program up to the Simulator it builds (no device): the Simulator, or the SystemExit of the check."""
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
    monkeypatch.setattr(B, "SAMPLER2_DEG_BY_DEFAULT", False)
    out = ["--outdir", str(tmp_path)]
    deg = ["--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "on"]
    s = _run(monkeypatch, "bp_lim_iter", *deg, "--sampler2", "on", *out)
    assert s.want_sampler2 is True and s.path.sampler == "deg_sock16" and s.path.decoder == "deg16" and not s.path.cn_pass
    s = _run(monkeypatch, "bp_lim_iter", *deg, "--sampler2", "off", *out)
    assert s.want_sampler2 is False and s.path.sampler == "first" and s.path.cn_pass
    s = _run(monkeypatch, "bp_lim_iter", *deg, *out)
    assert s.want_sampler2 is None and s.path.sampler == "first" and s.path.cn_pass
    s = _run(monkeypatch, "bp_traj", *deg, "--sampler2", "on", *out)
    assert s.path.sampler == "deg_sock16" and s.path.decoder == "deg16"
    s = _run(monkeypatch, "sw_lim_iter", "--dv", "5", "--dc", "10", "--N", "200", "--L", "16", "--ring", "on", "--sampler2", "on", *out)
    assert s.path.sampler == "deg_sock16" and s.ring_deg
    s = _run(monkeypatch, "bp_lim_iter", "--window", "classical", "--ring", "on", "--dv", "3", "--dc", "6", "--N", "200", "--L", "16",
             "--sampler2", "on", *out)
    assert s.path.sampler == "deg_sock16" and s.path.decoder == "swc_ring"
    s = _run(monkeypatch, "bp_lim_iter", "--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--caps", "3,4", "--caps-fused", "on",
             "--sampler2", "on", *out)
    assert s.path.sampler == "deg_sock16" and s.path.decoder == "deg16" and tuple(s.caps) == (3, 4, 6)


def test_on_where_it_cannot_apply_exits_with_the_reason(monkeypatch, tmp_path):
    out = ["--outdir", str(tmp_path)]
    for prog, more, part in (
            ("bp_lim_iter", ["--N", "1000"], "dv = 4, dc = 8 has a second-generation sampler of its own"),
            ("bp_lim_iter", ["--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "off"], "reads no CN -> socket table"),
            ("bp_traj", ["--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "on", "--rng", "glibc"],
             "--rng glibc samples the code on the host"),
            ("bp_lim_iter", ["--dv", "3", "--dc", "6", "--N", "5000", "--deg", "on"], "at most 8192 sockets per position"),
            ("sw_lim_iter", ["--dv", "3", "--dc", "6", "--N", "200", "--L", "16", "--ring", "off"], "reads no CN -> socket table")):
        with pytest.raises(SystemExit) as e:
            _run(monkeypatch, prog, "--sampler2", "on", *more, *out)
        assert str(e.value).startswith("--sampler2 on: ") and part in str(e.value), (prog, more, str(e.value))
        _run(monkeypatch, prog, "--sampler2", "auto", *more, *out)                                # auto and off run as before
        _run(monkeypatch, prog, "--sampler2", "off", *more, *out)
    # both switches on: --sampled-table on's own refusal
    with pytest.raises(SystemExit) as e:
        _run(monkeypatch, "bp_lim_iter", "--dv", "3", "--dc", "6", "--N", "200", "--L", "12", "--deg", "on", "--sampler2", "on",
             "--sampled-table", "on", *out)
    assert str(e.value).startswith("--sampled-table on: ") and "second-generation sampler" in str(e.value)
