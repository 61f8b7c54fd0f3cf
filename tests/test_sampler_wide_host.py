"""The second-generation sampler beyond 8192 sockets per CN position, on the CPU: the two symbols, the shape rule behind
scldpc_sample_philox_wide_sock16_supported, the refusal and the argument checks decided before any device work (placeholder
pointers that are never dereferenced, as tests/test_sampler_deg_host.py), the Simulator's choice of the path with the
sampler2_wide switch set, unset and off, the command line, and the registers of every instance of the kernel."""
import ctypes as C
import os
import re
import shutil
import sys

import pytest

from fakes import SelectOnly
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, PRED = "scldpc_sample_philox_device_wide_sock16", "scldpc_sample_philox_wide_sock16_supported"
ONE = C.c_void_p(256)                                                   # non-null placeholder
BAD_ARG, TOO_LARGE = -1, -2
P = _lib.CodeParams

# the shapes tests/test_gpu_sampler_wide.py launches
YES = [(4, 8, 5, 2050), (3, 6, 4, 2734), (5, 10, 6, 1642), (4, 8, 5, 3072), (4, 8, 5, 3074), (4, 8, 5, 4096), (4, 8, 5, 4098),
       (4, 8, 5, 5120), (3, 6, 4, 6826), (5, 10, 6, 4094), (3, 6, 3, 2800), (5, 10, 5, 1700), (4, 8, 50, 5000), (4, 8, 12, 2400),
       (3, 6, 12, 3000), (4, 8, 16, 2400)]
NO = [(4, 8, 50, 2048),         # S = 8192: the neighbour's range
      (3, 6, 5, 2730),          # S = 8190
      (4, 8, 5, 5122),          # S = 20488
      (5, 10, 50, 5000),        # S = 25000
      (3, 9, 7, 3000)]          # another pair


def test_library_exports_and_header_declares_both_symbols():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    for name in (ENTRY, PRED):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert L.scldpc_abi_version() == 2                                   # additions only
    assert callable(E.wide_sock16_supported) and callable(E.sample_philox_wide_sock16)


@pytest.mark.parametrize("shape", YES)
def test_supported_says_yes(shape):
    p = E.make_params(*shape)
    assert 8192 < p.cns_pos * p.dc <= 20480 and E.wide_sock16_supported(p)


@pytest.mark.parametrize("shape", NO)
def test_supported_says_no(shape):
    assert not E.wide_sock16_supported(E.make_params(*shape))


def test_supported_refuses_invalid_parameters():
    fn = getattr(_lib.lib(), PRED)
    assert fn(C.byref(P(4, 8, 50, 2500, 999))) == 0 and fn(None) == 0


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
        assert "dv = 3, dc = 6, dv = 4, dc = 8 or dv = 5, dc = 10" in msg, msg
        assert "more than 8192 and at most 20480 sockets per position" in msg, msg
        assert "dv=%d dc=%d cns_pos=%d: %d sockets" % (p.dv, p.dc, p.cns_pos, p.cns_pos * p.dc) in msg, msg


@pytest.mark.parametrize("shape", [(4, 8, 5, 2050), (3, 6, 50, 5000)])
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
    assert call(P(4, 8, 50, 2500, 999))[0] == BAD_ARG and call(None)[0] == BAD_ARG


# ---- the Simulator's choice ------------------------------------------------------------------------------------------------
def _sim(dv, dc, L, N, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), device="cpu", **kw)


# the configurations beyond 8192 sockets per position whose decoder reads a CN -> socket table today
CASES = [
    ("wide_rows", (4, 8, 50, 5000), dict(max_it=500, rows_cap=64), "wide"),
    ("wide", (4, 8, 50, 5000), dict(max_it=500), "wide"),
    ("caps_wide", (4, 8, 50, 5000), dict(caps=[175, 200, 250], fused_caps=True), "wide"),
    ("degwide", (3, 6, 50, 5000), dict(deg=True, max_it=500), "degwide"),
    ("sw_ring", (4, 8, 100, 2500), dict(decoder="sw", W=10, max_it=20), "sw_ring"),
    ("ring_deg", (3, 6, 100, 3000), dict(decoder="sw", W=10, max_it=20, ring=True), "sw_ring"),
    ("classical_ring", (4, 8, 100, 2500), dict(decoder="swc", W=10, max_it=20, ring=True), "swc_ring"),
]


def test_the_constant_stays_off():
    assert B.SAMPLER2_WIDE_BY_DEFAULT is False


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_simulator_takes_the_wide_sampler_where_the_decoder_reads_a_socket_table(case, monkeypatch):
    name, shape, kw, decoder = case
    monkeypatch.setattr(B, "SAMPLER2_WIDE_BY_DEFAULT", False)
    today = _sim(*shape, sampler2_wide=False, **kw)
    assert today.path.sampler == "first" and today.path.decoder == decoder
    # (the (4,8) ring leaves its table to E.sw_bp: no pass of the Simulator's, no table of its own)
    assert today.path.cn_pass or (name == "sw_ring" and today.path.cn_table is None)
    s = _sim(*shape, sampler2_wide=True, **kw)
    assert s.path == today.path._replace(sampler="wide_sock16", cn_table="sock", cn_pass=False)
    assert s.sampler2_wide_reason is None
    new = "sampler_v2 wide (dv = %d, dc = %d, CN->socket table)" % shape[:2]
    if name == "sw_ring":
        assert today.kernel_choice() == "sampler (first generation) + sw_ring + cn_sockets pass"
        assert s.kernel_choice() == new + " + sw_ring (window state in LDS)"
    else:
        assert "sampler (first generation) + cn_sockets pass + " in today.kernel_choice()
        assert s.kernel_choice() == today.kernel_choice().replace("sampler (first generation) + cn_sockets pass", new)
    # the decoder's own flags stay where they were
    assert (s.ring_deg, s.wide, s.deg, s.lvl2, s.gen2) == (today.ring_deg, today.wide, today.deg, today.lvl2, today.gen2)
    # unset or off: the path and the line without the switch
    for want in (None, False):
        off = _sim(*shape, sampler2_wide=want, **kw)
        assert off.path == today.path and off.kernel_choice() == today.kernel_choice()
        assert off.sampler2_wide_reason == "switched off"
    plain = SelectOnly(E.make_params(*shape), device="cpu", **kw)       # the keyword not given at all
    assert plain.path == today.path and plain.kernel_choice() == today.kernel_choice()
    # the constant decides for None
    monkeypatch.setattr(B, "SAMPLER2_WIDE_BY_DEFAULT", True)
    assert _sim(*shape, **kw).path.sampler == "wide_sock16" and _sim(*shape, sampler2_wide=False, **kw).path == today.path
    # both switches on: the new sampler runs, and no first-generation sampler is left to take the table from
    both = _sim(*shape, sampler2_wide=True, sampled_table=True, **kw)
    assert both.path == s.path and "second-generation sampler" in both.sampled_table_reason
    # --sampler2 does not take these shapes, and leaves them to this switch
    assert _sim(*shape, sampler2=True, sampler2_wide=True, **kw).path == s.path


def test_kernel_choice_lines_of_the_new_path():
    lines = {name: _sim(*shape, sampler2_wide=True, **kw).kernel_choice() for name, shape, kw, _ in CASES}
    assert lines["wide_rows"] == ("sampler_v2 wide (dv = 4, dc = 8, CN->socket table) + full_bp_small wide level-synchronous "
                                  "(4-bit CN counts, 32-bit queue entries, trajectory rows)")
    assert lines["degwide"].startswith("sampler_v2 wide (dv = 3, dc = 6, CN->socket table) + full_bp_small wide level-synchronous (")
    assert lines["ring_deg"] == "sampler_v2 wide (dv = 3, dc = 6, CN->socket table) + sw_ring (window state in LDS, dv = 3, dc = 6)"
    assert lines["classical_ring"] == ("sampler_v2 wide (dv = 4, dc = 8, CN->socket table) + sw_ring classical window (window state "
                                       "in LDS, dv = 4, dc = 8)")


REFUSED = [
    ((4, 8, 50, 5000), dict(max_it=500, rng="glibc"), "--rng glibc samples the code on the host"),
    ((4, 8, 50, 2048), dict(max_it=500), "at most 8192 sockets per position takes this ensemble"),          # S = 8192
    ((3, 6, 50, 1000), dict(deg=True, max_it=500), "more than 8192 and at most 20480 sockets per position (dv = 3, dc = 6, N = 1000: "
                                                   "3000 sockets)"),
    ((5, 10, 50, 5000), dict(deg=True, max_it=500), "at most 20480 sockets per position (dv = 5, dc = 10, N = 5000: 25000 sockets)"),
    ((4, 8, 50, 5000), dict(schedule="fixpoint"), "reads no CN -> socket table"),               # keeps full_bp_fixpoint
    ((4, 8, 50, 5000), dict(max_it=500, wide=False), "reads no CN -> socket table"),
    ((3, 6, 50, 5000), dict(max_it=500), "reads no CN -> socket table"),                        # full_bp: --deg not on
]


@pytest.mark.parametrize("shape,kw,part", REFUSED)
def test_where_it_does_not_apply_the_path_stays_and_the_reason_says_why(shape, kw, part, monkeypatch):
    monkeypatch.setattr(B, "SAMPLER2_WIDE_BY_DEFAULT", False)
    today = _sim(*shape, **kw)
    s = _sim(*shape, sampler2_wide=True, **kw)
    assert s.path == today.path and s.kernel_choice() == today.kernel_choice()
    assert part in s.sampler2_wide_reason, s.sampler2_wide_reason


# ---- the command line --------------------------------------------------------------------------------------------------------
def _argv(prog, *more):
    return ["0", "10", "0", "6"] + (["60"] if prog == "sw_lim_iter" else ["0"] if prog == "bp_traj" else []) + list(more)


def test_the_three_parsers_accept_the_switch():
    for prog in ("bp_lim_iter", "bp_traj", "sw_lim_iter"):
        ap = B._parser(prog)
        assert ap.parse_args(_argv(prog)).sampler2_wide == "auto"
        for v in ("auto", "on", "off"):
            assert ap.parse_args(_argv(prog, "--sampler2-wide", v)).sampler2_wide == v
        with pytest.raises(SystemExit):
            ap.parse_args(_argv(prog, "--sampler2-wide", "maybe"))


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
    monkeypatch.setattr(B, "SAMPLER2_WIDE_BY_DEFAULT", False)
    out = ["--outdir", str(tmp_path)]
    big = ["--N", "5000", "--L", "50"]
    s = _run(monkeypatch, "bp_traj", *big, "--sampler2-wide", "on", *out)
    assert s.want_sampler2_wide is True and s.path.sampler == "wide_sock16" and s.path.decoder == "wide" and not s.path.cn_pass
    s = _run(monkeypatch, "bp_traj", *big, "--sampler2-wide", "off", *out)
    assert s.want_sampler2_wide is False and s.path.sampler == "first" and s.path.cn_pass
    s = _run(monkeypatch, "bp_traj", *big, *out)
    assert s.want_sampler2_wide is None and s.path.sampler == "first" and s.path.cn_pass
    s = _run(monkeypatch, "bp_lim_iter", *big, "--sampler2-wide", "on", *out)
    assert s.path.sampler == "wide_sock16" and s.path.decoder == "wide"
    s = _run(monkeypatch, "bp_lim_iter", "--dv", "3", "--dc", "6", *big, "--deg", "on", "--sampler2-wide", "on", *out)
    assert s.path.sampler == "wide_sock16" and s.path.decoder == "degwide"
    s = _run(monkeypatch, "sw_lim_iter", "--N", "2500", "--L", "100", "--sampler2-wide", "on", *out)
    assert s.path.sampler == "wide_sock16" and s.path.decoder == "sw_ring" and s.path.cn_table == "sock"
    s = _run(monkeypatch, "bp_lim_iter", *big, "--caps", "3,4", "--caps-fused", "on", "--sampler2-wide", "on", *out)
    assert s.path.sampler == "wide_sock16" and s.path.decoder == "wide" and tuple(s.caps) == (3, 4, 6)


def test_on_where_it_cannot_apply_exits_with_the_reason(monkeypatch, tmp_path):
    out = ["--outdir", str(tmp_path)]
    for prog, more, part in (
            ("bp_lim_iter", ["--N", "1000"], "at most 8192 sockets per position takes this ensemble"),
            ("bp_lim_iter", ["--N", "5000", "--wide", "off"], "reads no CN -> socket table"),
            ("bp_traj", ["--N", "5000", "--rng", "glibc"], "--rng glibc samples the code on the host"),
            ("bp_lim_iter", ["--dv", "5", "--dc", "10", "--N", "5000", "--deg", "on"], "at most 20480 sockets per position"),
            ("sw_lim_iter", ["--dv", "3", "--dc", "6", "--N", "200", "--L", "16", "--ring", "on"], "more than 8192")):
        with pytest.raises(SystemExit) as e:
            _run(monkeypatch, prog, "--sampler2-wide", "on", *more, *out)
        assert str(e.value).startswith("--sampler2-wide on: ") and part in str(e.value), (prog, more, str(e.value))
        _run(monkeypatch, prog, "--sampler2-wide", "auto", *more, *out)                           # auto and off run as before
        _run(monkeypatch, prog, "--sampler2-wide", "off", *more, *out)
    # both switches on: --sampled-table on's own refusal
    with pytest.raises(SystemExit) as e:
        _run(monkeypatch, "bp_traj", "--N", "5000", "--sampler2-wide", "on", "--sampled-table", "on", *out)
    assert str(e.value).startswith("--sampled-table on: ") and "second-generation sampler" in str(e.value)


# ---- the registers of every instance: a 1024-thread workgroup leaves a wave 128 VGPRs ------------------------------------------
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def wide_asm(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_ledger as IL
    out = tmp_path_factory.mktemp("wide") / "w.s"
    IL.compile_asm(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "sampler_v2_wide.hip"), str(out))
    return IL, out.read_text()


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="needs hipcc to build the assembly")
@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("calls", [3, 4, 5])
@pytest.mark.parametrize("dv,dc", [(3, 6), (4, 8), (5, 10)])
def test_every_instance_fits_128_vgprs_without_scratch(wide_asm, dv, dc, calls, table):
    IL, text = wide_asm
    name, _, res = IL.parse_kernel(text, "sample_philox_v2_wide_kernelILi%dELi%dELi%dELb%dEE" % (dv, dc, calls, table))
    assert "sample_philox_v2_wide_kernel" in name
    assert res["NumVgprs"] <= 128 and res["ScratchSize"] == 0 and res["VgprSpills"] == 0, res
