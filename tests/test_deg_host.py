"""The 4-bit level decoder for the degree pairs (3,6) and (5,10) on the CPU: the seven _deg symbols, the host-side shape rule
behind scldpc_full_bp_deg_supported / scldpc_full_bp_deg_wide_supported, the refusals decided before any device work
(placeholder pointers that are never dereferenced, as tests/test_wide_host.py) and the Simulator's choice of the path.

Every refusal of the new forms occurs below except two that no valid shape reaches: "a wave's releases per iteration could
exceed 15 bits" (narrow: needs 65 536 CNs and a carve squeezed to 256 queue entries — the 17-bit bound of dv = 5 trips first
where such a carve exists; wide: below 23 900 for every state that fits the LDS) and "at most 65536 CNs per position" (the
socket limit trips first)."""
import ctypes as C

import pytest
import torch

from fakes import SelectOnly
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

FIX = ("scldpc_full_bp_fixpoint_device_deg",)
LEVEL = ("scldpc_full_bp_device_deg", "scldpc_full_bp_device_deg_wide")
TRAJ = ("scldpc_full_bp_traj_device_deg", "scldpc_full_bp_traj_device_deg_wide")
ALL = FIX + LEVEL + TRAJ
NARROW = tuple(e for e in ALL if not e.endswith("_wide"))
WIDE = tuple(e for e in ALL if e.endswith("_wide"))
ONE = C.c_void_p(16)                                                    # non-null placeholder
BAD_ARG, TOO_LARGE = -1, -2
P = _lib.CodeParams


def test_library_exports_the_deg_entry_points():
    L = _lib.lib()
    for name in ALL + ("scldpc_full_bp_deg_supported", "scldpc_full_bp_deg_wide_supported"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.scldpc_abi_version() == 2                                   # additions only


# dv, dc, L, N, narrow takes it, wide takes it — derived from make_args (the LEVEL carve) and pinned
SHAPES = [
    (3, 6, 50, 1000, True, True), (5, 10, 50, 1000, True, True), (4, 8, 50, 1000, True, True),
    (3, 6, 50, 5000, False, True), (5, 10, 50, 5000, False, True), (4, 8, 50, 5000, False, True),
    (3, 6, 16, 200, True, True), (5, 10, 12, 40, True, True), (3, 6, 9, 24, True, True),
    (3, 6, 50, 2500, True, True),           # 65 000 CNs
    (5, 10, 50, 2500, False, True),         # 67 500 CNs
    (5, 10, 10, 9286, False, True),         # 65 002 CNs on a carve with short narrow queues: the 17-bit bound of the reduction
    (3, 6, 50, 6000, False, True), (5, 10, 50, 6000, False, True),
    (3, 6, 50, 7000, False, False),         # fewer than 1024 entries per wide queue
    (3, 6, 50, 8000, False, False),         # the state leaves no room for the queues
    (5, 10, 50, 7000, False, False),        # the state leaves no room for the queues
    (3, 6, 50, 10000, False, False),        # the state alone exceeds the LDS
]


@pytest.mark.parametrize("dv,dc,L,N,narrow,wide", SHAPES)
def test_deg_supported_follows_the_shape_rule(dv, dc, L, N, narrow, wide):
    p = E.make_params(dv, dc, L, N)
    assert E.full_bp_deg_supported(p) == narrow and E.full_bp_deg_supported(p, wide=True) == wide
    if (L, N) == (50, 5000):
        assert p.nk > 65536


def test_deg_supported_refuses_what_has_no_instance():
    L = _lib.lib()
    for fn in (L.scldpc_full_bp_deg_supported, L.scldpc_full_bp_deg_wide_supported):
        for p in (P(4, 16, 50, 250, 1000), P(3, 9, 50, 300, 900), P(2, 4, 50, 500, 1000), P(6, 12, 50, 500, 1000),
                  P(3, 6, 2, 10923, 21846),                              # 65 538 sockets per position
                  P(5, 10, 2, 6554, 13108),                              # 65 540
                  P(3, 6, 50, 500, 999)):                                # invalid parameters
            assert fn(C.byref(p)) == 0, p.key()
        assert fn(C.byref(P(3, 6, 2, 10922, 21844))) == 1                # 65 532 sockets
        assert fn(None) == 0


def call(entry, p, ntrials=1, a=ONE, cn=ONE, ch=ONE, cnt=ONE, rows=ONE, rows_cap=8):
    fn = getattr(_lib.lib(), entry)
    p = C.byref(p) if p is not None else None
    if entry in FIX:
        rc = fn(p, ntrials, a, cn, ch, 1, cnt, None, None)
    elif entry in LEVEL:
        rc = fn(p, ntrials, a, cn, ch, 0, 1, cnt, None, None)
    else:
        rc = fn(p, ntrials, a, cn, ch, 0, 1, cnt, rows, rows_cap, None, None)
    return rc, _lib.lib().scldpc_last_error().decode()


def good(entry, dv=3, dc=6):
    return E.make_params(dv, dc, 50, 5000 if entry in WIDE else 1000)


# (defect, entry points, parameters, return code, part of the message)
REFUSALS = [
    ("dc beyond a nibble", ALL, P(4, 16, 50, 250, 1000), TOO_LARGE, "dc must be at most 15"),
    ("pair without an instance", ALL, P(3, 9, 50, 300, 900), TOO_LARGE, "no instance for dv = 3, dc = 9"),
    ("pair without an instance", ALL, P(6, 12, 50, 500, 1000), TOO_LARGE, "no instance for dv = 6, dc = 12"),
    ("too many sockets", ALL, P(3, 6, 2, 10923, 21846), TOO_LARGE, "sockets: vns_pos * dv must fit 16 bits (at most 65535)"),
    ("too many CNs", NARROW, E.make_params(3, 6, 50, 5000), TOO_LARGE, "at most 65536 CNs per trial"),
    ("too many CNs", NARROW, E.make_params(5, 10, 50, 2500), TOO_LARGE, "at most 65536 CNs per trial"),
    ("zeroed CNs beyond 17 bits", NARROW, E.make_params(5, 10, 10, 9286), TOO_LARGE,
     "queue: the CNs a wave zeroes per iteration could exceed 17 bits"),
    ("short queues", WIDE, E.make_params(3, 6, 50, 7000), TOO_LARGE, "queue: the LDS left by the state holds fewer than 1024 entries"),
    ("no room for the queues", WIDE, E.make_params(3, 6, 50, 8000), TOO_LARGE, "leave no room for the queues"),
    ("no room for the queues", WIDE, E.make_params(5, 10, 50, 7000), TOO_LARGE, "leave no room for the queues"),
    ("state beyond the LDS", WIDE, E.make_params(5, 10, 50, 10000), TOO_LARGE, "exceed 160 KiB"),
    ("invalid parameters", ALL, P(3, 6, 50, 500, 999), BAD_ARG, "dv*vns_pos (3*999) must equal dc*cns_pos (6*500)"),
    ("null parameters", ALL, None, BAD_ARG, "null scldpc_code_params"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0].replace(" ", "_"))
def test_refusal_names_the_limit_and_the_entry_point(case):
    defect, entries, p, want_rc, part = case
    for entry in entries:
        for ntrials in (1, 0):                                           # the shape is judged even for an empty batch
            rc, msg = call(entry, p, ntrials=ntrials)
            assert rc == want_rc and part in msg, (defect, entry, rc, msg)
            assert msg.startswith(entry + ": ") or defect in ("invalid parameters", "null parameters"), (entry, msg)


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10), (4, 8)])
def test_argument_checks_come_before_any_launch(dv, dc):
    for entry in ALL:
        p = good(entry, dv, dc)
        assert call(entry, p, ntrials=0, a=None, cn=None, ch=None, cnt=None)[0] == 0              # empty batch, null buffers
        rc, msg = call(entry, p, ntrials=-1)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
        for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(cnt=None)):
            rc, msg = call(entry, p, **kw)
            assert rc == BAD_ARG and "null buffer" in msg and msg.startswith(entry + ": "), (entry, kw, msg)
    for entry in TRAJ:
        p = good(entry, dv, dc)
        rc, msg = call(entry, p, rows=None)
        assert rc == BAD_ARG and msg == entry + ": null d_rows"
        for cap in (0, -3):
            rc, msg = call(entry, p, rows_cap=cap)
            assert rc == BAD_ARG and msg == entry + ": d_rows given but rows_cap <= 0"
        # the fixed order — parameters, rows arguments, shape, buffers: the rows defect is reported before the shape's
        rc, msg = call(entry, P(3, 9, 50, 300, 900), rows_cap=0, a=None)
        assert rc == BAD_ARG and "rows_cap" in msg
        rc, msg = call(entry, P(3, 9, 50, 300, 900), a=None)
        assert rc == TOO_LARGE and "no instance" in msg


def test_the_older_entry_points_still_refuse_other_degrees():
    L = _lib.lib()
    p = E.make_params(3, 6, 50, 1000)
    assert L.scldpc_full_bp_device_sock16(C.byref(p), 0, None, None, None, 0, 1, None, None, None) == TOO_LARGE
    assert b"takes dv = 4, dc = 8" in L.scldpc_last_error()
    assert L.scldpc_full_bp_sock16_supported(C.byref(p)) == 0 and L.scldpc_full_bp_wide_supported(C.byref(p)) == 0


def _sim(dv, dc, L, N, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), device="cpu", **kw)


HEAD = "sampler (first generation) + cn_sockets pass + full_bp_small "
FIRST = "sampler (first generation) + full_bp (16-bit CN words"


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_simulator_takes_the_deg_path_where_it_applies(dv, dc, monkeypatch):
    pair = "4-bit CN counts, dv = %d, dc = %d" % (dv, dc)
    s = _sim(dv, dc, 50, 1000, deg=True, max_it=500)
    assert s.path == B.Path(torch.int16, "first", "sock", True, "deg16", None) and s.deg
    assert not (s.sock or s.gen2 or s.lvl2 or s.ring2 or s.wide or s.wide_sock)
    assert s.kernel_choice() == HEAD + "level-synchronous (" + pair + ")"
    s = _sim(dv, dc, 50, 1000, deg=True, rows_cap=64, doped=(3,))         # doped positions come with the channel
    assert s.path.decoder == "deg16" and s.kernel_choice() == HEAD + "level-synchronous (" + pair + ", trajectory rows)"
    s = _sim(dv, dc, 50, 5000, deg=True, rows_cap=4096)
    assert s.path == B.Path(torch.int16, "first", "sock", True, "degwide", None)
    assert s.kernel_choice() == HEAD + "wide level-synchronous (" + pair + ", 32-bit queue entries, trajectory rows)"
    assert _sim(dv, dc, 50, 5000, deg=True).kernel_choice() == HEAD + "wide level-synchronous (" + pair + ", 32-bit queue entries)"
    # an unlimited fixpoint run: the narrow fixpoint form; a wide shape keeps full_bp_fixpoint (rows: the wide level form)
    s = _sim(dv, dc, 50, 1000, deg=True, schedule="fixpoint")
    assert s.path == B.Path(torch.int16, "first", "sock", True, "deg16", "fixpoint_deg")
    assert s.kernel_choice() == HEAD + "fixpoint (" + pair + ")"
    s = _sim(dv, dc, 50, 5000, deg=True, schedule="fixpoint")
    assert s.path == B.Path(torch.int16, "first", None, False, "full_bp", "fixpoint") and not s.deg
    s = _sim(dv, dc, 50, 5000, deg=True, schedule="fixpoint", rows_cap=64)
    assert s.path == B.Path(torch.int16, "first", "sock", True, "degwide", "fixpoint")
    assert _sim(dv, dc, 50, 1000, deg=True, schedule="fixpoint", max_it=500).path.fix_decoder is None      # a cap to honour
    # off, or not applicable: the first-generation path and its line as they were
    old = _sim(dv, dc, 50, 1000, deg=False)
    assert old.path == B.Path(torch.int16, "first", None, False, "full_bp", None) and not old.deg
    assert old.kernel_choice().startswith(FIRST + "): the 4-bit decoders take dv = 4, dc = 8")
    for kw in (dict(deg=False), dict(deg=True, decoder="sw", W=10), dict(deg=True, L=50, N=7000)):
        kw = dict(kw)
        assert not _sim(dv, dc, kw.pop("L", 50), kw.pop("N", 1000), **kw).deg, kw
    s = _sim(dv, dc, 50, 1000, deg=True, rng="glibc")                     # glibc: the first generation on the int32 table
    assert not s.deg and s.path == B.Path(torch.int32, "glibc", None, False, "full_bp", None)
    assert s.kernel_choice().startswith("glibc replay on the host + full_bp (16-bit CN words)")
    assert _sim(dv, dc, 50, 1000).deg == B.DEG_BY_DEFAULT                 # deg=None follows the measured default
    monkeypatch.setattr(B, "DEG_BY_DEFAULT", True)
    assert _sim(dv, dc, 50, 1000).deg and _sim(dv, dc, 50, 5000).path.decoder == "degwide"
    assert not _sim(dv, dc, 50, 1000, deg=False).deg
    monkeypatch.setattr(E, "full_bp_deg_supported", lambda p, wide=False: False)                  # the library's rule decides
    assert not _sim(dv, dc, 50, 1000, deg=True).deg


def test_4_8_selection_does_not_look_at_deg():
    for L, N in ((50, 1000), (50, 5000), (100, 1000)):
        ref = SelectOnly(E.make_params(4, 8, L, N), device="cpu")
        for deg in (True, False):
            s = SelectOnly(E.make_params(4, 8, L, N), device="cpu", deg=deg)
            assert s.path == ref.path and not s.deg and s.kernel_choice() == ref.kernel_choice()


@pytest.mark.parametrize("dv,dc", [(3, 6), (5, 10)])
def test_caps_keep_their_sequential_passes(dv, dc):
    why = B.caps_sequential_reason(E.make_params(dv, dc, 50, 1000), "philox", 0, "flooding")
    assert why == "the level-synchronous 4-bit decoder takes dv = 4, dc = 8 and at most 65536 CNs per trial"
    for deg in (None, True, False):
        with pytest.raises(ValueError, match="caps: the fused decode takes Philox sampling"):
            _sim(dv, dc, 50, 1000, caps=[100, 200], deg=deg)


def test_cli_passes_the_deg_switch_through():
    for prog in ("bp_traj", "bp_lim_iter"):
        ap = B._parser(prog)
        base = ["0", "0", "0", "500"] + (["0"] if prog == "bp_traj" else [])
        assert ap.parse_args(base).deg == "auto"
        assert ap.parse_args(base + ["--deg", "off", "--dv", "3", "--dc", "6"]).deg == "off"
    with pytest.raises(SystemExit):
        B._parser("sw_lim_iter").parse_args(["0", "10", "0", "6", "60", "--deg", "on"])
