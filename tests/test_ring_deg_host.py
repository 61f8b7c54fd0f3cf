"""The ring window decoder for the degree pairs (3,6) and (5,10) on the CPU: the two _deg symbols of sw_ring.hip, the shape
rule behind scldpc_sw_bp_ring_deg_supported, the refusals of scldpc_sw_bp_ring_device_deg decided before any device work
(placeholder pointers that are never dereferenced, as tests/test_small_refusals.py), the Simulator's choice of the path and the
--ring switch of sw_lim_iter."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from fakes import SelectOnly
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

NEW = ("scldpc_sw_bp_ring_deg_supported", "scldpc_sw_bp_ring_device_deg")
ENTRY = "scldpc_sw_bp_ring_device_deg"
ONE = C.c_void_p(16)                                                    # non-null placeholder
BAD_ARG, TOO_LARGE = -1, -2
P = _lib.CodeParams
PAIRS = [(3, 6), (5, 10)]

MANY_SOCKETS = P(3, 6, 2, 10923, 21846)                                 # vns_pos * dv = 65 538
LONG_CHAIN = P(3, 6, 65534, 2, 4)                                       # L + dv - 1 = 65 536 CN positions
BIG_WINDOW = (E.make_params(4, 8, 400, 5000), 300)                      # 307 slots of 313 count words: 384 KB


def test_library_exports_and_header_declares_the_two_symbols():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert L.scldpc_abi_version() == 2                                   # additions only


# dv, dc, L, N, W: the shapes of the GPU tests and of tools/ring_deg_speedup.py among them
TAKEN = [(3, 6, 50, 1000, 20), (5, 10, 50, 1000, 20), (4, 8, 50, 1000, 20), (3, 6, 100, 2000, 10), (5, 10, 100, 2000, 10),
         (4, 8, 100, 2000, 10), (3, 6, 9, 24, 20), (3, 6, 9, 24, 1), (5, 10, 12, 40, 3), (3, 6, 12, 6000, 10), (5, 10, 12, 6000, 10)]


@pytest.mark.parametrize("dv,dc,L,N,W", TAKEN)
def test_the_predicate_takes_the_three_pairs(dv, dc, L, N, W):
    p = E.make_params(dv, dc, L, N)
    assert E.sw_ring_deg_supported(p, W)
    # the existing predicate answers as before: (4,8) only
    assert E.sw_ring_supported(p, W) == ((dv, dc) == (4, 8))
    assert _lib.lib().scldpc_sw_bp_ring_supported(C.byref(p), W) == int((dv, dc) == (4, 8))


def test_the_predicate_refuses_what_the_kernel_cannot_hold():
    fn = _lib.lib().scldpc_sw_bp_ring_deg_supported
    for p, W in ((P(3, 7, 50, 300, 700), 10), (P(6, 12, 50, 500, 1000), 10), (P(4, 16, 50, 250, 1000), 10),
                 (E.make_params(3, 6, 50, 1000), 0), (E.make_params(5, 10, 50, 1000), -1), (MANY_SOCKETS, 1), (LONG_CHAIN, 1),
                 BIG_WINDOW, (E.make_params(3, 6, 400, 5000), 300), (E.make_params(5, 10, 400, 5000), 300),
                 (E.make_params(3, 6, 50, 1000), 2 ** 31 - 1),
                 (P(3, 6, 50, 500, 999), 10)):                           # invalid parameters
        assert fn(C.byref(p), W) == 0, (p.key(), W)
    assert fn(C.byref(P(3, 6, 2, 10922, 21844)), 1) == 1                 # 65 532 sockets
    assert fn(None, 10) == 0


def call(p, W=10, ntrials=1, a=ONE, cn=ONE, ch=ONE, cnt=ONE, max_it=5, init_it=0):
    fn = getattr(_lib.lib(), ENTRY)
    rc = fn(C.byref(p) if p is not None else None, ntrials, a, cn, ch, W, max_it, init_it, cnt, None, None)
    return rc, _lib.lib().scldpc_last_error().decode()


# (defect, parameters, W, return code, part of the message)
REFUSALS = [
    ("dc beyond a nibble", P(4, 16, 50, 250, 1000), 10, TOO_LARGE, "dc must be at most 15"),
    ("pair without an instance", P(3, 7, 50, 300, 700), 10, TOO_LARGE, "no instance for dv = 3, dc = 7"),
    ("pair without an instance", P(6, 12, 50, 500, 1000), 10, TOO_LARGE, "no instance for dv = 6, dc = 12"),
    ("too many sockets", MANY_SOCKETS, 1, TOO_LARGE, "sockets: vns_pos * dv must fit 16 bits (at most 65535)"),
    ("too many CN positions", LONG_CHAIN, 1, TOO_LARGE, "queue: L + dv - 1 CN positions must fit 16 bits (at most 65535)"),
    ("window beyond the LDS", BIG_WINDOW[0], BIG_WINDOW[1], TOO_LARGE, "LDS: the window's CN counts, S bits and queues exceed 160 KiB"),
    ("window beyond the LDS", E.make_params(5, 10, 400, 5000), 300, TOO_LARGE, "exceed 160 KiB"),
    ("W = 0", E.make_params(3, 6, 50, 1000), 0, BAD_ARG, "need W >= 1"),
    ("invalid parameters", P(3, 6, 50, 500, 999), 10, BAD_ARG, "dv*vns_pos (3*999) must equal dc*cns_pos (6*500)"),
    ("null parameters", None, 10, BAD_ARG, "null scldpc_code_params"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0].replace(" ", "_"))
def test_refusal_names_the_limit_and_the_entry_point(case):
    defect, p, W, want_rc, part = case
    for ntrials in (1, 0):                                               # the shape is judged even for an empty batch
        rc, msg = call(p, W, ntrials=ntrials)
        assert rc == want_rc and part in msg, (defect, rc, msg)
        assert msg.startswith(ENTRY + ": ") or defect in ("invalid parameters", "null parameters"), msg


@pytest.mark.parametrize("dv,dc", PAIRS + [(4, 8)])
def test_argument_checks_come_before_any_launch(dv, dc):
    p = E.make_params(dv, dc, 50, 1000)
    assert call(p, ntrials=0, a=None, cn=None, ch=None, cnt=None)[0] == 0                         # empty batch, null buffers
    rc, msg = call(p, ntrials=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials"
    for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(cnt=None)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials", (kw, msg)
    for kw in (dict(max_it=-1), dict(init_it=-1)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": need W >= 1, max_it >= 0, init_it >= 0", (kw, msg)


@pytest.mark.parametrize("dv,dc", PAIRS)
def test_the_older_entry_point_still_refuses_other_degrees(dv, dc):
    L = _lib.lib()
    p = E.make_params(dv, dc, 50, 1000)
    for ntrials in (1, 0):
        assert L.scldpc_sw_bp_ring_device(C.byref(p), ntrials, ONE, ONE, ONE, 10, 5, 0, ONE, None, None) == TOO_LARGE
        assert b"scldpc_sw_bp_ring_device: takes dv = 4, dc = 8" in L.scldpc_last_error()


def _sim(dv, dc, L=50, N=1000, W=20, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), decoder="sw", W=W, max_it=6, init_it=60, device="cpu", **kw)


RING = "sampler (first generation) + cn_sockets pass + sw_ring (window state in LDS, dv = %d, dc = %d)"
CHAIN = "sampler (first generation) + sw_bp (whole chain)"


@pytest.mark.parametrize("dv,dc", PAIRS)
def test_simulator_takes_the_ring_path_where_it_applies(dv, dc, monkeypatch):
    chain = B.Path(torch.int16, "first", None, False, "sw_chain", None)
    for L, N, W in ((50, 1000, 20), (100, 2000, 10), (9, 6 * dc, 20)):
        s = _sim(dv, dc, L, N, W, ring=True)
        assert s.path == B.Path(torch.int16, "first", "sock", True, "sw_ring", None) and s.ring_deg
        assert s.kernel_choice() == RING % (dv, dc)
        assert not (s.sock or s.gen2 or s.lvl2 or s.wide or s.wide_sock or s.deg)
        old = _sim(dv, dc, L, N, W, ring=False)                          # today's path and its line
        assert old.path == chain and not old.ring_deg and not old.ring2 and old.kernel_choice() == CHAIN
    # ring=None follows the measured default
    assert _sim(dv, dc).ring_deg == B.RING_DEG_BY_DEFAULT
    monkeypatch.setattr(B, "RING_DEG_BY_DEFAULT", True)
    assert _sim(dv, dc).ring_deg and _sim(dv, dc).kernel_choice() == RING % (dv, dc)
    assert not _sim(dv, dc, ring=False).ring_deg
    monkeypatch.setattr(B, "RING_DEG_BY_DEFAULT", False)
    assert _sim(dv, dc).path == chain and _sim(dv, dc, ring=True).ring_deg
    # not applicable: glibc sampling (the int32 table), a window the predicate refuses
    s = _sim(dv, dc, ring=True, rng="glibc")
    assert s.path == B.Path(torch.int32, "glibc", None, False, "sw_chain", None) and s.kernel_choice() == CHAIN
    assert not E.sw_ring_deg_supported(E.make_params(dv, dc, 400, 5000), 300)
    assert _sim(dv, dc, 400, 5000, 300, ring=True).path == chain
    assert _sim(dv, dc, W=0, ring=True).path == chain
    # deg= belongs to full BP: it neither switches the ring path on nor off
    assert _sim(dv, dc, deg=True).path == chain and not _sim(dv, dc, deg=True).deg
    assert _sim(dv, dc, deg=False, ring=True).ring_deg
    # full BP does not look at ring
    for ring in (True, False):
        s = SelectOnly(E.make_params(dv, dc, 50, 1000), decoder="full", device="cpu", ring=ring)
        assert s.path == B.Path(torch.int16, "first", None, False, "full_bp", None) and not s.ring_deg
    monkeypatch.setattr(E, "sw_ring_deg_supported", lambda p, W: False)  # the library's rule decides
    assert _sim(dv, dc, ring=True).path == chain


def test_4_8_selection_does_not_look_at_ring():
    for L, N, W in ((50, 1000, 20), (100, 2000, 10), (50, 2474, 10), (50, 1000, 400)):
        ref = _sim(4, 8, L, N, W)
        for ring in (True, False):
            s = _sim(4, 8, L, N, W, ring=ring)
            assert s.path == ref.path and not s.ring_deg and s.kernel_choice() == ref.kernel_choice()
    assert _sim(4, 8, 50, 2474, 10).kernel_choice() == "sampler (first generation) + sw_ring + cn_sockets pass"


def test_ring_deg_reason_says_why():
    p = E.make_params(3, 6, 50, 1000)
    assert B.ring_deg_reason(p, 20, "philox") is None
    assert "--rng glibc" in B.ring_deg_reason(p, 20, "glibc")
    assert "W = 0" in B.ring_deg_reason(p, 0, "philox")
    assert "fits the LDS" in B.ring_deg_reason(E.make_params(5, 10, 400, 5000), 300, "philox")
    assert "dv = 4, dc = 8" in B.ring_deg_reason(E.make_params(4, 8, 50, 1000), 20, "philox")
    assert B.ring_deg_reason(p, 20, "philox", want=False) == "switched off"


def test_cli_has_the_ring_switch_on_sw_lim_iter_only():
    ap = B._parser("sw_lim_iter")
    base = ["0", "6", "0", "5", "10"]
    assert ap.parse_args(base).ring == "auto"
    for mode in ("auto", "on", "off"):
        assert ap.parse_args(base + ["--dv", "3", "--dc", "6", "--ring", mode]).ring == mode
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--ring", "maybe"])
    for prog in ("bp_lim_iter", "bp_traj"):
        with pytest.raises(SystemExit):
            B._parser(prog).parse_args(["0", "0", "0", "500"] + (["0"] if prog == "bp_traj" else []) + ["--ring", "on"])


@pytest.mark.parametrize("extra,why", [(["--dv", "3", "--dc", "6", "--rng", "glibc"], "--rng glibc"),
                                       (["--dv", "5", "--dc", "10", "--L", "400", "--N", "5000"], "fits the LDS"),
                                       ([], "dv = 4, dc = 8")])
def test_ring_on_where_the_path_does_not_apply_is_an_error_that_says_why(tmp_path, extra, why):
    """Raised before the Simulator (and any device buffer) exists."""
    argv = ["0", "300", "0", "5", "10", "--seed", "1", "--quiet", "--outdir", str(tmp_path), "--ring", "on"] + extra
    with pytest.raises(SystemExit) as e:
        B.sw_lim_iter(argv)
    assert str(e.value.code).startswith("--ring on: ") and why in str(e.value.code)
    assert os.listdir(tmp_path) == []
