"""The classical ring window decoder on the CPU: the two symbols of sw_ring.hip's classical form, the shape rule behind
scldpc_swc_bp_ring_supported, the refusals of scldpc_swc_bp_ring_device decided before any device work (placeholder pointers
that are never dereferenced, as tests/test_small_refusals.py), the Simulator's choice of the path for decoder="swc" and the
--window / --ring switches of bp_lim_iter."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from fakes import FakeSimulator, SelectOnly
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

NEW = ("scldpc_swc_bp_ring_supported", "scldpc_swc_bp_ring_device")
ENTRY = "scldpc_swc_bp_ring_device"
ONE = C.c_void_p(16)                                                    # non-null placeholder
BAD_ARG, TOO_LARGE = -1, -2
P = _lib.CodeParams
PAIRS = [(3, 6), (4, 8), (5, 10)]

MANY_SOCKETS = P(3, 6, 2, 10923, 21846)                                 # vns_pos * dv = 65 538
LONG_CHAIN = P(3, 6, 65534, 2, 4)                                       # L + dv - 1 = 65 536 CN positions


def test_library_exports_and_header_declares_the_two_symbols():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert L.scldpc_abi_version() == 2                                   # additions only


# dv, dc, L, N, W: the shapes of the GPU tests and of tools/classical_ring_speedup.py among them
TAKEN = [(4, 8, 100, 2000, 10), (3, 6, 50, 1000, 20), (5, 10, 50, 1000, 20), (4, 8, 50, 1000, 20), (3, 6, 9, 24, 20),
         (3, 6, 9, 24, 1), (5, 10, 12, 40, 3), (3, 6, 12, 6000, 10), (4, 8, 12, 6000, 10), (5, 10, 12, 6000, 10)]


@pytest.mark.parametrize("dv,dc,L,N,W", TAKEN)
def test_the_predicate_takes_the_three_pairs(dv, dc, L, N, W):
    p = E.make_params(dv, dc, L, N)
    assert E.swc_ring_supported(p, W) and _lib.lib().scldpc_swc_bp_ring_supported(C.byref(p), W) == 1
    # the existing predicates answer as before
    assert E.sw_ring_deg_supported(p, W) and E.sw_ring_supported(p, W) == ((dv, dc) == (4, 8))


def test_the_predicate_refuses_what_the_kernel_cannot_hold():
    fn = _lib.lib().scldpc_swc_bp_ring_supported
    for p, W in ((P(4, 6, 50, 1000, 1500), 10), (P(3, 7, 50, 300, 700), 10), (P(6, 12, 50, 500, 1000), 10),
                 (E.make_params(4, 8, 50, 1000), 0), (E.make_params(5, 10, 50, 1000), -1), (MANY_SOCKETS, 1), (LONG_CHAIN, 1),
                 (E.make_params(4, 8, 50, 1000), 10 ** 6), (E.make_params(3, 6, 50, 1000), 2 ** 31 - 1),
                 (E.make_params(4, 8, 400, 5000), 300),
                 (P(3, 6, 50, 500, 999), 10)):                           # invalid parameters
        assert fn(C.byref(p), W) == 0, (p.key(), W)
    assert fn(C.byref(P(3, 6, 2, 10922, 21844)), 1) == 1                 # 65 532 sockets
    assert fn(None, 10) == 0


def _state_bytes(p, W, classical):
    """The window's state as the predicates sum it (sw_ring.hip), without the queues."""
    Cw, wpp = (p.cns_pos + 7) // 8, (p.vns_pos + 31) // 32
    R, RV = (W + 3 * p.dv - 2, W + 2 * p.dv - 1) if classical else (W + 2 * p.dv - 1, W + p.dv)
    return 4 * (R * Cw + RV * wpp + (W * Cw + 3) // 4 + 2 * p.L)


def test_the_classical_ring_takes_no_more_than_the_square_ring():
    """The classical state is the square state plus dv - 1 positions of counts and of S bits: over a sweep of shapes the
    classical predicate implies the square one, and near the LDS limit the square ring takes shapes the classical refuses."""
    only_square = taken = 0
    for dv, dc in PAIRS:
        for L, N in ((9, 6 * dc), (50, 1000), (100, 2000), (12, 6000), (400, 5000), (20, 20000)):
            p = E.make_params(dv, dc, L, N)
            for W in (1, 3, 10, 20, 40, 50, 60, 62, 64, 66, 68, 80, 100, 125, 130, 150, 200, 250, 300, 1000):   # 62 .. 66: the limit at N = 5000
                c, s = E.swc_ring_supported(p, W), E.sw_ring_deg_supported(p, W)
                assert s or not c, (dv, dc, L, N, W)
                taken += c
                only_square += s and not c
                if s and not c:                                          # the reason is the size of the state
                    assert _state_bytes(p, W, False) <= 160 * 1024 < _state_bytes(p, W, True) + 2 * 4 * 512 + 256
    assert taken > 50 and only_square > 0, (taken, only_square)


def call(p, W=10, ntrials=1, a=ONE, cn=ONE, ch=ONE, cnt=ONE, max_it=5):
    fn = getattr(_lib.lib(), ENTRY)
    rc = fn(C.byref(p) if p is not None else None, ntrials, a, cn, ch, W, max_it, cnt, None, None)
    return rc, _lib.lib().scldpc_last_error().decode()


# (defect, parameters, W, return code, part of the message)
REFUSALS = [
    ("dc beyond a nibble", P(4, 16, 50, 250, 1000), 10, TOO_LARGE, "dc must be at most 15"),
    ("pair without an instance", P(4, 6, 50, 1000, 1500), 10, TOO_LARGE, "no instance for dv = 4, dc = 6"),
    ("pair without an instance", P(6, 12, 50, 500, 1000), 10, TOO_LARGE, "no instance for dv = 6, dc = 12"),
    ("too many sockets", MANY_SOCKETS, 1, TOO_LARGE, "sockets: vns_pos * dv must fit 16 bits (at most 65535)"),
    ("too many CN positions", LONG_CHAIN, 1, TOO_LARGE, "queue: L + dv - 1 CN positions must fit 16 bits (at most 65535)"),
    ("window beyond the LDS", E.make_params(4, 8, 50, 1000), 10 ** 6, TOO_LARGE,
     "LDS: the window's CN counts, S bits and queues exceed 160 KiB"),
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


@pytest.mark.parametrize("dv,dc", PAIRS)
def test_argument_checks_come_before_any_launch(dv, dc):
    p = E.make_params(dv, dc, 50, 1000)
    assert call(p, ntrials=0, a=None, cn=None, ch=None, cnt=None)[0] == 0                         # empty batch, null buffers
    rc, msg = call(p, ntrials=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials"
    for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(cnt=None)):
        rc, msg = call(p, **kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer or negative ntrials", (kw, msg)
    rc, msg = call(p, max_it=-1)
    assert rc == BAD_ARG and msg == ENTRY + ": need W >= 1, max_it >= 0"


def _sim(dv, dc, L=50, N=1000, W=20, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), decoder="swc", W=W, max_it=6, device="cpu", **kw)


RING = " + sw_ring classical window (window state in LDS, dv = %d, dc = %d)"
CHAIN = "sampler (first generation) + sw_bp classical window (whole chain)"


@pytest.mark.parametrize("dv,dc", PAIRS)
def test_simulator_takes_the_ring_path_where_it_applies(dv, dc, monkeypatch):
    chain = B.Path(torch.int16, "first", None, False, "swc_chain", None)
    for L, N, W in ((50, 1000, 20), (100, 2000, 10), (9, 6 * dc, 20), (12, 6000, 10)):
        s = _sim(dv, dc, L, N, W, ring=True)
        if E.sock16_supported(s.p):                                      # the socket table is sampled with the code
            assert (dv, dc) == (4, 8) and s.path == B.Path(torch.int16, "sock16", "sock", False, "swc_ring", None)
            assert s.kernel_choice() == "sampler_v3 (CN->socket table)" + RING % (dv, dc)
        else:
            assert s.path == B.Path(torch.int16, "first", "sock", True, "swc_ring", None)
            assert s.kernel_choice() == "sampler (first generation) + cn_sockets pass" + RING % (dv, dc)
        assert not (s.sock or s.gen2 or s.lvl2 or s.wide or s.wide_sock or s.deg or s.ring2 or s.ring_deg)
        old = _sim(dv, dc, L, N, W, ring=False)
        assert old.path == chain and old.kernel_choice() == CHAIN
    assert E.sock16_supported(E.make_params(4, 8, 50, 1000)) and not E.sock16_supported(E.make_params(4, 8, 12, 6000))
    # ring=None follows the measured default
    assert (_sim(dv, dc).path.decoder == "swc_ring") == B.CLASSICAL_RING_BY_DEFAULT
    monkeypatch.setattr(B, "CLASSICAL_RING_BY_DEFAULT", True)
    assert _sim(dv, dc).path.decoder == "swc_ring" and _sim(dv, dc, ring=False).path == chain
    monkeypatch.setattr(B, "CLASSICAL_RING_BY_DEFAULT", False)
    assert _sim(dv, dc).path == chain and _sim(dv, dc, ring=True).path.decoder == "swc_ring"
    # not applicable: glibc sampling (the int32 table), a window the predicate refuses
    s = _sim(dv, dc, ring=True, rng="glibc")
    assert s.path == B.Path(torch.int32, "glibc", None, False, "swc_chain", None)
    assert s.kernel_choice() == "glibc replay on the host + sw_bp classical window (whole chain)"
    assert _sim(dv, dc, 400, 5000, 300, ring=True).path == chain and _sim(dv, dc, W=0, ring=True).path == chain
    monkeypatch.setattr(E, "swc_ring_supported", lambda p, W: False)     # the library's rule decides
    assert _sim(dv, dc, ring=True).path == chain


def test_classical_ring_reason_says_why():
    p = E.make_params(3, 6, 50, 1000)
    assert B.classical_ring_reason(p, 20, "philox") is None
    assert B.classical_ring_reason(E.make_params(4, 8, 100, 2000), 10, "philox") is None
    assert "--rng glibc" in B.classical_ring_reason(p, 20, "glibc")
    assert "W = 0" in B.classical_ring_reason(p, 0, "philox")
    assert "fits the LDS" in B.classical_ring_reason(E.make_params(5, 10, 400, 5000), 300, "philox")
    assert B.classical_ring_reason(p, 20, "philox", want=False) == "switched off"
    assert (B.classical_ring_reason(p, 20, "philox", want=None) is None) == B.CLASSICAL_RING_BY_DEFAULT


def test_cli_has_the_window_switch_on_bp_lim_iter_only():
    ap = B._parser("bp_lim_iter")
    base = ["0", "6", "0", "5"]
    assert ap.parse_args(base).window == "off" and ap.parse_args(base).ring == "auto"
    for mode in ("auto", "on", "off"):
        assert ap.parse_args(base + ["--window", "classical", "--ring", mode]).ring == mode
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--window", "square"])
    for prog, more in (("sw_lim_iter", ["10"]), ("bp_traj", ["0"])):
        with pytest.raises(SystemExit):
            B._parser(prog).parse_args(base + more + ["--window", "classical"])


# every refusal is raised where the command line is read and again by the program, before the Simulator exists
REFUSED = [(["--window", "classical", "--caps", "3,4"], "--window classical: --caps"),
           (["--window", "classical", "--schedule", "fixpoint"], "--window classical: --schedule fixpoint"),
           (["--ring", "on"], "--ring on: needs --window classical"),
           (["--ring", "on", "--caps", "3,4"], "--ring on: needs --window classical")]


@pytest.mark.parametrize("extra,why", REFUSED)
def test_combinations_that_cannot_run_exit_with_their_reason(tmp_path, monkeypatch, extra, why):
    monkeypatch.setattr(B, "Simulator", None)                            # never reached
    argv = ["0", "6", "0", "5", "--seed", "1", "--quiet", "--outdir", str(tmp_path)] + extra
    with pytest.raises(SystemExit) as e:
        B.bp_lim_iter(argv)
    assert str(e.value.code).startswith(why), e.value.code
    with pytest.raises(SystemExit) as e:
        B._parser("bp_lim_iter").parse_args(argv)
    assert str(e.value.code).startswith(why)
    opts = argparse_namespace(argv)
    with pytest.raises(SystemExit) as e:
        B.run_program("bp_lim_iter", 0, 6, 0, 5, None, opts)
    assert str(e.value.code).startswith(why)
    assert os.listdir(tmp_path) == []


def argparse_namespace(argv):
    """The options of argv as the plain parser reads them (without the checks of bp_lim_iter's own parser)."""
    import argparse
    ap = B._parser("bp_lim_iter")
    opts = argparse.ArgumentParser.parse_args(ap, argv)
    opts.seed = 1
    return opts


@pytest.mark.parametrize("extra,why", [(["--rng", "glibc"], "--rng glibc"),
                                       (["--dv", "5", "--dc", "10", "--L", "400", "--N", "5000"], "fits the LDS"),
                                       (["--dv", "4", "--dc", "6", "--N", "1500"], "the pairs (3,6), (4,8) and (5,10)")])
def test_ring_on_where_the_ring_does_not_apply_is_an_error_that_says_why(tmp_path, monkeypatch, extra, why):
    monkeypatch.setattr(B, "Simulator", None)
    argv = ["0", "300", "0", "5", "--window", "classical", "--seed", "1", "--quiet", "--outdir", str(tmp_path), "--ring", "on"]
    with pytest.raises(SystemExit) as e:
        B.bp_lim_iter(argv + extra)
    assert str(e.value.code).startswith("--ring on: ") and why in str(e.value.code)
    assert os.listdir(tmp_path) == []


class Recorded(Exception):
    pass


def _constructed(monkeypatch, argv):
    """The arguments with which bp_lim_iter constructs its Simulator."""
    def record(p, **kw):
        raise Recorded((p.key(), kw))
    monkeypatch.setattr(B, "Simulator", record)
    with pytest.raises(Recorded) as e:
        B.bp_lim_iter(argv + ["--seed", "1", "--quiet"])
    return e.value.args[0]


def test_window_classical_constructs_the_classical_simulator(monkeypatch, tmp_path):
    base = ["0", "6", "0", "0", "--dv", "3", "--dc", "6", "--L", "20", "--N", "200", "--outdir", str(tmp_path)]
    for mode, ring in (("auto", None), ("on", True), ("off", False)):
        key, kw = _constructed(monkeypatch, base + ["--window", "classical", "--ring", mode])
        assert key == E.make_params(3, 6, 20, 200).key()
        assert (kw["decoder"], kw["W"], kw["max_it"], kw["init_it"], kw["ring"]) == ("swc", 6, 1, 0, ring)     # MAX_IT: at least 1
    # without --window: full BP, as before, whatever --ring off / auto says
    for extra in ([], ["--ring", "off"], ["--window", "off"]):
        key, kw = _constructed(monkeypatch, base + extra)
        assert (kw["decoder"], kw["ring"], kw["max_it"]) == ("full", None, 1)


def test_bp_lim_iter_without_window_selects_the_path_of_full_bp():
    """decoder="full" does not look at ring: the paths the parent commit selects for these shapes."""
    I16 = torch.int16
    for dv, dc, L, N, want in ((4, 8, 50, 1000, B.Path(I16, "cn16", "vn", False, "level16", None)),
                               (3, 6, 50, 1000, B.Path(I16, "first", None, False, "full_bp", None)),
                               (5, 10, 50, 1000, B.Path(I16, "first", None, False, "full_bp", None)),
                               (4, 8, 100, 2000, B.Path(I16, "sock16", "sock", False, "wide", None)),
                               (4, 8, 50, 5000, B.Path(I16, "first", "sock", True, "wide", None)),
                               (4, 8, 100, 5000, B.Path(I16, "first", None, False, "full_bp", None))):
        for ring in (None, True, False):
            s = SelectOnly(E.make_params(dv, dc, L, N), decoder="full", max_it=500, device="cpu", ring=ring)
            assert s.path == want, (dv, dc, L, N, ring, s.path)
            assert "classical" not in s.kernel_choice()


def test_the_classical_file_is_bp_lim_iters_own(tmp_path, monkeypatch):
    """The whole program on the fake device: the file name of BPF:487 with W in it, the usual rows."""
    monkeypatch.setattr(B, "Simulator", FakeSimulator)
    B.bp_lim_iter(["0", "6", "0", "5", "--window", "classical", "--dv", "3", "--dc", "6", "--L", "20", "--N", "200", "--num-points",
                   "2", "--max-frames", "16", "--min-frame-err", "16", "--batch", "8", "--seed", "5", "--quiet", "--outdir",
                   str(tmp_path)])
    assert os.listdir(tmp_path) == ["SC_LDPC_3_6_L20_M100_BP_SW6_5it_Random_BLER_0.dat"]
    lines = open(tmp_path / os.listdir(tmp_path)[0]).read().split("\n")
    assert lines[0] + "\n" == B.RISULTATI_HEADER and len(lines) == 4 and len(lines[1].split()) == 16
