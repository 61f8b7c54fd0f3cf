"""Several iteration caps from one decode for the wide form and the pairs (3,6) and (5,10), on the CPU: the three caps symbols,
their refusals decided before any device work (placeholder pointers that are never dereferenced, as tests/test_small_refusals.py),
the Simulator's opt-in choice of the fused path, caps_sequential_reason with and without the new arguments, and the
`--caps-fused` switch of bp_lim_iter with the device work faked (tests/test_caps_host.py's CapsFake)."""
import ctypes as C
import os
import re

import pytest
import torch

from fakes import SelectOnly
from test_caps_host import CapsFake

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

WIDE, DEG, DEG_WIDE = ("scldpc_full_bp_caps_device_wide", "scldpc_full_bp_caps_device_deg",
                       "scldpc_full_bp_caps_device_deg_wide")
ALL = (WIDE, DEG, DEG_WIDE)
ONE = C.c_void_p(16)                                                    # non-null placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
P = _lib.CodeParams
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scldpc.h")


def good(entry, dv=None, dc=None):
    """A shape the entry point takes (the _deg forms: (3,6) unless told otherwise)."""
    if entry == WIDE:
        return E.make_params(4, 8, 50, 5000)
    return E.make_params(dv or 3, dc or 6, 50, 5000 if entry == DEG_WIDE else 1000)


def call(entry, p, caps=(3, 5), ncaps=None, ntrials=1, a=ONE, cn=ONE, ch=ONE, cnt=ONE):
    arr = (C.c_int32 * max(1, len(caps)))(*caps) if caps is not None else None
    n = (len(caps) if caps is not None else 0) if ncaps is None else ncaps
    rc = getattr(_lib.lib(), entry)(C.byref(p), ntrials, a, cn, ch, n, arr, 1, cnt, None)
    return rc, _lib.lib().scldpc_last_error().decode()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_listed_and_exported():
    header = open(HEADER).read()
    L = _lib.lib()
    for name in ALL:
        assert re.search(r"\bint %s\(const scldpc_code_params \*p, int32_t ntrials," % name, header), name
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes == L.scldpc_full_bp_caps_device_sock16.argtypes
    assert L.scldpc_abi_version() == 2                                   # additions only


@pytest.mark.parametrize("entry", ALL)
def test_caps_list_refusals(entry):
    p = good(entry)
    for caps, ncaps, part in (((), 0, "takes 1 .. 16 caps (ncaps = 0)"),
                              (tuple(range(1, 18)), None, "takes 1 .. 16 caps (ncaps = 17)"),
                              (None, 2, "takes 1 .. 16 caps (ncaps = 2, caps NULL)"),
                              ((5, 3), None, "caps must be strictly increasing and >= 1 (caps[1] = 3)"),
                              ((3, 3), None, "caps must be strictly increasing and >= 1 (caps[1] = 3)"),
                              ((0, 3), None, "caps must be strictly increasing and >= 1 (caps[0] = 0)")):
        for ntrials in (1, 0):                                           # the caps list is judged even for an empty batch
            rc, msg = call(entry, p, caps=caps, ncaps=ncaps, ntrials=ntrials)
            assert rc == BAD_ARG and msg == entry + ": " + part, (caps, ncaps, rc, msg)
    assert call(entry, p, caps=tuple(range(1, 17)), ntrials=0)[0] == OK  # 16 caps
    assert call(entry, p, caps=(1000000,), ntrials=0)[0] == OK


# (defect, entry points, parameters, part of the message)
SHAPE_REFUSALS = [
    ("pair without an instance", (DEG, DEG_WIDE), P(4, 6, 50, 1000, 1500), "no instance for dv = 4, dc = 6"),
    ("dc beyond a nibble", (DEG, DEG_WIDE), P(4, 16, 50, 250, 1000), "dc must be at most 15"),
    ("dc beyond a nibble or another pair", (WIDE,), P(4, 16, 50, 250, 1000), "takes dv = 4, dc = 8 only"),
    ("another pair through the (4,8) form", (WIDE,), E.make_params(3, 6, 50, 5000), "takes dv = 4, dc = 8 only"),
    ("too many CNs for 16-bit queue entries", (DEG,), E.make_params(3, 6, 50, 5000), "at most 65536 CNs per trial"),
    ("short queues", (WIDE, DEG_WIDE), E.make_params(4, 8, 50, 7000), "queue: the LDS left by the state holds fewer than 1024"),
    ("state beyond the LDS", (WIDE, DEG_WIDE), E.make_params(4, 8, 50, 10000), "LDS: the CN counts and VN bits of a trial exceed"),
    ("short queues", (DEG_WIDE,), E.make_params(3, 6, 50, 7000), "queue: the LDS left by the state holds fewer than 1024"),
]


@pytest.mark.parametrize("case", SHAPE_REFUSALS, ids=lambda c: c[0].replace(" ", "_"))
def test_shape_refusals_name_the_limit_and_the_entry_point(case):
    defect, entries, p, part = case
    for entry in entries:
        for ntrials in (1, 0):                                           # the shape is judged even for an empty batch
            rc, msg = call(entry, p, ntrials=ntrials)
            assert rc == TOO_LARGE and part in msg and msg.startswith(entry + ": "), (defect, entry, rc, msg)


def test_a_caps_form_takes_the_shapes_of_its_level_form():
    """No predicate of its own: an empty batch is accepted exactly where the family's *_supported says so."""
    shapes = [(dv, dc, L, N) for dv, dc in ((3, 6), (4, 8), (5, 10))
              for L, N in ((50, 1000), (50, 2500), (50, 5000), (50, 6000), (50, 7000), (16, 200), (9, 24 if dv == 3 else 40))]
    for dv, dc, L, N in shapes:
        p = E.make_params(dv, dc, L, N)
        assert (call(DEG, p, ntrials=0)[0] == OK) == E.full_bp_deg_supported(p), (dv, dc, L, N)
        assert (call(DEG_WIDE, p, ntrials=0)[0] == OK) == E.full_bp_deg_supported(p, wide=True), (dv, dc, L, N)
        assert (call(WIDE, p, ntrials=0)[0] == OK) == E.full_bp_wide_supported(p), (dv, dc, L, N)


@pytest.mark.parametrize("entry", ALL)
def test_buffers_are_checked_last(entry):
    for p in [good(entry)] + ([good(entry, 5, 10), good(entry, 4, 8)] if entry != WIDE else []):
        assert call(entry, p, ntrials=0, a=None, cn=None, ch=None, cnt=None) == (OK, call(entry, p, ntrials=0)[1])
        rc, msg = call(entry, p, ntrials=-1)
        assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials"
        for kw in (dict(a=None), dict(cn=None), dict(ch=None), dict(cnt=None)):
            rc, msg = call(entry, p, **kw)
            assert rc == BAD_ARG and msg == entry + ": null buffer or negative ntrials", (entry, kw, msg)
    # the fixed order — parameters, caps list, shape, buffers
    bad_shape = E.make_params(4, 8, 50, 10000)
    rc, msg = call(entry, bad_shape, caps=(5, 3), a=None)
    assert rc == BAD_ARG and "strictly increasing" in msg                # a bad caps list and a bad shape: the caps list
    rc, msg = call(entry, bad_shape, a=None)
    assert rc == TOO_LARGE and ("65536 CNs per trial" if entry == DEG else "LDS") in msg      # … and a null buffer: the shape
    rc, msg = call(entry, P(3, 6, 50, 500, 999), caps=(5, 3))
    assert rc == BAD_ARG and "must equal" in msg                         # invalid parameters come first


# ---- the Simulator's choice ------------------------------------------------------------------------------------------------
def _sim(dv, dc, L, N, **kw):
    return SelectOnly(E.make_params(dv, dc, L, N), device="cpu", **kw)


CAPS5 = [175, 200, 250, 300, 350]
TODAY = "caps: the fused decode takes Philox sampling, no doping and an ensemble of the level-synchronous 4-bit decoder"


def test_the_constant_stays_off():
    assert B.CAPS_FORMS_BY_DEFAULT is False


def test_fused_caps_selects_the_paths_of_the_single_cap_runs():
    first = "sampler (first generation) + cn_sockets pass + full_bp_small "
    s = _sim(4, 8, 50, 5000, caps=CAPS5, fused_caps=True)
    assert s.path == B.Path(torch.int16, "first", "sock", True, "wide", None) and s.wide and not s.wide_sock and not s.lvl2
    assert s.path == _sim(4, 8, 50, 5000, max_it=350).path               # the path of the single-cap run
    assert s.max_it == 350
    assert s.kernel_choice() == first + ("wide level-synchronous with 5 cap checkpoints per decode (4-bit CN counts, "
                                         "32-bit queue entries)")
    s = _sim(4, 8, 100, 2000, caps=CAPS5, fused_caps=True)               # 8000 sockets per position: sampled with the code
    assert s.path == B.Path(torch.int16, "sock16", "sock", False, "wide", None) and s.wide_sock
    assert s.kernel_choice() == ("sampler_v3 (CN->socket table) + full_bp_small wide level-synchronous with 5 cap checkpoints "
                                 "per decode (4-bit CN counts, 32-bit queue entries)")
    s = _sim(3, 6, 50, 1000, caps=CAPS5, fused_caps=True)
    assert s.path == B.Path(torch.int16, "first", "sock", True, "deg16", None) and s.deg
    assert s.path == _sim(3, 6, 50, 1000, max_it=350, deg=True).path
    assert s.kernel_choice() == first + "level-synchronous with 5 cap checkpoints per decode (4-bit CN counts, dv = 3, dc = 6)"
    s = _sim(5, 10, 50, 5000, caps=CAPS5[:3], fused_caps=True, deg=True)
    assert s.path == B.Path(torch.int16, "first", "sock", True, "degwide", None) and s.deg
    assert s.kernel_choice() == first + ("wide level-synchronous with 3 cap checkpoints per decode (4-bit CN counts, dv = 5, "
                                         "dc = 10, 32-bit queue entries)")
    assert _sim(3, 6, 50, 5000, caps=CAPS5, fused_caps=True).kernel_choice() == first + (
        "wide level-synchronous with 5 cap checkpoints per decode (4-bit CN counts, dv = 3, dc = 6, 32-bit queue entries)")
    # the (4,8) forms of at most 65 536 CNs fuse as before, whatever the switch says
    for fused in (None, True, False):
        s = _sim(4, 8, 50, 1000, caps=CAPS5, fused_caps=fused)
        assert s.path == B.Path(torch.int16, "cn16", "vn", False, "level16", None)
        assert s.kernel_choice() == "sampler_v3 (CN->VN table) + full_bp_small level-synchronous with 5 cap checkpoints per " \
                                    "decode (4-bit CN counts)"


@pytest.mark.parametrize("shape", [(4, 8, 50, 5000), (3, 6, 50, 1000), (5, 10, 50, 5000)])
def test_without_the_opt_in_caps_raise_as_before(shape, monkeypatch):
    for fused in (None, False):
        for deg in (None, True, False):
            for wide in (None, True, False):
                with pytest.raises(ValueError) as e:
                    _sim(*shape, caps=CAPS5, fused_caps=fused, deg=deg, wide=wide)
                assert str(e.value) == TODAY + " (caps_sequential_reason)"
    # the vetoes, and what the fused decode never takes
    for kw in (dict(deg=False) if shape[0] != 4 else dict(wide=False), dict(rng="glibc"), dict(doped=(3,)), dict(rows_cap=64),
               dict(decoder="sw", W=10), dict(schedule="fixpoint")):
        with pytest.raises(ValueError, match=TODAY):
            _sim(*shape, caps=CAPS5, fused_caps=True, **kw)
    # a veto of the other family is none
    assert _sim(*shape, caps=CAPS5, fused_caps=True, **(dict(wide=False) if shape[0] != 4 else dict(deg=False))).path.cn_pass
    monkeypatch.setattr(B, "CAPS_FORMS_BY_DEFAULT", True)                # fused_caps=None follows the constant
    assert _sim(*shape, caps=CAPS5).path.decoder in ("wide", "deg16", "degwide")
    with pytest.raises(ValueError, match=TODAY):
        _sim(*shape, caps=CAPS5, fused_caps=False)


def test_the_librarys_shape_rule_decides(monkeypatch):
    with pytest.raises(ValueError, match=TODAY):
        _sim(4, 8, 50, 7000, caps=CAPS5, fused_caps=True)                # fewer than 1024 entries per wide queue
    with pytest.raises(ValueError, match=TODAY):
        _sim(3, 6, 50, 7000, caps=CAPS5, fused_caps=True)
    with monkeypatch.context() as m:
        m.setattr(E, "full_bp_wide_supported", lambda p: False)
        with pytest.raises(ValueError, match=TODAY):
            _sim(4, 8, 50, 5000, caps=CAPS5, fused_caps=True)
        assert _sim(3, 6, 50, 5000, caps=CAPS5, fused_caps=True).path.decoder == "degwide"
    with monkeypatch.context() as m:
        m.setattr(E, "full_bp_deg_supported", lambda p, wide=False: False)
        for N in (1000, 5000):
            with pytest.raises(ValueError, match=TODAY):
                _sim(3, 6, 50, N, caps=CAPS5, fused_caps=True)
        assert _sim(4, 8, 50, 5000, caps=CAPS5, fused_caps=True).path.decoder == "wide"
    with monkeypatch.context() as m:
        m.setattr(E, "full_bp_deg_supported", lambda p, wide=False: wide)
        assert _sim(3, 6, 50, 1000, caps=CAPS5, fused_caps=True).path.decoder == "degwide"


def test_decode_batch_caps_dispatches_on_the_path(monkeypatch):
    calls = []
    monkeypatch.setattr(E, "full_bp_caps_wide", lambda p, a, cn, ch, caps, is_term=True, counters=None:
                        calls.append(("wide", caps, tuple(counters.shape))))
    monkeypatch.setattr(E, "full_bp_caps_deg", lambda p, a, cn, ch, caps, is_term=True, counters=None, wide=False:
                        calls.append(("deg", wide, caps, tuple(counters.shape))))
    for shape in ((4, 8, 50, 5000), (3, 6, 50, 1000), (5, 10, 50, 5000)):
        s = _sim(*shape, caps=[3, 5], fused_caps=True, batch=4)
        s.d_adj = s.d_cn = s.d_ch = torch.zeros(4, 1)
        s.d_cnt_caps = torch.zeros(2 * 4 * E.NCOUNTERS, dtype=torch.int32)
        s.decode_batch_caps(3)
    assert calls == [("wide", (3, 5), (2, 3, 8)), ("deg", False, (3, 5), (2, 3, 8)), ("deg", True, (3, 5), (2, 3, 8))]


# ---- caps_sequential_reason --------------------------------------------------------------------------------------------------
def test_four_argument_reasons_are_todays():
    r = B.caps_sequential_reason
    assert r(E.make_params(4, 8, 10, 10), "philox", 0, "flooding") is None
    assert r(E.make_params(4, 8, 50, 1000), "philox", 0, "flooding") is None
    assert r(E.make_params(4, 8, 50, 5000), "philox", 0, "flooding") == (
        "more than 65536 CNs per trial: the wide form of the level-synchronous 4-bit decoder has no cap checkpoints")
    narrow_only = "the level-synchronous 4-bit decoder takes dv = 4, dc = 8 and at most 65536 CNs per trial"
    for p in (E.make_params(4, 8, 50, 10000), E.make_params(3, 6, 50, 1000), E.make_params(5, 10, 50, 1000),
              E.make_params(3, 6, 10, 10), E.make_params(3, 6, 50, 5000)):
        assert r(p, "philox", 0, "flooding") == narrow_only
        for wide in (None, True, False):                                 # and with the switch off or left alone
            for deg in (None, True, False):
                assert r(p, "philox", 0, "flooding", None, wide, deg) == r(p, "philox", 0, "flooding", False, wide, deg) \
                    == narrow_only
    p = E.make_params(4, 8, 10, 10)
    assert r(p, "glibc", 0, "flooding").startswith("--rng glibc: each cap's run replays srandom(seed)")
    assert r(p, "philox", 2, "flooding").startswith("NUM_DOPED > 0: the first doped position is MAX_IT")
    assert r(p, "philox", 0, "fixpoint") == "--schedule fixpoint has no iteration caps"


def test_seven_argument_reasons_follow_the_forms(monkeypatch):
    r = B.caps_sequential_reason
    wide48, n36, w510 = E.make_params(4, 8, 50, 5000), E.make_params(3, 6, 50, 1000), E.make_params(5, 10, 50, 5000)
    for p in (wide48, n36, w510, E.make_params(3, 6, 50, 5000), E.make_params(5, 10, 50, 1000), E.make_params(4, 8, 100, 2000),
              E.make_params(4, 8, 50, 1000)):
        assert r(p, "philox", 0, "flooding", True) is None
        assert r(p, "philox", 0, "flooding", True, True, True) is None
        assert "glibc" in r(p, "glibc", 0, "flooding", True)
        assert "NUM_DOPED" in r(p, "philox", 1, "flooding", True)
        assert "fixpoint" in r(p, "philox", 0, "fixpoint", True)
    # the vetoes act on their own family only
    assert r(wide48, "philox", 0, "flooding", True, False).startswith("--wide off")
    assert r(wide48, "philox", 0, "flooding", True, None, False) is None
    assert r(n36, "philox", 0, "flooding", True, None, False).startswith("--deg off")
    assert r(w510, "philox", 0, "flooding", True, None, False).startswith("--deg off")
    assert r(n36, "philox", 0, "flooding", True, False) is None and r(w510, "philox", 0, "flooding", True, False) is None
    # every other case names the limit
    assert "1024 queue entries" in r(E.make_params(4, 8, 50, 7000), "philox", 0, "flooding", True)
    assert "1024 queue entries" in r(E.make_params(3, 6, 50, 7000), "philox", 0, "flooding", True)
    assert "(3,6), (4,8) and (5,10)" in r(_lib.CodeParams(3, 9, 50, 300, 900), "philox", 0, "flooding", True)
    assert "no 2-byte VN -> CN table" in r(_lib.CodeParams(3, 6, 2, 70000, 140000), "philox", 0, "flooding", True)
    with monkeypatch.context() as m:                                     # the library's rule decides
        m.setattr(E, "full_bp_wide_supported", lambda p: False)
        assert "wide form" in r(wide48, "philox", 0, "flooding", True) and r(n36, "philox", 0, "flooding", True) is None
    with monkeypatch.context() as m:
        m.setattr(E, "full_bp_deg_supported", lambda p, wide=False: False)
        assert "_deg forms" in r(n36, "philox", 0, "flooding", True) and "_deg forms" in r(w510, "philox", 0, "flooding", True)
        assert r(wide48, "philox", 0, "flooding", True) is None
    monkeypatch.setattr(B, "CAPS_FORMS_BY_DEFAULT", True)                # None follows the constant, False stays off
    assert r(n36, "philox", 0, "flooding") is None and r(wide48, "philox", 0, "flooding", None) is None
    assert r(n36, "philox", 0, "flooding", False) is not None


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_only_bp_lim_iter_takes_the_switch():
    ap = B._parser("bp_lim_iter")
    assert ap.parse_args(["0", "0", "0", "350"]).caps_fused == "auto"
    for mode in ("auto", "on", "off"):
        assert ap.parse_args(["0", "0", "0", "350", "--caps", "175", "--caps-fused", mode]).caps_fused == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["0", "0", "0", "350", "--caps-fused", "yes"])
    with pytest.raises(SystemExit):
        B._parser("sw_lim_iter").parse_args(["0", "4", "0", "5", "5", "--caps-fused", "on"])
    with pytest.raises(SystemExit):
        B._parser("bp_traj").parse_args(["0", "0", "0", "50", "1", "--caps-fused", "on"])


class RecordingFake(CapsFake):
    made = []

    def __init__(self, p, **kw):
        type(self).made.append({k: kw.get(k) for k in ("caps", "wide", "deg", "fused_caps", "max_it")})
        super().__init__(p, **kw)


BASE = ["1", "0", "0", "350", "--L", "10", "--N", "10", "--num-points", "3", "--min-frame-err", "40", "--max-frames", "300",
        "--batch", "64", "--seed", "3"]
CAPS = "175,200,50,300"
ITS = (50, 175, 200, 300, 350)


def _run(monkeypatch, outdir, argv, quiet=True):
    monkeypatch.setattr(B, "Simulator", RecordingFake)
    RecordingFake.made = []
    RecordingFake.fused_calls = 0
    opts = B._parser("bp_lim_iter").parse_args(list(argv) + ["--outdir", str(outdir)] + (["--quiet"] if quiet else []))
    try:
        return B.run_program("bp_lim_iter", opts.INDEX, opts.W, opts.NUM_DOPED, opts.MAX_IT, None, opts)
    except SystemExit as e:
        return e.code


def _files(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


def _single_cap_files(monkeypatch, tmp_path, argv):
    want = {}
    for v in ITS:
        a = list(argv)
        a[3] = str(v)
        assert _run(monkeypatch, tmp_path / ("one%d" % v), a) == 0
        want.update(_files(tmp_path / ("one%d" % v)))
    return want


@pytest.mark.parametrize("pair", [("3", "6"), ("5", "10")])
def test_caps_fused_on_decodes_once_and_writes_the_single_cap_files(monkeypatch, tmp_path, capsys, pair):
    argv = BASE + ["--dv", pair[0], "--dc", pair[1]]
    want = _single_cap_files(monkeypatch, tmp_path, argv)
    assert len(want) == 5
    capsys.readouterr()
    assert _run(monkeypatch, tmp_path / "fused", argv + ["--caps", CAPS, "--caps-fused", "on"], quiet=False) == 0
    log = capsys.readouterr().err
    assert RecordingFake.fused_calls > 0 and "one after another" not in log
    assert RecordingFake.made == [dict(caps=[50, 175, 200, 300, 350], wide=None, deg=None, fused_caps=True, max_it=350)]
    assert _files(tmp_path / "fused") == want
    # --deg on is not needed and changes nothing; --wide off is no veto for this family
    assert _run(monkeypatch, tmp_path / "fused2", argv + ["--caps", CAPS, "--caps-fused", "on", "--deg", "on", "--wide", "off"]) == 0
    assert RecordingFake.made[0]["deg"] is True and RecordingFake.made[0]["wide"] is False and RecordingFake.fused_calls > 0
    assert _files(tmp_path / "fused2") == want
    # the default and `off`: one single-cap pass per cap, logged as before, the same files
    for extra in ([], ["--caps-fused", "off"], ["--caps-fused", "auto", "--deg", "on"]):
        d = tmp_path / ("seq" + "_".join(extra))
        capsys.readouterr()
        assert _run(monkeypatch, d, argv + ["--caps", CAPS] + extra, quiet=False) == 0
        log = capsys.readouterr().err
        assert ("[scldpc] kernels: --caps runs 5 single-cap passes one after another (the level-synchronous 4-bit decoder takes "
                "dv = 4, dc = 8 and at most 65536 CNs per trial)") in log
        assert RecordingFake.fused_calls == 0 and all(m["caps"] is None for m in RecordingFake.made) and len(RecordingFake.made) == 5
        assert _files(d) == want


def test_caps_fused_on_where_it_cannot_apply_is_an_error(monkeypatch, tmp_path):
    argv = BASE + ["--dv", "3", "--dc", "6", "--caps", CAPS, "--caps-fused", "on"]
    rc = _run(monkeypatch, tmp_path / "a", argv + ["--rng", "glibc"])
    assert isinstance(rc, str) and rc.startswith("--caps-fused on: --rng glibc: each cap's run replays srandom(seed)")
    rc = _run(monkeypatch, tmp_path / "b", argv + ["--deg", "off"])
    assert isinstance(rc, str) and rc.startswith("--caps-fused on: --deg off")
    doped = list(argv)
    doped[2] = "1"
    rc = _run(monkeypatch, tmp_path / "c", doped)
    assert isinstance(rc, str) and rc.startswith("--caps-fused on: NUM_DOPED > 0")
    rc = _run(monkeypatch, tmp_path / "d", BASE + ["--L", "50", "--N", "7000", "--caps", CAPS, "--caps-fused", "on"])
    assert isinstance(rc, str) and "1024 queue entries" in rc
    assert RecordingFake.made == [] and not any(os.path.exists(tmp_path / x) for x in "abcd")       # nothing ran
    # without --caps the switch is accepted and does nothing
    assert _run(monkeypatch, tmp_path / "e", BASE + ["--dv", "3", "--dc", "6", "--caps-fused", "on", "--rng", "glibc"]) == 0
    assert len(RecordingFake.made) == 1 and RecordingFake.made[0]["fused_caps"] is None and len(_files(tmp_path / "e")) == 1


def test_the_4_8_runs_pass_the_switches_and_fuse_as_before(monkeypatch, tmp_path):
    want = _single_cap_files(monkeypatch, tmp_path, BASE)
    for k, extra in enumerate(([], ["--caps-fused", "on"], ["--caps-fused", "off"])):
        assert _run(monkeypatch, tmp_path / ("f%d" % k), BASE + ["--caps", CAPS] + extra) == 0
        assert RecordingFake.fused_calls > 0 and len(RecordingFake.made) == 1
        assert _files(tmp_path / ("f%d" % k)) == want
