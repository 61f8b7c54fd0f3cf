"""The wide 4-bit level decoder on CPU: the three new C-ABI symbols, the host-side shape rule of
scldpc_full_bp_wide_supported (what keeps a wrong shape from ever reaching a launch), the refusals decided before any device
work, and the Simulator's choice of the path (no device buffers: _alloc replaced as tests/fakes.py does)."""
import ctypes as C

import pytest

from fakes import SelectOnly
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

WIDE = "full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries"


def _lib():
    from fl_scaling_sc_ldpc_amd import _lib
    return _lib, _lib.lib()


def test_library_exports_the_wide_entry_points():
    _l, L = _lib()
    for name in ("scldpc_full_bp_wide_supported", "scldpc_full_bp_device_wide", "scldpc_full_bp_traj_device_wide"):
        assert name in _l.EXPORTS and hasattr(L, name)
    assert L.scldpc_abi_version() == 2                                   # additions only


# L, N, wide takes it — the table of the shape rule: the LEVEL carve at one workgroup per CU leaves >= 1024 entries per queue
SHAPES = [(50, 5000, True), (100, 2000, True), (50, 2474, True), (50, 1000, True), (50, 6000, True),
          (50, 7000, False),        # 392 entries per queue
          (50, 10000, False)]       # the state alone exceeds the LDS


@pytest.mark.parametrize("L,N,yes", SHAPES)
def test_wide_supported_follows_the_shape_rule(L, N, yes):
    p = E.make_params(4, 8, L, N)
    assert E.full_bp_wide_supported(p) == yes
    if (L, N) in ((50, 5000), (100, 2000), (50, 2474), (50, 6000)):      # that is why the wide form is needed
        _l, lib = _lib()
        assert lib.scldpc_full_bp_cn16_supported(C.byref(p)) == 0 and lib.scldpc_full_bp_sock16_supported(C.byref(p)) == 0
        assert p.nk > 65536
    if (L, N) == (50, 1000):                                             # the narrow forms take it too
        assert E.cn16_supported(p) and E.full_bp_sock16_supported(p)


def test_wide_supported_refuses_other_degrees_and_wide_sockets():
    _l, L = _lib()
    for dv, dc, cns, vns in ((3, 6, 500, 1000), (4, 16, 250, 1000), (5, 10, 500, 1000)):
        assert L.scldpc_full_bp_wide_supported(C.byref(_l.CodeParams(dv, dc, 50, cns, vns))) == 0
    assert L.scldpc_full_bp_wide_supported(C.byref(_l.CodeParams(4, 8, 2, 8192, 16384))) == 0       # vns_pos * dv = 65536
    assert L.scldpc_full_bp_wide_supported(C.byref(_l.CodeParams(4, 8, 2, 8190, 16380))) == 1       # 65520 sockets
    assert L.scldpc_full_bp_wide_supported(C.byref(_l.CodeParams(4, 8, 50, 500, 999))) == 0         # invalid parameters
    assert L.scldpc_full_bp_wide_supported(None) == 0


def test_wide_entry_points_refuse_on_the_host_before_any_launch():
    _l, L = _lib()
    ok = E.make_params(4, 8, 50, 5000)
    one = C.c_void_p(16)                                                 # non-null placeholders: never dereferenced on these paths

    def level(p, ntrials, a=one, cs=one, ch=one, cnt=one):
        return L.scldpc_full_bp_device_wide(C.byref(p), ntrials, a, cs, ch, 0, 1, cnt, None, None)

    def traj(p, ntrials, rows=one, rows_cap=8, a=one):
        return L.scldpc_full_bp_traj_device_wide(C.byref(p), ntrials, a, one, one, 0, 1, one, rows, rows_cap, None, None)

    for why, p in ((b"queue", E.make_params(4, 8, 50, 7000)), (b"LDS", E.make_params(4, 8, 50, 10000)),
                   (b"sockets", _l.CodeParams(4, 8, 2, 8192, 16384)), (b"dv = 4", _l.CodeParams(3, 6, 50, 500, 1000))):
        for rc in (level(p, 1), traj(p, 1), level(p, 0)):                # the shape is judged even for an empty batch
            assert rc == -2, (why, rc)                                   # SCLDPC_ERR_TOO_LARGE
            assert why in L.scldpc_last_error(), (why, L.scldpc_last_error())
    assert level(ok, 0, None, None, None, None) == 0 and traj(ok, 0) == 0                           # empty batch
    assert level(ok, -1) == -1 and traj(ok, -1) == -1                                                # SCLDPC_ERR_BAD_ARG
    for kw in (dict(a=None), dict(cs=None), dict(ch=None), dict(cnt=None)):
        assert level(ok, 1, **kw) == -1 and b"null buffer" in L.scldpc_last_error()
    assert traj(ok, 1, a=None) == -1
    assert traj(ok, 1, rows=None) == -1 and b"d_rows" in L.scldpc_last_error()
    assert traj(ok, 1, rows_cap=0) == -1 and b"rows_cap" in L.scldpc_last_error()


def _sim(L, N, **kw):
    return SelectOnly(E.make_params(4, 8, L, N), device="cpu", **kw)


def test_simulator_takes_the_wide_path_only_where_nothing_narrower_applies():
    assert B.WIDE_BY_DEFAULT is True                                     # profiles/traj_wide_speedup.json
    s = _sim(50, 5000, rows_cap=4096)
    assert s.wide and not s.wide_sock and not s.lvl2 and not s.gen2
    assert s.kernel_choice() == "sampler (first generation) + cn_sockets pass + " + WIDE + ", trajectory rows)"
    s = _sim(50, 5000, max_it=500)
    assert s.wide and s.kernel_choice() == "sampler (first generation) + cn_sockets pass + " + WIDE + ")"
    s = _sim(100, 2000, max_it=200)                                      # 8000 sockets per position: sampled with the code
    assert s.wide and s.wide_sock and s.kernel_choice() == "sampler_v3 (CN->socket table) + " + WIDE + ")"
    for kw in (dict(L=50, N=1000), dict(L=100, N=1000), dict(L=50, N=5000, rng="glibc"), dict(L=50, N=5000, decoder="sw", W=10),
               dict(L=50, N=5000, wide=False), dict(L=50, N=7000), dict(L=50, N=5000, schedule="fixpoint")):
        kw = dict(kw)
        s = _sim(kw.pop("L"), kw.pop("N"), **kw)
        assert not s.wide and not s.wide_sock, kw
    assert _sim(50, 1000).lvl2 and _sim(100, 1000).sock                  # the 16-bit forms keep their shapes
    assert _sim(50, 1000, wide=True).wide is False                       # … even when the wide form is asked for
    assert _sim(50, 5000, wide=True).wide and _sim(50, 5000, schedule="fixpoint", rows_cap=64).wide
    old = _sim(50, 5000, wide=False, rows_cap=64).kernel_choice()
    assert old.startswith("sampler (first generation) + full_bp (16-bit CN words, trajectory rows)")
    assert "65536 CNs" in old and "N <= 2048" not in old
    assert _sim(50, 5000, rng="glibc").kernel_choice().startswith("glibc replay on the host + full_bp (16-bit CN words)")


def test_simulator_follows_the_librarys_shape_rule(monkeypatch):
    monkeypatch.setattr(E, "full_bp_wide_supported", lambda p: False)
    assert not _sim(50, 5000).wide
    monkeypatch.setattr(E, "full_bp_wide_supported", lambda p: True)
    monkeypatch.setattr(E, "sock16_supported", lambda p: True)
    s = _sim(50, 5000)
    assert s.wide and s.wide_sock


def test_caps_keep_their_sequential_passes_on_a_wide_shape():
    p = E.make_params(4, 8, 50, 5000)
    why = B.caps_sequential_reason(p, "philox", 0, "flooding")
    assert why is not None and "wide" in why and "no cap checkpoints" in why
    assert B.caps_sequential_reason(E.make_params(4, 8, 50, 1000), "philox", 0, "flooding") is None
    assert "65536 CNs" in B.caps_sequential_reason(E.make_params(4, 8, 50, 10000), "philox", 0, "flooding")
    with pytest.raises(ValueError, match="caps"):
        _sim(50, 5000, caps=[100, 200])


def test_cli_passes_the_wide_switch_through():
    for prog in ("bp_traj", "bp_lim_iter"):
        ap = B._parser(prog)
        base = ["0", "0", "0", "500"] + (["0"] if prog == "bp_traj" else [])
        assert ap.parse_args(base).wide == "auto"
        assert ap.parse_args(base + ["--wide", "off"]).wide == "off"
