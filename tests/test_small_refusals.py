"""What the ten entry points of the 4-bit decoder family refuse on the host, pinned call by call (CPU: placeholder pointers
that are never dereferenced, one defect per call): the return code and a distinguishing part of scldpc_last_error(), as
recorded before the three launchers became one.  A call with several defects may report any of them; none is made here."""
import ctypes as C

import pytest

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E

ONE = C.c_void_p(16)
NULL = "NULL"                                               # call(p=NULL): no parameter struct
FIX = ("scldpc_full_bp_fixpoint_device_cn16", "scldpc_full_bp_fixpoint_device_sock16")
LEVEL = ("scldpc_full_bp_device_cn16", "scldpc_full_bp_device_sock16", "scldpc_full_bp_device_wide")
TRAJ = ("scldpc_full_bp_traj_device_cn16", "scldpc_full_bp_traj_device_sock16", "scldpc_full_bp_traj_device_wide")
CAPS = ("scldpc_full_bp_caps_device_cn16", "scldpc_full_bp_caps_device_sock16")
ALL = FIX + LEVEL + TRAJ + CAPS
WIDE = tuple(e for e in ALL if e.endswith("_wide"))
NARROW = tuple(e for e in ALL if not e.endswith("_wide"))
CN16 = tuple(e for e in ALL if e.endswith("_cn16"))
SOCK16 = tuple(e for e in ALL if e.endswith("_sock16"))
BAD_ARG, TOO_LARGE = -1, -2


def good(entry):
    """An ensemble the entry point takes."""
    return E.make_params(4, 8, 50, 5000) if entry in WIDE else E.make_params(4, 8, 50, 1000)


def call(entry, p=None, ntrials=1, a=ONE, cn=ONE, ch=ONE, cnt=ONE, rows=ONE, rows_cap=8, caps=(3, 5), ncaps=None):
    """(return code, last error) of one call; every buffer a non-null placeholder unless the defect says otherwise."""
    fn = getattr(_lib.lib(), entry)
    p = C.byref(good(entry) if p is None else p) if p is not NULL else None
    if entry in FIX:
        rc = fn(p, ntrials, a, cn, ch, 1, cnt, None, None)
    elif entry in LEVEL:
        rc = fn(p, ntrials, a, cn, ch, 0, 1, cnt, None, None)
    elif entry in TRAJ:
        rc = fn(p, ntrials, a, cn, ch, 0, 1, cnt, rows, rows_cap, None, None)
    else:
        arr = (C.c_int32 * max(1, len(caps)))(*caps) if caps is not None else None
        rc = fn(p, ntrials, a, cn, ch, len(caps or ()) if ncaps is None else ncaps, arr, 1, cnt, None)
    return rc, _lib.lib().scldpc_last_error().decode()


DEGREES = _lib.CodeParams(3, 6, 50, 500, 1000)
INVALID = _lib.CodeParams(4, 8, 50, 500, 999)               # dv * vns_pos != dc * cns_pos
MANY_CNS = E.make_params(4, 8, 50, 5000)                    # 132 500 CNs per trial, 20 000 sockets per position
MANY_CNS_FEW_VNS = E.make_params(4, 8, 2, 26216)            # 65 540 CNs per trial, 52 432 VNs
MANY_VNS = E.make_params(4, 8, 100, 1000)                   # 100 000 VNs, 51 500 CNs: the socket table only
SHORT_QUEUE = E.make_params(4, 8, 50, 7000)                 # 392 entries per queue
NO_ROOM = E.make_params(4, 8, 50, 10000)                    # the state alone exceeds the LDS
MANY_SOCKETS = _lib.CodeParams(4, 8, 2, 8192, 16384)        # vns_pos * dv = 65536

# (defect, the entry points it is tried on, call arguments, return code, part of the message)
CASES = [
    ("negative ntrials", ALL, dict(ntrials=-1), BAD_ARG, "negative ntrials"),
    ("vn_adj16 null", ALL, dict(a=None), BAD_ARG, "null buffer"),
    ("CN table null", ALL, dict(cn=None), BAD_ARG, "null buffer"),
    ("chan_bits null", ALL, dict(ch=None), BAD_ARG, "null buffer"),
    ("counters null", ALL, dict(cnt=None), BAD_ARG, "null buffer"),
    ("d_rows null", TRAJ, dict(rows=None), BAD_ARG, "null d_rows"),
    ("rows_cap 0", TRAJ, dict(rows_cap=0), BAD_ARG, "rows_cap <= 0"),
    ("rows_cap negative", TRAJ, dict(rows_cap=-3), BAD_ARG, "rows_cap <= 0"),
    ("no caps", CAPS, dict(caps=(), ncaps=0), BAD_ARG, "takes 1 .. 16 caps (ncaps = 0)"),
    ("17 caps", CAPS, dict(caps=tuple(range(1, 18))), BAD_ARG, "takes 1 .. 16 caps (ncaps = 17)"),
    ("caps NULL", CAPS, dict(caps=None, ncaps=2), BAD_ARG, "caps NULL"),
    ("caps decreasing", CAPS, dict(caps=(5, 3)), BAD_ARG, "strictly increasing and >= 1 (caps[1] = 3)"),
    ("caps repeated", CAPS, dict(caps=(3, 3)), BAD_ARG, "strictly increasing and >= 1 (caps[1] = 3)"),
    ("cap below one", CAPS, dict(caps=(0, 3)), BAD_ARG, "strictly increasing and >= 1 (caps[0] = 0)"),
    ("wrong degrees", ALL, dict(p=DEGREES), TOO_LARGE, "takes dv = 4, dc = 8"),
    ("too many CNs", CN16, dict(p=MANY_CNS_FEW_VNS), TOO_LARGE, "at most 65536 CNs per trial"),
    ("too many CNs", SOCK16, dict(p=MANY_CNS), TOO_LARGE, "at most 65536 CNs per trial"),
    ("too many sockets", SOCK16, dict(p=MANY_SOCKETS), TOO_LARGE, "sockets"),
    ("too many VNs for the CN -> VN table", CN16, dict(p=MANY_VNS), TOO_LARGE, "fewer than 65535 VNs (use the _sock16 form beyond)"),
    ("short queues", WIDE, dict(p=SHORT_QUEUE), TOO_LARGE, "queue: the LDS left by the state holds fewer than 1024 entries"),
    ("state beyond the LDS", WIDE, dict(p=NO_ROOM), TOO_LARGE, "LDS: the CN counts and VN bits of a trial exceed 160 KiB"),
    ("too many sockets", WIDE, dict(p=MANY_SOCKETS), TOO_LARGE, "sockets: vns_pos * dv must fit 16 bits (at most 65535)"),
    ("invalid parameters", ALL, dict(p=INVALID), BAD_ARG, "dv*vns_pos (4*999) must equal dc*cns_pos (8*500)"),
    ("null parameters", ALL, dict(p=NULL), BAD_ARG, "null scldpc_code_params"),
    # the shape is judged even for an empty batch …
    ("wrong degrees, empty batch", ALL, dict(p=DEGREES, ntrials=0), TOO_LARGE, "dv = 4"),
    ("too many CNs, empty batch", SOCK16, dict(p=MANY_CNS, ntrials=0), TOO_LARGE, "65536 CNs"),
    ("too many VNs, empty batch", CN16, dict(p=MANY_VNS, ntrials=0), TOO_LARGE, "_sock16"),
    ("short queues, empty batch", WIDE, dict(p=SHORT_QUEUE, ntrials=0), TOO_LARGE, "queue"),
    # … which needs no buffers
    ("empty batch", ALL, dict(ntrials=0), 0, None),
    ("empty batch, null buffers", FIX + LEVEL + CAPS, dict(ntrials=0, a=None, cn=None, ch=None, cnt=None), 0, None),
    ("empty batch, null buffers", TRAJ, dict(ntrials=0, a=None, cn=None, ch=None, cnt=None), 0, None),
]


def test_the_ten_entry_points_are_exported():
    assert len(ALL) == 10 and len(set(ALL)) == 10
    for entry in ALL:
        assert entry in _lib.EXPORTS and hasattr(_lib.lib(), entry)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0].replace(" ", "_"))
def test_refusal_is_the_recorded_one(case):
    defect, entries, kw, want_rc, part = case
    for entry in entries:
        rc, msg = call(entry, **kw)
        assert rc == want_rc, (defect, entry, rc, msg)
        if part is not None:
            assert part in msg, (defect, entry, msg)
            # every refusal of the launcher itself names the entry point; the parameter check is shared by the whole library
            assert msg.startswith(entry + ": ") or defect in ("invalid parameters", "null parameters"), (defect, entry, msg)


def test_the_socket_forms_have_no_persistent_instance(monkeypatch):
    """SCLDPC_DEBUG_GRID_DECODER (fewer workgroups than trials) reaches the persistent instances, which exist for the CN -> VN
    table only; the caps and wide forms do not read the knob, so with placeholder pointers they are not called here."""
    monkeypatch.setenv("SCLDPC_DEBUG_GRID_DECODER", "1")
    for entry in ("scldpc_full_bp_fixpoint_device_sock16", "scldpc_full_bp_device_sock16", "scldpc_full_bp_traj_device_sock16"):
        rc, msg = call(entry, ntrials=2)
        assert rc == BAD_ARG and msg == entry + ": no persistent form with the socket table", (entry, rc, msg)
        assert call(entry, ntrials=0)[0] == 0
