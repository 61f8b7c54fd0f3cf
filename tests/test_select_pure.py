"""bp_decoding.select_path is a function of its two records (CPU): hand-made Config and Capabilities, no ensemble of the
library, no *_supported call — the same answers with every one of them made to raise."""
import pytest
import torch

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

NOTHING = B.Capabilities(None, *[False] * (len(B.Capabilities._fields) - 1))
SWITCHES = ("wide", "deg", "ring", "fused_caps", "sampled_table", "sampler2", "sampler2_wide")


def config(dv, dc, N, **kw):
    """A Config written out by hand: L = 50, N VNs per position, full BP with Philox sampling, every switch off."""
    c = B.Config(dv=dv, dc=dc, L=50, vns_pos=N, cns_pos=N * dv // dc, W=0, decoder="full", rng="philox", schedule="flooding",
                 max_it=0, rows_cap=0, caps=False, num_doped=0, wide=False, deg=False, ring=False, fused_caps=False,
                 sampled_table=False, sampler2=False, sampler2_wide=False, wide_off=False, deg_off=False)
    return c._replace(**kw)


def all_on(c):
    return c._replace(**dict.fromkeys(SWITCHES, True))


def cases():
    """(name, Config, Capabilities, the Path, the reasons that are None)."""
    i16 = torch.int16
    yield ("nothing supported", config(4, 8, 1000), NOTHING, B.Path(i16, "first", None, False, "full_bp", None), ())
    yield ("nothing supported, every switch on", all_on(config(4, 8, 1000)), NOTHING,
           B.Path(i16, "first", None, False, "full_bp", None), ())
    yield ("nothing supported, glibc", config(4, 8, 1000, rng="glibc"), NOTHING,
           B.Path(torch.int32, "glibc", None, False, "full_bp", None), ())
    yield ("nothing supported, sw", all_on(config(3, 6, 1000, decoder="sw", W=10)), NOTHING,
           B.Path(i16, "first", None, False, "sw_chain", None), ())
    yield ("nothing supported, swc", all_on(config(5, 10, 1000, decoder="swc", W=10)), NOTHING,
           B.Path(i16, "first", None, False, "swc_chain", None), ())
    yield ("(4,8), cn16", config(4, 8, 1000), NOTHING._replace(cn16_table="vn"), B.Path(i16, "cn16", "vn", False, "level16", None), ())
    yield ("(4,8), sock16 table", config(4, 8, 1000), NOTHING._replace(cn16_table="sock"),
           B.Path(i16, "sock16", "sock", False, "level16", None), ())
    yield ("(4,8), cn16, unlimited fixpoint", config(4, 8, 1000, schedule="fixpoint"), NOTHING._replace(cn16_table="vn"),
           B.Path(i16, "cn16", "vn", False, "full_bp", "fixpoint16"), ())
    deg = NOTHING._replace(full_bp_deg=True, deg_sock16=True)
    yield ("(3,6), deg", config(3, 6, 1000, deg=True), deg, B.Path(i16, "first", "sock", True, "deg16", None), ())
    yield ("(3,6), deg, sampler2", config(3, 6, 1000, deg=True, sampler2=True), deg,
           B.Path(i16, "deg_sock16", "sock", False, "deg16", None), ("sampler2_deg_reason",))
    yield ("(3,6), deg off, sampler2", config(3, 6, 1000, sampler2=True), deg, B.Path(i16, "first", None, False, "full_bp", None), ())
    wide = NOTHING._replace(full_bp_wide=True, wide_sock16=True, first_sock=True)
    yield ("(4,8), wide", config(4, 8, 5000, wide=True), wide, B.Path(i16, "first", "sock", True, "wide", None), ())
    yield ("(4,8), wide, sampled table", config(4, 8, 5000, wide=True, sampled_table=True), wide,
           B.Path(i16, "first_sock", "sock", False, "wide", None), ("sampled_table_reason",))
    yield ("(4,8), wide, sampler2_wide and sampled table", config(4, 8, 5000, wide=True, sampler2_wide=True, sampled_table=True),
           wide, B.Path(i16, "wide_sock16", "sock", False, "wide", None), ("sampler2_wide_reason",))


CASES = list(cases())


def check(case):
    name, c, k, path, taken = case
    sel = B.select_path(c, k)
    assert sel.path == path, name
    for reason in ("sampler2_deg_reason", "sampler2_wide_reason", "sampled_table_reason"):
        assert (getattr(sel, reason) is None) == (reason in taken), (name, reason)
    assert sel.caps_error is None, name
    return sel


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_selection_of_hand_made_records(case):
    check(case)


def test_the_wide_sampler_wins_and_the_sampled_table_says_why_it_stood_back():
    sel = check(CASES[-1])
    assert sel.sampled_table_reason == ("the second-generation sampler takes this ensemble and writes the CN table with the code "
                                        "already")
    assert sel.sampler2_deg_reason == "switched off"
    sel = B.select_path(CASES[-1][1]._replace(sampler2=True), CASES[-1][2])
    assert sel.path == CASES[-1][3]
    assert sel.sampler2_deg_reason == "dv = 4, dc = 8 has a second-generation sampler of its own, chosen without this switch"


def test_caps_without_a_decode_that_has_checkpoints_are_the_error():
    assert B.select_path(config(4, 8, 1000, caps=True), NOTHING).caps_error == B.CAPS_ERROR
    level16 = NOTHING._replace(cn16_table="vn")
    assert B.select_path(config(4, 8, 1000, caps=True), level16).caps_error is None
    assert B.select_path(config(4, 8, 1000, caps=True, num_doped=1), level16).caps_error == B.CAPS_ERROR
    assert B.select_path(config(4, 8, 1000, caps=True, rows_cap=64), level16).caps_error == B.CAPS_ERROR


def test_no_library_rule_is_asked(monkeypatch):
    """Every *_supported of the engine, and the library's loader, raise: select_path answers as before."""
    def refuse(*a, **kw):
        raise AssertionError("select_path asked the library")
    names = [n for n in dir(E) if n.endswith("_supported")]
    assert len(names) >= 12
    for n in names:
        monkeypatch.setattr(E, n, refuse)
    monkeypatch.setattr(E, "lib", refuse)
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(B, "_capabilities", refuse)
    monkeypatch.setattr(B, "_cn16_table", refuse)
    for case in CASES:
        check(case)
