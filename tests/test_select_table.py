"""The Simulator's choice of the path, pinned as a table (CPU, no device buffers): for every combination of the axes below
the six path attributes, the dtype of the VN -> CN table and the kernel_choice() line — or the ValueError — as recorded
before the selection was gathered into one record.  `python tests/test_select_table.py` prints the two literals afresh.

The wide pin below it (WIDE_*) covers the three degree pairs, the four decoders and the seven switches, and records the
whole outcome of a selection: the Path, the dtype, kernel_choice(), the three sampler-switch reasons, ring_deg and the seven
legacy flags — or the ValueError.  Its record is tests/golden/select_table.json, written by
`python tests/test_select_table.py --record` from the code before the selection moved into one pure function."""
import itertools
import json
import os
import sys

import pytest
import torch

from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

SHAPES = [(50, 1000), (100, 1000), (50, 2474), (50, 5000), (100, 2000), (50, 7000)]
DECODERS = [("full", 0), ("sw", 10), ("sw", 400)]       # the ring window kernel takes W = 10 on every shape, W = 400 on none
# the axes of one group, in the order of the characters of its TABLE string
AXES = [("rng", ("philox", "glibc")), ("schedule", ("flooding", "fixpoint")), ("max_it", (0, 500)), ("rows_cap", (0, 64)),
        ("wide", (None, True, False)), ("caps", (None, (100, 200))), ("doped", ((), (3,)))]
FLAGS = ("sock", "gen2", "lvl2", "ring2", "wide", "wide_sock")
CODE = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


class SelectOnly(B.Simulator):
    """The Simulator's choice of kernels without its device buffers (its own copy of tests/fakes.py's: the recorder below runs
    against any revision of the package, also one whose tests/fakes.py has none)."""

    def _alloc(self):
        self.d_adj = torch.empty(0, dtype=self._select())


def outcome(L, N, decoder, W, **kw):
    """(the six flags as a 0/1 string, dtype, kernel_choice()) or ("ValueError", text)."""
    try:
        s = SelectOnly(E.make_params(4, 8, L, N), decoder=decoder, W=W, device="cpu", **kw)
    except ValueError as e:
        return ("ValueError", str(e))
    return ("".join("01"[bool(getattr(s, f))] for f in FLAGS), str(s.d_adj.dtype), s.kernel_choice())


def groups():
    for (L, N), (decoder, W) in itertools.product(SHAPES, DECODERS):
        yield (L, N, decoder, W)


def rows():
    for values in itertools.product(*(v for _, v in AXES)):
        yield dict(zip((k for k, _ in AXES), values))


# every distinct outcome; a character of TABLE is an index into this list (CODE)
OUTCOMES = [
    ('001000', 'torch.int16', 'sampler_v3 (CN->VN table) + full_bp_small level-synchronous (4-bit CN counts)'),
    ('001000', 'torch.int16', 'sampler_v3 (CN->VN table) + full_bp_small level-synchronous with 2 cap checkpoints per decode (4-bit CN counts)'),
    ('ValueError', 'caps: the fused decode takes Philox sampling, no doping and an ensemble of the level-synchronous 4-bit decoder (caps_sequential_reason)'),
    ('001000', 'torch.int16', 'sampler_v3 (CN->VN table) + full_bp_small level-synchronous (4-bit CN counts, trajectory rows)'),
    ('010000', 'torch.int16', 'sampler_v3 (CN->VN table) + full_bp_small fixpoint (4-bit CN counts)'),
    ('000000', 'torch.int32', "glibc replay on the host + full_bp (16-bit CN words): the 4-bit decoders take dv = 4, dc = 8 with device sampling and at most 65536 CNs per trial, or (the wide form, unless switched off) a state that leaves 1024 queue entries in one CU's LDS"),
    ('000000', 'torch.int32', "glibc replay on the host + full_bp (16-bit CN words, trajectory rows): the 4-bit decoders take dv = 4, dc = 8 with device sampling and at most 65536 CNs per trial, or (the wide form, unless switched off) a state that leaves 1024 queue entries in one CU's LDS"),
    ('000100', 'torch.int16', 'sampler_v2 (CN->socket table) + sw_ring (window state in LDS)'),
    ('000000', 'torch.int32', 'sampler (first generation) + sw_bp (whole chain)'),
    ('000000', 'torch.int16', 'sampler (first generation) + sw_bp (whole chain)'),
    ('101000', 'torch.int16', 'sampler_v3 (CN->socket table) + full_bp_small level-synchronous (4-bit CN counts)'),
    ('101000', 'torch.int16', 'sampler_v3 (CN->socket table) + full_bp_small level-synchronous with 2 cap checkpoints per decode (4-bit CN counts)'),
    ('101000', 'torch.int16', 'sampler_v3 (CN->socket table) + full_bp_small level-synchronous (4-bit CN counts, trajectory rows)'),
    ('110000', 'torch.int16', 'sampler_v3 (CN->socket table) + full_bp_small fixpoint (4-bit CN counts)'),
    ('000010', 'torch.int16', 'sampler (first generation) + cn_sockets pass + full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries)'),
    ('000000', 'torch.int16', "sampler (first generation) + full_bp (16-bit CN words): the 4-bit decoders take dv = 4, dc = 8 with device sampling and at most 65536 CNs per trial, or (the wide form, unless switched off) a state that leaves 1024 queue entries in one CU's LDS"),
    ('000010', 'torch.int16', 'sampler (first generation) + cn_sockets pass + full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries, trajectory rows)'),
    ('000000', 'torch.int16', "sampler (first generation) + full_bp (16-bit CN words, trajectory rows): the 4-bit decoders take dv = 4, dc = 8 with device sampling and at most 65536 CNs per trial, or (the wide form, unless switched off) a state that leaves 1024 queue entries in one CU's LDS"),
    ('000000', 'torch.int16', 'sampler (first generation) + sw_ring + cn_sockets pass'),
    ('000011', 'torch.int16', 'sampler_v3 (CN->socket table) + full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries)'),
    ('000011', 'torch.int16', 'sampler_v3 (CN->socket table) + full_bp_small wide level-synchronous (4-bit CN counts, 32-bit queue entries, trajectory rows)'),
]

# (L, N, decoder, W) -> one character per row of rows(), 192 of them
TABLE = {
    (50, 1000, 'full', 0):
        '001200120012332233223322001200120012332233223322441244124412332233223322001200120012332233223322'
        '552255225522662266226622552255225522662266226622552255225522662266226622552255225522662266226622',
    (50, 1000, 'sw', 10):
        '772277227722772277227722772277227722772277227722772277227722772277227722772277227722772277227722'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 1000, 'sw', 400):
        '992299229922992299229922992299229922992299229922992299229922992299229922992299229922992299229922'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (100, 1000, 'full', 0):
        'aab2aab2aab2cc22cc22cc22aab2aab2aab2cc22cc22cc22ddb2ddb2ddb2cc22cc22cc22aab2aab2aab2cc22cc22cc22'
        '552255225522662266226622552255225522662266226622552255225522662266226622552255225522662266226622',
    (100, 1000, 'sw', 10):
        '772277227722772277227722772277227722772277227722772277227722772277227722772277227722772277227722'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (100, 1000, 'sw', 400):
        '992299229922992299229922992299229922992299229922992299229922992299229922992299229922992299229922'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 2474, 'full', 0):
        'ee22ee22ff22gg22gg22hh22ee22ee22ff22gg22gg22hh22ff22ff22ff22gg22gg22hh22ee22ee22ff22gg22gg22hh22'
        '552255225522662266226622552255225522662266226622552255225522662266226622552255225522662266226622',
    (50, 2474, 'sw', 10):
        'ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 2474, 'sw', 400):
        '992299229922992299229922992299229922992299229922992299229922992299229922992299229922992299229922'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 5000, 'full', 0):
        'ee22ee22ff22gg22gg22hh22ee22ee22ff22gg22gg22hh22ff22ff22ff22gg22gg22hh22ee22ee22ff22gg22gg22hh22'
        '552255225522662266226622552255225522662266226622552255225522662266226622552255225522662266226622',
    (50, 5000, 'sw', 10):
        'ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 5000, 'sw', 400):
        '992299229922992299229922992299229922992299229922992299229922992299229922992299229922992299229922'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (100, 2000, 'full', 0):
        'jj22jj22ff22kk22kk22hh22jj22jj22ff22kk22kk22hh22ff22ff22ff22kk22kk22hh22jj22jj22ff22kk22kk22hh22'
        '552255225522662266226622552255225522662266226622552255225522662266226622552255225522662266226622',
    (100, 2000, 'sw', 10):
        '772277227722772277227722772277227722772277227722772277227722772277227722772277227722772277227722'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (100, 2000, 'sw', 400):
        '992299229922992299229922992299229922992299229922992299229922992299229922992299229922992299229922'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 7000, 'full', 0):
        'ff22ff22ff22hh22hh22hh22ff22ff22ff22hh22hh22hh22ff22ff22ff22hh22hh22hh22ff22ff22ff22hh22hh22hh22'
        '552255225522662266226622552255225522662266226622552255225522662266226622552255225522662266226622',
    (50, 7000, 'sw', 10):
        'ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22ii22'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
    (50, 7000, 'sw', 400):
        '992299229922992299229922992299229922992299229922992299229922992299229922992299229922992299229922'
        '882288228822882288228822882288228822882288228822882288228822882288228822882288228822882288228822',
}


def test_the_axes_are_the_recorded_ones():
    assert sorted(TABLE) == sorted(groups()) and all(len(v) == 192 for v in TABLE.values())
    assert len(list(rows())) == 192 and len(OUTCOMES) <= len(CODE)
    for L, N in SHAPES:
        p = E.make_params(4, 8, L, N)
        assert E.sw_ring_supported(p, 10) and not E.sw_ring_supported(p, 400)


@pytest.mark.parametrize("group", list(groups()), ids=lambda g: "L%d-N%d-%s-W%d" % g)
def test_selection_is_the_recorded_one(group):
    L, N, decoder, W = group
    for ch, kw in zip(TABLE[group], rows()):
        assert outcome(L, N, decoder, W, **kw) == OUTCOMES[CODE.index(ch)], (group, kw)


# ---------------------------------------------------------------------------------------------------------------------
# the wide pin: every pair, decoder and switch
# ---------------------------------------------------------------------------------------------------------------------
WIDE_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_table.json")
WIDE_SHAPES = [(4, 8, 50, 1000), (4, 8, 50, 2474), (4, 8, 50, 5000), (4, 8, 50, 7000),
               (3, 6, 50, 1000), (3, 6, 50, 5000), (3, 6, 50, 7000),
               (5, 10, 50, 1000), (5, 10, 50, 5000), (5, 10, 50, 7000)]
WIDE_DECODERS = [("full", 0), ("sw", 10), ("sw", 400), ("swc", 10)]
WIDE_AXES = [("rng", ("philox", "glibc")), ("schedule", ("flooding", "fixpoint")), ("max_it", (0, 500)), ("rows_cap", (0, 64)),
             ("caps", (None, (100, 200))), ("doped", ((), (3,)))]
SWITCHES = ("wide", "deg", "ring", "fused_caps", "sampled_table", "sampler2", "sampler2_wide")
# all seven left out, all True, all False, each True alone, each of wide / deg / ring False alone
SETTINGS = ([{}, dict.fromkeys(SWITCHES, True), dict.fromkeys(SWITCHES, False)] + [{name: True} for name in SWITCHES]
            + [{name: False} for name in ("wide", "deg", "ring")])
LEGACY_FLAGS = ("gen2", "lvl2", "wide", "sock", "ring2", "wide_sock", "deg")
REASONS = ("sampler2_deg_reason", "sampler2_wide_reason", "sampled_table_reason")


def wide_groups():
    for (dv, dc, L, N), (decoder, W) in itertools.product(WIDE_SHAPES, WIDE_DECODERS):
        yield (dv, dc, L, N, decoder, W)


def wide_rows():
    for values in itertools.product(*(v for _, v in WIDE_AXES)):
        for setting in SETTINGS:
            yield dict(zip((k for k, _ in WIDE_AXES), values), **setting)


def wide_outcome(dv, dc, L, N, decoder, W, **kw):
    """The whole outcome of one selection in the JSON form of the record: {"error": text} or the Path (dtype as its name),
    kernel_choice(), the three reasons, ring_deg and the legacy flags."""
    try:
        s = SelectOnly(E.make_params(dv, dc, L, N), decoder=decoder, W=W, device="cpu", **kw)
    except ValueError as e:
        return {"error": str(e)}
    return {"path": [str(s.path.adj_dtype)] + list(s.path[1:]), "dtype": str(s.d_adj.dtype), "kernel_choice": s.kernel_choice(),
            "reasons": [getattr(s, name) for name in REASONS], "ring_deg": bool(s.ring_deg),
            "flags": "".join("01"[bool(getattr(s, f))] for f in LEGACY_FLAGS)}


def _group_id(g):
    return "dv%d-dc%d-L%d-N%d-%s-W%d" % g


def load_record():
    with open(WIDE_RECORD) as f:
        return json.load(f)


def test_wide_axes_are_the_recorded_ones():
    rec = load_record()
    assert sorted(rec["table"]) == sorted(_group_id(g) for g in wide_groups())
    assert len(SETTINGS) == 13 and len(list(wide_rows())) == 832 and all(len(v) == 832 for v in rec["table"].values())
    assert rec["flags"] == list(LEGACY_FLAGS) and rec["reasons"] == list(REASONS) and rec["switches"] == list(SWITCHES)
    assert all(0 <= i < len(rec["outcomes"]) for v in rec["table"].values() for i in v)


def test_wide_record_covers_every_value_of_the_path():
    """Between them the recorded outcomes hold every sampler, CN table, decoder and fixpoint decoder of a Path, and the
    ValueError of caps that do not fuse: a record that lost one of them pins less than the selection has."""
    outcomes = load_record()["outcomes"]
    paths = [o["path"] for o in outcomes if "path" in o]
    assert {p[1] for p in paths} == {"glibc", "first", "first_sock", "cn16", "sock16", "deg_sock16", "wide_sock16"}
    assert {p[2] for p in paths} == {None, "vn", "sock"}
    assert {p[4] for p in paths} == {"sw_ring", "sw_chain", "swc_ring", "swc_chain", "level16", "wide", "full_bp", "deg16",
                                     "degwide"}
    assert {p[5] for p in paths} == {None, "fixpoint16", "fixpoint_deg", "fixpoint"}
    assert [o for o in outcomes if "error" in o] == [{"error": OUTCOMES[2][1]}]


@pytest.mark.parametrize("group", list(wide_groups()), ids=_group_id)
def test_wide_selection_is_the_recorded_one(group):
    rec = load_record()
    for i, kw in zip(rec["table"][_group_id(group)], wide_rows()):
        assert wide_outcome(*group, **kw) == rec["outcomes"][i], (group, kw)


def record_wide():
    seen, table = [], {}
    for g in wide_groups():
        row = []
        for kw in wide_rows():
            o = wide_outcome(*g, **kw)
            if o not in seen:
                seen.append(o)
            row.append(seen.index(o))
        table[_group_id(g)] = row
    with open(WIDE_RECORD, "w") as f:
        f.write('{"switches": %s,\n "flags": %s,\n "reasons": %s,\n "outcomes": [\n' % tuple(
            json.dumps(list(x)) for x in (SWITCHES, LEGACY_FLAGS, REASONS)))
        f.write(",\n".join("  " + json.dumps(o, sort_keys=True) for o in seen))
        f.write('\n ],\n "table": {\n')
        f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items()))
        f.write("\n }}\n")
    print("%d configurations, %d distinct outcomes, %d distinct paths" % (
        sum(len(v) for v in table.values()), len(seen), len({tuple(o["path"]) for o in seen if "path" in o})))


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record_wide()
        sys.exit(0)
    seen, table = [], {}
    for g in groups():
        text = ""
        for kw in rows():
            o = outcome(*g, **kw)
            if o not in seen:
                seen.append(o)
            text += CODE[seen.index(o)]
        table[g] = text
    for o in seen:
        print("    %r," % (o,))
    for g, text in table.items():
        print("    %r:\n        %r\n        %r," % (g, text[:96], text[96:]))
