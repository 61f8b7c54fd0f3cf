"""The Simulator's choice of the path, pinned as a table (CPU, no device buffers): for every combination of the axes below
the six path attributes, the dtype of the VN -> CN table and the kernel_choice() line — or the ValueError — as recorded
before the selection was gathered into one record.  `python tests/test_select_table.py` prints the two literals afresh."""
import itertools

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
    """The Simulator's choice of kernels without its device buffers (as tests/test_wide_host.py)."""

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


if __name__ == "__main__":
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
