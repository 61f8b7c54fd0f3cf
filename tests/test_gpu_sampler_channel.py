"""The channel words of every sampler entry point against the CPU twin, oracle.sample_philox, bit for bit (-m gpu).

The samplers share the steps of a channel word (csrc/sampler_common.h: a draw's four bits, the bits past n masked, a doped
position cleared), so a test that compares one sampler with another cannot see an error there: only the twin can.  T = 2
trials at eps = 0.45, a seed with both halves set and a first trial above 2^32, on the smallest shapes that reach every branch
of the word's mask:

    (4,8)  L = 5, N = 64     n = 320 is a multiple of 32; doped (2,) covers words 4 and 5 exactly (hi - lo == 32)
    (4,8)  L = 7, N = 66     n = 462, n % 32 = 14; doped (0, 6) start and end inside words, the last word takes the tail
                             mask and the doping
    (3,6)  L = 5, N = 66     S % 4 == 2 (sampler_v2_deg.hip)
    (5,10) L = 5, N = 66     S % 4 == 2
    (4,8)  L = 5, N = 2050   S = 8200: sample_philox_big_kernel

So that no case is vacuous each one also asserts: no bit set in a doped position, none at or past n in the last word, and
at least one in every other position — which the twin alone satisfies on these shapes (checked without a GPU below)."""
import numpy as np
import pytest

from conftest import require_gpu

T, EPS = 2, 0.45
SEED = 0xFEDCBA9876543210
TRIAL0 = (1 << 32) + 5

# (dv, dc, L, N, doped)
SMALL_A = (4, 8, 5, 64, (2,))
SMALL_B = (4, 8, 7, 66, (0, 6))
DEG_36 = (3, 6, 5, 66, (0, 4))
DEG_510 = (5, 10, 5, 66, (0, 4))
BIG = (4, 8, 5, 2050, (4,))

ENTRIES_48 = ["philox32", "philox16", "sock", "cn16", "sock16", "cn16_gen3"]
CASES = ([(s, e) for s in (SMALL_A, SMALL_B) for e in ENTRIES_48]
         + [(s, e) for s in (DEG_36, DEG_510) for e in ("philox16", "sock", "deg_sock16")]
         + [(BIG, e) for e in ("philox16", "sock")])


_TWIN = {}


def _twin(O, shape):
    """Channel words [T, nw] of the CPU twin; computed once per shape and left unchanged."""
    if shape in _TWIN:
        return _TWIN[shape]
    from fl_scaling_sc_ldpc_amd import engine as E
    dv, dc, L, N, doped = shape
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    words = np.stack([O.sample_philox(po, SEED, TRIAL0 + t, EPS, doped=doped)[1] for t in range(T)])
    words.setflags(write=False)
    _TWIN[shape] = words
    return words


def _not_vacuous(shape, words):
    from fl_scaling_sc_ldpc_amd import engine as E
    dv, dc, L, N, doped = shape
    n = L * N
    w = np.ascontiguousarray(words).view(np.uint32).reshape(T, -1)
    assert w.shape[1] == (n + 31) // 32
    if n % 32:
        assert not (w[:, -1] >> np.uint32(n % 32)).any(), "a bit at or past n in the last word"
    bits = E.unpack_bits(w, n).reshape(T, L, N)
    for pos in range(L):
        if pos in doped:
            assert not bits[:, pos].any(), f"doped position {pos} has an erased VN"
        else:
            assert bits[:, pos].any(axis=1).all(), f"position {pos} has no erased VN"


@pytest.mark.parametrize("shape", [SMALL_A, SMALL_B, DEG_36, DEG_510, BIG], ids=lambda s: "%d-%d-L%d-N%d" % s[:4])
def test_twin_reaches_every_branch_of_the_mask(oracle, shape):
    _not_vacuous(shape, _twin(oracle, shape))
    dv, dc, L, N, doped = shape
    assert (N * dv // dc * dc) % 4 == (2 if dv != 4 else 0)
    if shape is SMALL_A:
        assert (L * N) % 32 == 0 and (doped[0] * N) % 32 == 0 and N == 64      # two whole words
    if shape is SMALL_B:
        assert (L * N) % 32 == 14 and N % 32 != 0 and doped[-1] == L - 1


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@pytest.mark.gpu
@pytest.mark.parametrize("shape,entry", CASES, ids=lambda v: v if isinstance(v, str) else "%d-%d-L%d-N%d" % v[:4])
def test_channel_words_equal_the_twin(E, oracle, monkeypatch, shape, entry):
    import torch
    dv, dc, L, N, doped = shape
    p = E.make_params(dv, dc, L, N)
    monkeypatch.setenv("SCLDPC_SAMPLER_GEN", "3" if entry == "cn16_gen3" else "2")
    call = {"philox32": lambda: E.sample_philox(p, SEED, TRIAL0, T, EPS, doped=doped, adj16=False),
            "philox16": lambda: E.sample_philox(p, SEED, TRIAL0, T, EPS, doped=doped, adj16=True),
            "sock": lambda: E.sample_philox_sock(p, SEED, TRIAL0, T, EPS, doped=doped),
            "cn16": lambda: E.sample_philox_cn16(p, SEED, TRIAL0, T, EPS, doped=doped),
            "cn16_gen3": lambda: E.sample_philox_cn16(p, SEED, TRIAL0, T, EPS, doped=doped),
            "sock16": lambda: E.sample_philox_sock16(p, SEED, TRIAL0, T, EPS, doped=doped),
            "deg_sock16": lambda: E.sample_philox_deg_sock16(p, SEED, TRIAL0, T, EPS, doped=doped)}[entry]
    chan = call()[-1]
    torch.cuda.synchronize()
    got = chan.cpu().numpy().view(np.uint32).reshape(T, -1)
    want = _twin(oracle, shape)
    assert got.shape == want.shape
    assert (got.astype(np.int64) == want.astype(np.int64)).all(), np.argwhere(got != want)[:8]
    _not_vacuous(shape, got)
