"""The second-generation sampler's split Philox draw (csrc/philox.h: per-trial prefix, per-position uniform part, tail)
against the first generation, which calls the plain philox4x32_10 (-m gpu).  sample_philox_cn16 and sample_philox_sock16
must give sample_philox(..., adj16=True)'s VN table and channel bit for bit, and CN rows that hold, as sets, the host's
inversion of the VN table — on the smallest shapes that reach each path:

    (4,8) L = 5, N = 16      most threads own no socket
    L = 6, N = 256           one histogram word per thread (ROWS = 1)
    L = 8, N = 1000          the headline instance <1,4,.> on a short chain
    L = 4, N = 2000          two calls per thread (KMAX = 2): a second prefix with c0 = tid + 1024

with trial offsets 0, 2^32 - 2 (one launch of three trials crosses the 32-bit boundary of the trial index: a prefix built
from the high word or a uniform part built from the low word would go wrong there) and 2^40 + 7, seeds with a zero high
half and with both halves set, and one doped position (the channel's draw has its own hoisted product)."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

SHAPES = [(5, 16), (6, 256), (8, 1000), (4, 2000)]
TRIAL0 = [0, (1 << 32) - 2, (1 << 40) + 7]
SEEDS = [0x5EED5EED, 0xFEDCBA9876543210]
T, EPS = 3, 0.48


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def _sock_as_vn(p, sock16):
    """CN -> socket table [D*cns_pos, dc] as global VN ids: socket 4t + u of CN position q is edge u of VN t of q - u."""
    s = np.ascontiguousarray(sock16).view(np.uint16).reshape(-1, p.cns_pos, 8).astype(np.int64)
    q = np.arange(s.shape[0])[:, None, None]
    u, t = s & 3, s >> 2
    vn = np.where((s != 0xFFFF) & (q - u >= 0) & (q - u < p.L), (q - u) * p.vns_pos + t, 0xFFFF)
    return np.sort(vn.reshape(-1, 8), axis=1)


def _check(E, p, seed, t0, doped):
    import torch
    a1, c1 = E.sample_philox(p, seed, t0, T, EPS, doped=doped, adj16=True)
    a2, cn2, c2 = E.sample_philox_cn16(p, seed, t0, T, EPS, doped=doped)
    a3, s3, c3 = E.sample_philox_sock16(p, seed, t0, T, EPS, doped=doped)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(a1, a3), "VN table"
    assert torch.equal(c1, c2) and torch.equal(c1, c3), "channel"
    A, CN, SK = a1.cpu().numpy(), cn2.cpu().numpy(), s3.cpu().numpy()
    want = E.cn_adj_from_vn_adj(p, A).view(np.uint16)                   # ascending VNs, then 0xFFFF
    assert (np.sort(CN.view(np.uint16), axis=2) == want).all()
    for t in range(T):
        assert (_sock_as_vn(p, SK[t]) == want[t].astype(np.int64)).all()
    # the doped position is never erased, and the channel is not trivially empty elsewhere
    bits = E.unpack_bits(c1.cpu().numpy(), p.n).reshape(T, p.L, p.vns_pos)
    assert not bits[:, doped[0]].any() and bits.any()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("t0", TRIAL0)
@pytest.mark.parametrize("L,N", SHAPES)
def test_split_draw_equals_first_generation(E, monkeypatch, L, N, t0, seed):
    monkeypatch.setenv("SCLDPC_SAMPLER_GEN", "2")
    _check(E, E.make_params(4, 8, L, N), seed, t0, doped=(1,))


def test_split_draw_with_every_position_on_the_exact_fallback(E, monkeypatch):
    monkeypatch.setenv("SCLDPC_SAMPLER_GEN", "2")
    monkeypatch.setenv("SCLDPC_DEBUG_SAMPLER_EXACT_POS", "-2")
    _check(E, E.make_params(4, 8, 6, 256), SEEDS[1], TRIAL0[1], doped=(1,))
