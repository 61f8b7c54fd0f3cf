"""The headline's sampler instance, sample_philox_v2_kernel<1,4,1> (C2: (4,8), L = 50, N = 1000, 4000 sockets per CN
position), against the first-generation sampler and the CPU twin at several seeds, trial offsets and erasure rates, and
its exact fallback forced position by position (-m gpu).  The VN -> CN table and the channel words must be bit for bit
the first generation's; the CN -> VN and CN -> socket tables hold, per CN, the same set as the host's inversion."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

L, N = 50, 1000


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def _cn_sets(E, p, adj16, cn16):
    c = np.sort(np.ascontiguousarray(cn16).view(np.uint16), axis=1)
    want = E.cn_adj_from_vn_adj(p, adj16)[0].view(np.uint16)            # ascending VNs, then 0xFFFF
    assert (c == want).all()


def _sock_as_vn(p, sock16):
    """CN -> socket table [D*cns_pos, dc] as global VN ids: socket 4t + u of CN position q is edge u of VN t of q - u."""
    s = np.ascontiguousarray(sock16).view(np.uint16).reshape(-1, p.cns_pos, 8).astype(np.int64)
    q = np.arange(s.shape[0])[:, None, None]
    u, t = s & 3, s >> 2
    vn = np.where((s != 0xFFFF) & (q - u >= 0) & (q - u < p.L), (q - u) * p.vns_pos + t, 0xFFFF)
    return np.sort(vn.reshape(-1, 8), axis=1)


@pytest.mark.parametrize("eps", [0.3, 0.48, 0.6])
@pytest.mark.parametrize("seed,t0", [(1, 0), (0x5EED5EED, 12345), (0xFEDCBA9876543210, (1 << 40) + 3)])
def test_c2_sampler_equals_first_generation_and_twin(E, oracle, monkeypatch, seed, t0, eps):
    import torch
    monkeypatch.setenv("SCLDPC_SAMPLER_GEN", "2")
    p = E.make_params(4, 8, L, N)
    T = 6
    a1, c1 = E.sample_philox(p, seed, t0, T, eps, adj16=True)
    a2, cn2, c2 = E.sample_philox_cn16(p, seed, t0, T, eps)
    a3, s3, c3 = E.sample_philox_sock16(p, seed, t0, T, eps)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(c1, c2) and torch.equal(a1, a3) and torch.equal(c1, c3)
    A, CN, SK = a2.cpu().numpy(), cn2.cpu().numpy(), s3.cpu().numpy()
    po = oracle.Params(4, 8, L, p.cns_pos, p.vns_pos)
    ta, tch = oracle.sample_philox(po, seed, t0 + T - 1, eps)           # CPU twin of the last trial (global ids)
    assert (E.adj16_to_global(p, A[T - 1]) == ta).all()
    assert (E.unpack_bits(c2[T - 1].cpu().numpy(), p.n) == E.unpack_bits(tch, p.n)).all()
    for t in (0, T - 1):
        _cn_sets(E, p, A[t], CN[t])
        want = E.cn_adj_from_vn_adj(p, A[t])[0].view(np.uint16).astype(np.int64)
        assert (_sock_as_vn(p, SK[t]) == want).all()


@pytest.mark.parametrize("which", [0, 1, 3, 26, L + 2, -2])
def test_c2_sampler_exact_fallback_per_position(E, monkeypatch, which):
    """SCLDPC_DEBUG_SAMPLER_EXACT_POS ranks one CN position (or every one, -2) by the exact fallback that a crowded
    histogram or a full worklist would take: the same tables come out."""
    import torch
    monkeypatch.setenv("SCLDPC_SAMPLER_GEN", "2")
    p = E.make_params(4, 8, L, N)
    seed, t0, T = 0xC2C2, 77, 4
    a1, cn1, c1 = E.sample_philox_cn16(p, seed, t0, T, 0.48)
    s1 = E.sample_philox_sock16(p, seed, t0, T, 0.48)[1]
    monkeypatch.setenv("SCLDPC_DEBUG_SAMPLER_EXACT_POS", str(which))
    a2, cn2, c2 = E.sample_philox_cn16(p, seed, t0, T, 0.48)
    s2 = E.sample_philox_sock16(p, seed, t0, T, 0.48)[1]
    torch.cuda.synchronize()
    monkeypatch.delenv("SCLDPC_DEBUG_SAMPLER_EXACT_POS")
    assert torch.equal(a1, a2) and torch.equal(c1, c2)
    for x, y in ((cn1, cn2), (s1, s2)):
        assert (np.sort(x.cpu().numpy().view(np.uint16), axis=2) == np.sort(y.cpu().numpy().view(np.uint16), axis=2)).all()
    _cn_sets(E, p, a2[0].cpu().numpy(), cn2[0].cpu().numpy())
