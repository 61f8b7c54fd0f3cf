"""The CN -> socket table written by the first-generation sampler's own launch (-m gpu): sample_philox_sock against a numpy
inversion of its own VN -> CN rows (neither the cn_sockets pass nor the code under test), its rows and channel words bit for bit
those of sample_philox(adj16=True), nothing written past the T trials asked for — through every instance of the small kernel,
every ranking of the big one, the decoders that consume the table, and the command line.  Integer work: no tolerance anywhere."""
import os

import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu

T, SEED, TRIAL0, EPS = 3, 2, 40, 0.45
SENTINEL = 0x5A5B


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@pytest.fixture(scope="module")
def B():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import bp_decoding
    return bp_decoding


def reference_table(p, adj16):
    """uint16 [T, nk, dc] from the rows alone: edge i of VN (q, t) with local CN l puts socket dv*t + i into the set of CN
    (q + i) * cns_pos + l; every CN's sockets ascending, 0xFFFF behind them.  Also the CNs' degrees [T, nk]."""
    a = np.ascontiguousarray(adj16).view(np.uint16).astype(np.int64).reshape(-1, p.n, p.dv)
    q, t, i = np.arange(p.n) // p.vns_pos, np.arange(p.n) % p.vns_pos, np.arange(p.dv)
    sock = (p.dv * t[:, None] + i[None, :]).ravel()
    out = np.full((a.shape[0], p.nk, p.dc), 0xFFFF, dtype=np.uint16)
    deg = np.zeros((a.shape[0], p.nk), dtype=np.int64)
    for k in range(a.shape[0]):
        assert a[k].max() < p.cns_pos
        cn = ((q[:, None] + i[None, :]) * p.cns_pos + a[k]).ravel()
        order = np.lexsort((sock, cn))
        cn_s, sock_s = cn[order], sock[order]
        start = np.searchsorted(cn_s, np.arange(p.nk))
        place = np.arange(cn_s.size) - start[cn_s]
        assert place.max() < p.dc
        out[k, cn_s, place] = sock_s
        deg[k] = np.bincount(cn, minlength=p.nk)
    return out, deg


def check_sampler(E, p, doped):
    """One table-mode launch of T trials into buffers of T + 1: the checks of this file's head."""
    import torch
    assert E.sample_philox_sock_supported(p)
    adj = torch.full((T + 1, p.n, p.dv), SENTINEL, dtype=torch.int16, device="cuda:0")
    cn = torch.full((T + 1, p.nk, p.dc), SENTINEL, dtype=torch.int16, device="cuda:0")
    ch = torch.full((T + 1, p.nw), SENTINEL, dtype=torch.int32, device="cuda:0")
    E.sample_philox_sock(p, SEED, TRIAL0, T, EPS, doped, out=(adj[:T], cn[:T], ch[:T]))
    ref_adj, ref_ch = E.sample_philox(p, SEED, TRIAL0, T, EPS, doped, adj16=True)
    torch.cuda.synchronize()
    for buf in (adj, cn, ch):                                            # nothing past the T trials
        assert bool((buf[T] == SENTINEL).all())
    assert torch.equal(adj[:T], ref_adj) and torch.equal(ch[:T], ref_ch)     # bit for bit the table-less launch
    want, deg = reference_table(p, ref_adj.cpu().numpy())
    got = np.sort(cn[:T].cpu().numpy().view(np.uint16), axis=-1)         # a set per CN: ascending, 0xFFFF last
    assert ((got == 0xFFFF).sum(axis=-1) == p.dc - deg).all()
    assert (got == want).all(), np.argwhere(got != want)[:4]
    assert deg.min() < p.dc and deg.max() == p.dc                        # the shape has chain-end CNs and full ones
    return adj[:T], cn[:T], ch[:T]


SMALL = [(3, 6, 8, 50),         # S = 150: S % 4 = 2, one row
         (5, 10, 12, 200),      # S = 1000
         (3, 9, 7, 60),         # dc neither a power of two nor 2 * dv
         (4, 8, 6, 600),        # S = 2400, four rows
         (3, 6, 6, 1400),       # S = 4200: two Philox calls per thread
         (4, 8, 5, 2048),       # S = 8192, the edge
         (4, 8, 4, 64)]         # L = dv: every CN position lacks some VN position


@pytest.mark.parametrize("doped", [(), (2,)])
@pytest.mark.parametrize("dv,dc,L,N", SMALL)
def test_small_kernel_writes_the_table_with_the_code(E, dv, dc, L, N, doped):
    p = E.make_params(dv, dc, L, N)
    assert p.cns_pos * dc <= 8192
    check_sampler(E, p, doped)


BIG = [(4, 8, 5, 2050),         # S = 8200, the first big size
       (3, 6, 5, 2734),         # S = 8202, S % 4 = 2
       (5, 10, 6, 2500),
       (4, 8, 5, 5000)]         # the shipped size


@pytest.mark.parametrize("path", ["fused", "nibble", "wide", "nibble+wide"])
@pytest.mark.parametrize("dv,dc,L,N", BIG)
def test_big_kernel_writes_the_table_through_every_ranking(E, monkeypatch, dv, dc, L, N, path):
    """Fused in LDS (the table is the stage), nibble-wide counters (SCLDPC_DEBUG_SAMPLER_FUSED=0) and the 16-bit-counter
    fallback of either (forced: SCLDPC_DEBUG_SAMPLER_WIDE), the last three building the table from the finished row."""
    if "nibble" in path:
        monkeypatch.setenv("SCLDPC_DEBUG_SAMPLER_FUSED", "0")
    if "wide" in path:
        monkeypatch.setenv("SCLDPC_DEBUG_SAMPLER_WIDE", "1")
    p = E.make_params(dv, dc, L, N)
    assert p.cns_pos * dc > 8192
    check_sampler(E, p, (2,) if path == "fused" else ())


def _same(torch, ref, out, what):
    assert torch.equal(ref["counters"], out["counters"]), (what, ref["counters"][:4], out["counters"][:4])
    if ref.get("rows") is not None:
        its = ref["counters"][:, 5].long()
        live = (torch.arange(ref["rows"].shape[1], device=its.device)[None, :] < its[:, None])[:, :, None]
        assert torch.equal(ref["rows"] * live, out["rows"] * live), what
    if ref.get("erased") is not None:
        assert torch.equal(ref["erased"], out["erased"]), what


def _both_tables(E, p, ntrials, eps):
    import torch
    a, cs, ch = E.sample_philox_sock(p, SEED, TRIAL0, ntrials, eps)
    ref = E.cn_sockets(p, a)
    torch.cuda.synchronize()
    return a, cs, ref, ch


def test_full_bp_deg_decodes_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(3, 6, 12, 200)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    for rows_cap in (0, 64):
        kw = dict(max_it=50, rows_cap=rows_cap, want_erased=True)
        _same(torch, E.full_bp_deg(p, a, ref, ch, **kw), E.full_bp_deg(p, a, cs, ch, **kw), ("full_bp_deg", rows_cap))


def test_full_bp_wide_with_rows_decodes_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(4, 8, 24, 5000)
    assert p.nk == 67500 and E.full_bp_wide_supported(p)
    a, cs, ref, ch = _both_tables(E, p, 2, 0.44)
    kw = dict(max_it=200, is_term=False, rows_cap=256)
    out_ref, out = E.full_bp_wide(p, a, ref, ch, **kw), E.full_bp_wide(p, a, cs, ch, **kw)
    assert int(out_ref["counters"][:, 5].min()) > 1                      # there are rows to compare
    _same(torch, out_ref, out, "full_bp_wide")


def test_ring_window_decoders_decode_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(5, 10, 16, 200)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    kw = dict(want_erased=True, ring=True, deg=True)
    _same(torch, E.sw_bp(p, a, ch, 5, 20, d_cn_sock=ref, **kw), E.sw_bp(p, a, ch, 5, 20, d_cn_sock=cs, **kw), "sw_ring deg")
    p = E.make_params(4, 8, 16, 2500)                                    # 10 000 sockets per position: the big kernel's table
    assert E.swc_ring_supported(p, 5) and E.sw_ring_supported(p, 5)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    kw = dict(want_erased=True, classical=True, ring=True)
    _same(torch, E.sw_bp(p, a, ch, 5, 20, d_cn_sock=ref, **kw), E.sw_bp(p, a, ch, 5, 20, d_cn_sock=cs, **kw), "swc_ring")
    kw = dict(want_erased=True, ring=True)                               # the square ring whose table sw_bp builds per call today
    _same(torch, E.sw_bp(p, a, ch, 5, 20, **kw), E.sw_bp(p, a, ch, 5, 20, d_cn_sock=cs, **kw), "sw_ring (4,8)")


def test_cli_writes_the_same_file_with_the_sampled_table(B, tmp_path, capfd):
    texts = {}
    for mode in ("on", "off"):
        d = tmp_path / mode
        capfd.readouterr()
        B.bp_lim_iter(["0", "0", "0", "200", "--dv", "3", "--dc", "6", "--N", "200", "--L", "16", "--eps-ini", "0.47",
                       "--num-points", "2", "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5",
                       "--deg", "on", "--sampled-table", mode, "--outdir", str(d)])
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "kernels:" in ln]
        assert len(lines) == 1, lines
        tail = " + full_bp_small level-synchronous (4-bit CN counts, dv = 3, dc = 6)"
        assert (("sampler (first generation, CN->socket table)" if mode == "on" else
                 "sampler (first generation) + cn_sockets pass") + tail) in lines[0], lines[0]
        files = sorted(os.listdir(d))
        assert len(files) == 1
        texts[mode] = open(d / files[0], "rb").read()
    assert texts["on"] == texts["off"] and len(texts["on"]) > 100
