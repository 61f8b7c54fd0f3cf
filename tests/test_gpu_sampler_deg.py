"""The second-generation sampler of the pairs (3,6) and (5,10) (-m gpu): sample_philox_deg_sock16 against the first-generation
sampler (rows and channel words bit for bit those of sample_philox(adj16=True)) and against a numpy inversion of the reference
rows (neither the cn_sockets pass nor the code under test), nothing written past the T trials asked for — through every
instance, S % 4 = 2, the chain ends, the exact fallback, the decoders that consume the table, and the command line.  Integer
work: no tolerance anywhere."""
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


def launch(E, p, doped, trial0=TRIAL0):
    """One launch of T trials into buffers of T + 1 filled with a sentinel: (rows, table, channel) with the extra trial."""
    import torch
    assert E.deg_sock16_supported(p)
    adj = torch.full((T + 1, p.n, p.dv), SENTINEL, dtype=torch.int16, device="cuda:0")
    cn = torch.full((T + 1, p.nk, p.dc), SENTINEL, dtype=torch.int16, device="cuda:0")
    ch = torch.full((T + 1, p.nw), SENTINEL, dtype=torch.int32, device="cuda:0")
    E.sample_philox_deg_sock16(p, SEED, trial0, T, EPS, doped, out=(adj[:T], cn[:T], ch[:T]))
    torch.cuda.synchronize()
    return adj, cn, ch


# The first-generation sampler keeps a ring of dv rows of S ids in LDS and refuses this shape (164 976 bytes of LDS for the
# 160 KiB a CU has), so there is no sample_philox(adj16=True) to compare with: its rows and channel words come from the CPU
# twin of that sampler (oracle.sample_philox: the same law and keys, which every device sampler equals bit for bit).
TWIN_ONLY = [(5, 10, 7, 1638)]


def reference_code(E, p, doped, trial0, oracle):
    """(rows int16 [T,n,dv], channel int32 [T,nw]) of sample_philox(adj16=True), on the device."""
    import torch
    if (p.dv, p.dc, p.L, p.vns_pos) not in TWIN_ONLY:
        return E.sample_philox(p, SEED, trial0, T, EPS, doped, adj16=True)
    with pytest.raises(E.ScldpcError, match="of LDS"):                   # (the day it takes the shape, compare with it)
        E.sample_philox(p, SEED, trial0, T, EPS, doped, adj16=True)
    po = oracle.Params(p.dv, p.dc, p.L, p.cns_pos, p.vns_pos)
    twin = [oracle.sample_philox(po, SEED, trial0 + t, EPS, doped) for t in range(T)]
    adj = np.stack([E.global_to_adj16(p, a) for a, _ in twin]).view(np.int16)
    ch = np.stack([c for _, c in twin]).view(np.int32)
    return torch.from_numpy(adj).to("cuda:0"), torch.from_numpy(ch).to("cuda:0")


def check_sampler(E, p, doped, trial0=TRIAL0, oracle=None):
    """The checks of this file's head for one launch."""
    import torch
    adj, cn, ch = launch(E, p, doped, trial0)
    ref_adj, ref_ch = reference_code(E, p, doped, trial0, oracle)
    torch.cuda.synchronize()
    for buf in (adj, cn, ch):                                            # nothing past the T trials
        assert bool((buf[T] == SENTINEL).all())
    assert torch.equal(adj[:T], ref_adj)                                 # bit for bit the first generation
    assert torch.equal(ch[:T], ref_ch)
    want, deg = reference_table(p, ref_adj.cpu().numpy())
    got = np.sort(cn[:T].cpu().numpy().view(np.uint16), axis=-1)         # a set per CN: ascending, 0xFFFF last
    assert ((got == 0xFFFF).sum(axis=-1) == p.dc - deg).all()
    assert (got == want).all(), np.argwhere(got != want)[:4]
    assert deg.min() < p.dc and deg.max() == p.dc                        # the shape has chain-end CNs and full ones
    # the same rows and channel without the table
    adj0 = torch.full_like(adj, SENTINEL)
    ch0 = torch.full_like(ch, SENTINEL)
    E.sample_philox_deg_sock16(p, SEED, trial0, T, EPS, doped, out=(adj0[:T], None, ch0[:T]))
    torch.cuda.synchronize()
    assert torch.equal(adj0, adj) and torch.equal(ch0, ch)
    return adj[:T], cn[:T], ch[:T]


SHAPES = [(3, 6, 8, 52),        # S = 156, one histogram row
          (3, 6, 8, 50),        # S = 150, S % 4 = 2
          (5, 10, 7, 50),       # S = 250, S % 4 = 2
          (5, 10, 12, 200),     # S = 1000
          (5, 10, 5, 818),      # S = 4090, the one-call edge
          (5, 10, 5, 820),      # S = 4100, two calls
          (3, 6, 6, 1400),      # S = 4200, two VNs per thread
          (3, 6, 5, 2730),      # S = 8190, three VNs per thread, the edge
          (5, 10, 7, 1638),     # S = 8190, the LDS edge
          (3, 6, 3, 64),        # L = dv: every CN position lacks some VN position
          (5, 10, 5, 64),
          (3, 6, 50, 1000),     # the shipped size
          (5, 10, 50, 1000)]


@pytest.mark.parametrize("doped", [(), (2,)])
@pytest.mark.parametrize("dv,dc,L,N", SHAPES)
def test_bit_for_bit_the_first_generation(E, oracle, dv, dc, L, N, doped):
    p = E.make_params(dv, dc, L, N)
    assert p.cns_pos * dc <= 8192
    check_sampler(E, p, doped, oracle=oracle)


def test_the_high_word_of_the_trial_counter(E):
    check_sampler(E, E.make_params(3, 6, 8, 50), (), trial0=2**32 + 7)


@pytest.mark.parametrize("dv,dc,L,N", [(3, 6, 6, 1400), (5, 10, 6, 200)])
def test_every_ranking(E, monkeypatch, dv, dc, L, N):
    """The exact fallback at every position (-2) and at one position (2) ranks as the histogram does."""
    import torch
    p = E.make_params(dv, dc, L, N)
    adj, cn, ch = check_sampler(E, p, ())
    want = np.sort(cn.cpu().numpy().view(np.uint16), axis=-1)
    for forced in ("-2", "2"):
        monkeypatch.setenv("SCLDPC_DEBUG_SAMPLER_EXACT_POS", forced)
        a2, c2, h2 = launch(E, p, ())
        for buf in (a2, c2, h2):
            assert bool((buf[T] == SENTINEL).all())
        assert torch.equal(a2[:T], adj) and torch.equal(h2[:T], ch), forced
        assert (np.sort(c2[:T].cpu().numpy().view(np.uint16), axis=-1) == want).all(), forced


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
    a, cs, ch = E.sample_philox_deg_sock16(p, SEED, TRIAL0, ntrials, eps)
    ref = E.cn_sockets(p, a)
    torch.cuda.synchronize()
    return a, cs, ref, ch


def test_full_bp_deg_forms_decode_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(3, 6, 12, 200)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    for rows_cap in (0, 64):
        kw = dict(max_it=50, rows_cap=rows_cap, want_erased=True)
        _same(torch, E.full_bp_deg(p, a, ref, ch, **kw), E.full_bp_deg(p, a, cs, ch, **kw), ("full_bp_deg", rows_cap))
    kw = dict(want_erased=True)
    _same(torch, E.full_bp_fixpoint_deg(p, a, ref, ch, **kw), E.full_bp_fixpoint_deg(p, a, cs, ch, **kw), "full_bp_fixpoint_deg")
    caps = (5, 20, 50)
    assert torch.equal(E.full_bp_caps_deg(p, a, ref, ch, caps), E.full_bp_caps_deg(p, a, cs, ch, caps))


def test_ring_window_decoders_decode_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(5, 10, 16, 200)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    kw = dict(want_erased=True, ring=True, deg=True)
    _same(torch, E.sw_bp(p, a, ch, 5, 20, d_cn_sock=ref, **kw), E.sw_bp(p, a, ch, 5, 20, d_cn_sock=cs, **kw), "sw_ring deg")
    kw = dict(want_erased=True, classical=True, ring=True)
    _same(torch, E.sw_bp(p, a, ch, 5, 20, d_cn_sock=ref, **kw), E.sw_bp(p, a, ch, 5, 20, d_cn_sock=cs, **kw), "swc_ring")


def _cli_pair(prog, argv, tmp_path, capfd, lines_want):
    texts = {}
    for mode in ("on", "off"):
        d = tmp_path / mode
        capfd.readouterr()
        prog(argv + ["--sampler2", mode, "--outdir", str(d)])
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "kernels:" in ln]
        assert len(lines) == 1, lines
        assert lines_want[mode] in lines[0], lines[0]
        files = sorted(os.listdir(d))
        assert len(files) == 1
        texts[mode] = open(d / files[0], "rb").read()
    assert texts["on"] == texts["off"] and len(texts["on"]) > 100


def test_cli_writes_the_same_file_with_the_second_generation_sampler(B, tmp_path, capfd):
    tail = " + full_bp_small level-synchronous (4-bit CN counts, dv = 3, dc = 6)"
    _cli_pair(B.bp_lim_iter,
              ["0", "0", "0", "200", "--dv", "3", "--dc", "6", "--N", "200", "--L", "16", "--eps-ini", "0.47", "--num-points", "2",
               "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5", "--deg", "on"], tmp_path, capfd,
              {"on": "sampler_v2 (dv = 3, dc = 6, CN->socket table)" + tail,
               "off": "sampler (first generation) + cn_sockets pass" + tail})


def test_cli_window_decoder_writes_the_same_file_with_the_second_generation_sampler(B, tmp_path, capfd):
    tail = " + sw_ring (window state in LDS, dv = 5, dc = 10)"
    _cli_pair(B.sw_lim_iter,
              ["0", "5", "0", "20", "60", "--dv", "5", "--dc", "10", "--N", "200", "--L", "16", "--eps-ini", "0.47", "--num-points", "2",
               "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5", "--ring", "on"], tmp_path, capfd,
              {"on": "sampler_v2 (dv = 5, dc = 10, CN->socket table)" + tail,
               "off": "sampler (first generation) + cn_sockets pass" + tail})
