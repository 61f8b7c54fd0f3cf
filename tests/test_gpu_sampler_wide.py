"""The second-generation sampler beyond 8192 sockets per CN position (-m gpu): sample_philox_wide_sock16 against the
first-generation sampler (rows and channel words bit for bit those of sample_philox(adj16=True)) and against a numpy inversion
of the reference rows (neither the cn_sockets pass nor the code under test), nothing written past the T trials asked for —
through three, four and five Philox calls per thread, S % 4 = 2, the chain ends, every ranking (the parts' histograms, the exact
fallback, a part over its capacity), the decoders that consume the table, and the command line.  Integer work: no tolerance
anywhere."""
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


def launch(E, p, doped, trial0=TRIAL0, table=True):
    """One launch of T trials into buffers of T + 1 filled with a sentinel: (rows, table, channel) with the extra trial."""
    import torch
    assert E.wide_sock16_supported(p)
    adj = torch.full((T + 1, p.n, p.dv), SENTINEL, dtype=torch.int16, device="cuda:0")
    cn = torch.full((T + 1, p.nk, p.dc), SENTINEL, dtype=torch.int16, device="cuda:0")
    ch = torch.full((T + 1, p.nw), SENTINEL, dtype=torch.int32, device="cuda:0")
    E.sample_philox_wide_sock16(p, SEED, trial0, T, EPS, doped, out=(adj[:T], cn[:T] if table else None, ch[:T]))
    torch.cuda.synchronize()
    return adj, cn, ch


def sets(cn):
    """The table as a set per CN: every CN's entries ascending, 0xFFFF last."""
    return np.sort(cn.cpu().numpy().view(np.uint16), axis=-1)


def check_sampler(E, p, doped, trial0=TRIAL0):
    """The checks of this file's head for one launch."""
    import torch
    adj, cn, ch = launch(E, p, doped, trial0)
    ref_adj, ref_ch = E.sample_philox(p, SEED, trial0, T, EPS, doped, adj16=True)
    torch.cuda.synchronize()
    for buf in (adj, cn, ch):                                            # nothing past the T trials
        assert bool((buf[T] == SENTINEL).all())
    assert torch.equal(adj[:T], ref_adj)                                 # bit for bit the first generation
    assert torch.equal(ch[:T], ref_ch)
    want, deg = reference_table(p, ref_adj.cpu().numpy())
    got = sets(cn[:T])
    assert ((got == 0xFFFF).sum(axis=-1) == p.dc - deg).all()
    assert (got == want).all(), np.argwhere(got != want)[:4]
    assert deg.min() < p.dc and deg.max() == p.dc                        # the shape has chain-end CNs and full ones
    # the same rows and channel without the table
    adj0, cn0, ch0 = launch(E, p, doped, trial0, table=False)
    assert torch.equal(adj0, adj) and torch.equal(ch0, ch)
    assert bool((cn0 == SENTINEL).all())
    return adj[:T], cn[:T], ch[:T]


SHAPES = [(4, 8, 5, 2050),      # S = 8200, the lower edge, three calls
          (3, 6, 4, 2734),      # S = 8202, S % 4 = 2
          (5, 10, 6, 1642),     # S = 8210, S % 4 = 2
          (4, 8, 5, 3072),      # S = 12288, the three-call edge
          (4, 8, 5, 3074),      # S = 12296, four calls
          (4, 8, 5, 4096),      # S = 16384
          (4, 8, 5, 4098),      # S = 16392, five calls
          (4, 8, 5, 5120),      # S = 20480, the upper edge
          (3, 6, 4, 6826),      # S = 20478, S % 4 = 2, the most VNs per thread
          (5, 10, 6, 4094),     # S = 20470, S % 4 = 2
          (3, 6, 3, 2800),      # L = dv: every CN position lacks some VN position
          (5, 10, 5, 1700)]


@pytest.mark.parametrize("doped", [(), (2,)])
@pytest.mark.parametrize("dv,dc,L,N", SHAPES)
def test_bit_for_bit_the_first_generation(E, dv, dc, L, N, doped):
    p = E.make_params(dv, dc, L, N)
    assert 8192 < p.cns_pos * dc <= 20480
    check_sampler(E, p, doped)


def test_the_shipped_size(E):
    check_sampler(E, E.make_params(4, 8, 50, 5000), ())


def test_the_high_word_of_the_trial_counter(E):
    check_sampler(E, E.make_params(4, 8, 5, 2050), (), trial0=2**32 + 7)


@pytest.fixture(scope="module")
def plain(E):
    """The plain launch of the shapes of test_every_ranking, checked once: (rows, table as sets, channel) by shape."""
    out = {}
    for shape in [(4, 8, 5, 2050), (3, 6, 4, 2734)]:
        adj, cn, ch = check_sampler(E, E.make_params(*shape), ())
        out[shape] = (adj, sets(cn), ch)
    return out


# -2: the exact fallback at every position; 2: at one position; a part capacity of 1024 is below a part's count (all S > 8192
# keys of a position here, half of them beyond 12288 sockets), so every position finds its first part over capacity and takes
# the fallback from there
@pytest.mark.parametrize("name,value", [("SCLDPC_DEBUG_SAMPLER_EXACT_POS", "-2"), ("SCLDPC_DEBUG_SAMPLER_EXACT_POS", "2"),
                                        ("SCLDPC_DEBUG_SAMPLER_PART_CAP", "1024")])
@pytest.mark.parametrize("dv,dc,L,N", [(4, 8, 5, 2050), (3, 6, 4, 2734)])
def test_every_ranking(E, plain, monkeypatch, dv, dc, L, N, name, value):
    """Every way to rank a position gives the rows, channel and table set of the plain launch."""
    import torch
    adj, want, ch = plain[(dv, dc, L, N)]
    monkeypatch.setenv(name, value)
    a2, c2, h2 = launch(E, E.make_params(dv, dc, L, N), ())
    for buf in (a2, c2, h2):
        assert bool((buf[T] == SENTINEL).all())
    assert torch.equal(a2[:T], adj) and torch.equal(h2[:T], ch)
    assert (sets(c2[:T]) == want).all()


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
    a, cs, ch = E.sample_philox_wide_sock16(p, SEED, TRIAL0, ntrials, eps)
    ref = E.cn_sockets(p, a)
    torch.cuda.synchronize()
    return a, cs, ref, ch


def test_full_bp_wide_decodes_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(4, 8, 12, 2400)
    assert E.full_bp_wide_supported(p)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    for rows_cap in (0, 64):
        kw = dict(max_it=50, rows_cap=rows_cap, want_erased=True)
        _same(torch, E.full_bp_wide(p, a, ref, ch, **kw), E.full_bp_wide(p, a, cs, ch, **kw), ("full_bp_wide", rows_cap))


def test_full_bp_deg_wide_decodes_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(3, 6, 12, 3000)
    assert E.full_bp_deg_supported(p, wide=True)
    a, cs, ref, ch = _both_tables(E, p, T, 0.40)
    for rows_cap in (0, 64):
        kw = dict(max_it=50, rows_cap=rows_cap, want_erased=True, wide=True)
        _same(torch, E.full_bp_deg(p, a, ref, ch, **kw), E.full_bp_deg(p, a, cs, ch, **kw), ("full_bp_deg wide", rows_cap))


def test_ring_window_decoder_decodes_the_same_from_the_sampled_table(E):
    import torch
    p = E.make_params(4, 8, 16, 2400)
    assert E.sw_ring_supported(p, 5)
    a, cs, ref, ch = _both_tables(E, p, T, 0.44)
    kw = dict(want_erased=True, ring=True)
    _same(torch, E.sw_bp(p, a, ch, 5, 20, d_cn_sock=ref, **kw), E.sw_bp(p, a, ch, 5, 20, d_cn_sock=cs, **kw), "sw_ring")


def _cli_pair(prog, argv, tmp_path, capfd, lines_want, nfiles):
    texts = {}
    for mode in ("on", "off"):
        d = tmp_path / mode
        capfd.readouterr()
        prog(argv + ["--sampler2-wide", mode, "--outdir", str(d)])
        lines = [ln for ln in capfd.readouterr().err.split("\n") if "kernels:" in ln]
        assert len(lines) == 1, lines
        assert lines_want[mode] in lines[0], lines[0]
        files = sorted(os.listdir(d))                                    # (bp_traj writes one file per ε point)
        assert len(files) == nfiles, files
        texts[mode] = {name: open(d / name, "rb").read() for name in files}
    assert texts["on"] == texts["off"] and all(len(t) > 100 for t in texts["on"].values())


def test_cli_bp_traj_writes_the_same_file_with_the_wide_sampler(B, tmp_path, capfd):
    _cli_pair(B.bp_traj,
              ["0", "0", "0", "200", "0", "--N", "2400", "--L", "12", "--eps-ini", "0.47", "--num-points", "2",
               "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5"], tmp_path, capfd,
              {"on": "sampler_v2 wide (dv = 4, dc = 8, CN->socket table) + ",
               "off": "sampler (first generation) + cn_sockets pass + "}, nfiles=2)


def test_cli_window_decoder_writes_the_same_file_with_the_wide_sampler(B, tmp_path, capfd):
    # (no --ring on: the (4,8) chain takes its ring decoder without that switch, which belongs to the pairs (3,6) and (5,10)
    # and exits when given with dv = 4, dc = 8; the kernels: line shows that the ring decoder runs)
    _cli_pair(B.sw_lim_iter,
              ["0", "5", "0", "20", "60", "--N", "2400", "--L", "16", "--eps-ini", "0.47", "--num-points", "2",
               "--max-frames", "64", "--min-frame-err", "64", "--batch", "32", "--seed", "5"], tmp_path, capfd,
              {"on": "sampler_v2 wide (dv = 4, dc = 8, CN->socket table) + sw_ring (window state in LDS)",
               "off": "sampler (first generation) + sw_ring + cn_sockets pass"}, nfiles=1)
