"""Several iteration caps from one decode on the GPU (-m gpu): scldpc_full_bp_caps_device_{cn16,sock16} against the
single-cap decoder counter for counter, against the reference's capped fixtures, through `bp_lim_iter --caps` against
single-cap runs file for file, and against the published BP_Full_{175..350}it tables from one decode per ε row."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden, require_gpu

pytestmark = pytest.mark.gpu

CAP_SETS = [(1,), (3, 5), (175, 200, 250, 300, 350), (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597),
            (40, 1000000)]


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


@pytest.mark.parametrize("caps", CAP_SETS, ids=lambda c: "caps%d_%d" % (len(c), c[-1]))
@pytest.mark.parametrize("is_term", [True, False])
@pytest.mark.parametrize("L,N,sockets", [(50, 1000, False), (20, 200, False), (20, 200, True), (100, 1000, True)])
def test_every_cap_equals_the_single_cap_decoder(E, L, N, sockets, is_term, caps):
    """Block k of one fused decode == full_bp_cn16(max_it = caps[k]) on all eight counters of every trial, on Philox batches
    from ε = 0.40 (frames done before the first cap) to 0.50 (above threshold), both table forms, n >= 65 535 included."""
    import torch
    p = E.make_params(4, 8, L, N)
    T = 64
    its = []
    for i, eps in enumerate((0.40, 0.45, 0.47, 0.48, 0.50)):
        a, tab, ch = (E.sample_philox_sock16 if sockets else E.sample_philox_cn16)(p, 91, 1000 * i, T, eps)
        got = E.full_bp_caps_cn16(p, a, tab, ch, caps, is_term=is_term, sockets=sockets)
        assert tuple(got.shape) == (len(caps), T, E.NCOUNTERS)
        for k, cap in enumerate(caps):
            ref = E.full_bp_cn16(p, a, tab, ch, max_it=cap, is_term=is_term, sockets=sockets)["counters"]
            torch.cuda.synchronize()
            g, r = got[k].cpu().numpy(), ref.cpu().numpy()
            assert (g == r).all(), (L, N, sockets, is_term, eps, cap, np.argwhere(g != r)[:4].tolist())
        its.append(got[-1, :, 5].cpu().numpy())
    its = np.concatenate(its)
    if (L, caps[0]) == (50, 175):
        assert (its < caps[0]).any() and (its >= caps[-1]).any()      # frames on both sides of the cap range


def _capped_fixtures():
    return [n for n in golden_names(prefixes=("c2_", "mid_", "tiny_"), variants=("bpf", "bpt")) if load_golden(n).max_it]


@pytest.mark.parametrize("name", _capped_fixtures())
def test_caps_on_the_reference_fixtures(E, name):
    """The reference's own graphs and channels with a binding MAX_IT (glibc replay, CN -> VN table built on the host): the
    fused decode with caps around g.max_it gives the fixture's counters at that cap; an uncapped fixture drawn on the same
    seeds is matched by the 10^6 cap of the same call."""
    import torch
    g = load_golden(name)
    m = g.meta
    p = E.make_params(m["dv"], m["dc"], m["L"], m["VNsPos"])
    T = min(g.T, 16 if p.n > 10000 else 64)
    adj, ch = E.sample_glibc_trials(p, g["seed"][:T], m["eps"])
    a16 = E.global_to_adj16(p, adj)
    d_a, d_ch = E.to_device(a16, ch)
    d_cn = torch.from_numpy(E.cn_adj_from_vn_adj(p, a16)).to(d_a.device)
    caps = sorted({max(1, g.max_it - 1), g.max_it, 2 * g.max_it + 1, 1000000})
    twins = [load_golden(n) for n in golden_names(prefixes=(name.split("_")[0] + "_",), variants=(m["variant"],))
             if not load_golden(n).max_it]
    twins = [u for u in twins if u.meta["is_term"] == m["is_term"] and u.meta["eps"] == m["eps"] and u.meta["L"] == m["L"]
             and u.meta["VNsPos"] == m["VNsPos"] and u.T >= T and (u["seed"][:T] == g["seed"][:T]).all()]
    for sockets, tab in ((False, d_cn), (True, E.cn_sockets(p, d_a))):
        c = E.full_bp_caps_cn16(p, d_a, tab, d_ch, caps, is_term=bool(m["is_term"]), sockets=sockets)
        torch.cuda.synchronize()
        c = c.cpu().numpy()
        for fx, k in [(g, caps.index(g.max_it))] + [(u, len(caps) - 1) for u in twins]:
            for col, key in ((0, "ne"), (1, "be"), (2, "ee"), (3, "bee"), (7, "nch")):
                assert (c[k, :, col] == fx[key][:T]).all(), (name, fx.name, sockets, key)
            assert (c[k, :, 6] == 0).all() and (c[k, :, 4] == 0).all()
            if fx.has("rows"):
                assert [int(x) for x in c[k, :, 5]] == [len(fx.rows_of(t)) for t in range(T)], (name, fx.name)


def _cli(outdir, argv):
    r = subprocess.run([sys.executable, "-m", "fl_scaling_sc_ldpc_amd.bp_decoding", "bp_lim_iter"] + argv +
                       ["--outdir", str(outdir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _files(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("extra,path", [([], "with 5 cap checkpoints per decode"),
                                        (["--dv", "3", "--dc", "6"], "single-cap passes one after another"),
                                        (["--rng", "glibc", "--N", "40", "--max-frames", "300"],
                                         "single-cap passes one after another")])
def test_cli_caps_write_the_single_cap_files(tmp_path, extra, path):
    require_gpu()
    argv = ["--L", "20", "--N", "200", "--num-points", "3", "--min-frame-err", "50", "--max-frames", "4096", "--seed", "5",
            "--batch", "1024"] + extra
    log = _cli(tmp_path / "caps", ["0", "0", "0", "350", "--caps", "175,200,250,300"] + argv)
    assert path in log, log
    got = _files(tmp_path / "caps")
    assert len(got) == 5
    for cap in (175, 200, 250, 300, 350):
        d = tmp_path / ("one%d" % cap)
        _cli(d, ["0", "0", "0", str(cap), "--quiet"] + argv)
        (name, text), = _files(d).items()
        assert got[name] == text, (cap, extra)


def test_one_fused_pass_reproduces_the_published_capped_tables(E):
    """bp_lim_iter at (4,8,L=50,Def_M=500) with MAX_IT 175 … 350 (the published BP_Full_*it family): ONE decode per ε row
    with the five caps, every cap's counters against its own table with test_gpu_published_curves' z-test."""
    import torch
    from test_gpu_published_curves import SIGMAS, _Acc, _compare, _pick, _risultati
    caps = (175, 200, 250, 300, 350)
    p = E.make_params(4, 8, 50, 1000)
    B, T = 16384, 65536
    a = torch.empty((B, p.n, 4), dtype=torch.int16, device="cuda")
    cn = torch.empty((B, p.nk, 8), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")
    cnt = torch.empty((len(caps), B, E.NCOUNTERS), dtype=torch.int32, device="cuda")
    tables = {cap: {round(r["eps"], 6): r for r in _pick(_risultati(f"SC_LDPC_4_8_L50_M500_BP_Full_{cap}it_BEC.dat"), lo=0.02)}
              for cap in caps}
    grid = sorted(set().union(*[set(t) for t in tables.values()]))
    assert len(grid) >= 5
    zs = {cap: [] for cap in caps}
    for i, eps in enumerate(grid):
        accs = [_Acc() for _ in caps]
        for b0 in range(0, T, B):
            E.sample_philox_cn16(p, 9100, (i << 24) + b0, B, eps, out=(a, cn, ch))
            E.full_bp_caps_cn16(p, a, cn, ch, caps, counters=cnt)
            for k in range(len(caps)):
                accs[k].add(cnt[k])
            assert int(cnt[:, :, 6].min().item()) == 0
        for k, cap in enumerate(caps):
            if eps in tables[cap]:
                zs[cap].append(_compare(accs[k], tables[cap][eps], f"BP_Full_{cap}it (fused)"))
    for cap in caps:
        assert len(zs[cap]) >= 3, (cap, zs[cap])
        assert abs(np.mean(zs[cap])) < SIGMAS / np.sqrt(len(zs[cap])) + 0.5, (cap, zs[cap])
