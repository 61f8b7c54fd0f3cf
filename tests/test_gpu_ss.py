"""The stopping-set spectrum on the GPU (-m gpu): scldpc_ss_spectrum_device (ss_spectrum.hip) against pd_oracle.components /
sc_ldpc_trial_stats with the bins formed in numpy (test_ss_host.np_spectrum).  Graphs come from the CPU twin
oracle.sample_philox and are uploaded, so nothing here leans on a device sampler except items 6 and 7, which run behind the
decoders.  Every comparison is exact integer equality; every shape runs with its state in LDS and in the workspace (the debug
switch) unless it is in the workspace anyway.  The code under test is never a reference."""
import ctypes as C

import numpy as np
import pytest

from conftest import require_gpu
from test_ss_host import FORCE, np_spectrum, np_spectrum_batch

pytestmark = pytest.mark.gpu
NBINS = 256
# name -> (dv, dc, L, M, rho, ensemble, trials)
SHAPES = {
    "3-6-olmos": (3, 6, 10, 128, 0.09, "olmos", 8), "4-8-olmos": (4, 8, 10, 96, 0.06, "olmos", 8),
    "5-10-olmos": (5, 10, 8, 80, 0.03, "olmos", 8), "3-6-tb": (3, 6, 10, 128, 0.09, "tail_biting", 8),
    "3-6-tb-L1": (3, 6, 1, 200, 0.09, "tail_biting", 4),
}
# what the issue found on these inputs with the oracle: (min components per trial, distinct sizes above 2)
FOUND = {"3-6-olmos": (44, 16), "4-8-olmos": (13, 14), "5-10-olmos": (7, 5), "3-6-tb": (39, 16), "3-6-tb-L1": (5, 6)}


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


_graphs, _refs = {}, {}


def graphs(E, oracle, dv, dc, L, M, ens, T):
    """int32 [T, n, dv] from the CPU twin of the sampler, seed 11, trials 0 .. T-1; computed once."""
    key = (dv, dc, L, M, ens, T)
    if key not in _graphs:
        p = E.make_params(dv, dc, L, M)
        po = oracle.Params(dv, dc, L, p.cns_pos, p.vns_pos)
        _graphs[key] = (p, np.stack([oracle.sample_philox(po, 11, t, 0.5, ensemble=ens)[0] for t in range(T)]))
    return _graphs[key]


def members_of(n, rho, T):
    """RandomState(1234).rand(n) < rho, trial after trial from the one stream."""
    rs = np.random.RandomState(1234)
    return np.stack([rs.rand(n) < rho for _ in range(T)])


def reference(key, trs, mem, p, nbins=NBINS):
    """The oracle's sums and rows for these inputs, computed once per key and left unchanged."""
    if key not in _refs:
        _refs[key] = np_spectrum_batch(trs, mem, nbins, p.L, p.vns_pos)
    return _refs[key]


def to_adj16(p, trs):
    """Position-local 2-byte rows of a chain: edge i of a VN of position pos lands in CN position pos + i."""
    pos = (np.arange(p.n) // p.vns_pos)[None, :, None]
    local = trs.astype(np.int64) - (pos + np.arange(p.dv)[None, None, :]) * p.cns_pos
    assert (local >= 0).all() and (local < p.cns_pos).all()
    return local.astype(np.uint16).view(np.int16)


def upload(E, trs, mem):
    import torch
    d_adj = torch.from_numpy(np.ascontiguousarray(trs)).cuda()
    d_m = torch.from_numpy(E.pack_bits(mem.astype(np.uint8)).view(np.int32)).cuda()
    return d_adj, d_m


def run(E, p, d_adj, d_m, nbins=NBINS, **kw):
    import torch
    res = E.ss_spectrum(p, d_adj, d_m, nbins, want_trial=True, **kw)
    torch.cuda.synchronize()
    return res["hist"].cpu().numpy(), res["pos_hist"].cpu().numpy(), res["trial"].cpu().numpy()


def same(what, got, want):
    for name, g, w in zip(("hist", "pos_hist", "trial"), got, want):
        assert g.shape == w.shape and (g == w).all(), (what, name, np.argwhere(g != w)[:4].tolist())


def both_forms(E, monkeypatch, what, p, d_adj, d_m, want, nbins=NBINS, natural=1):
    monkeypatch.delenv(FORCE, raising=False)
    assert E.ss_spectrum_form(p) == natural, what
    same((what, "natural form"), run(E, p, d_adj, d_m, nbins), want)
    if natural == 1:
        monkeypatch.setenv(FORCE, "1")
        assert E.ss_spectrum_form(p) == 2
        same((what, "workspace"), run(E, p, d_adj, d_m, nbins), want)
        monkeypatch.delenv(FORCE)


# ---- 1. random subsets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_subsets(E, oracle, monkeypatch, name):
    dv, dc, L, M, rho, ens, T = SHAPES[name]
    p, trs = graphs(E, oracle, dv, dc, L, M, ens, T)
    mem = members_of(p.n, rho, T)
    want = reference((name, rho), trs, mem, p)
    hist, _, rows = want
    # the conditions the inputs meet, on the reference alone
    assert rows[:, 0].min() == FOUND[name][0] >= 5 and np.count_nonzero(hist[3:]) == FOUND[name][1] >= 5 and hist[NBINS - 1] == 0
    assert hist[0] == 0 and hist[1] > 0 and hist[2] > 0
    d_adj, d_m = upload(E, trs, mem)
    both_forms(E, monkeypatch, name, p, d_adj, d_m, want)
    if ens == "olmos":                                                   # the 2-byte rows give the same
        d_adj16, _ = upload(E, to_adj16(p, trs), mem)
        both_forms(E, monkeypatch, name + " adj16", p, d_adj16, d_m, want)


# ---- 2. giant and mixed ----------------------------------------------------------------------------------------------------------
def test_giant_and_mixed_components(E, oracle, monkeypatch):
    p, trs = graphs(E, oracle, 3, 6, 10, 128, "olmos", 8)
    mem = members_of(p.n, 0.2, 4)
    want = reference("giant-0.2", trs[:4], mem, p)
    assert want[2][:, 1].min() == 234 and want[2][:, 1].max() == 287 and want[0][1] > 0        # giants beside singletons
    d_adj, d_m = upload(E, trs[:4], mem)
    both_forms(E, monkeypatch, "rho 0.2", p, d_adj, d_m, want)
    for nbins in (16, 2):
        w = reference(("giant-0.2", nbins), trs[:4], mem, p, nbins)
        assert w[0][nbins - 1] >= 4 and (w[1] == want[1]).all() and (w[2] == want[2]).all()
        both_forms(E, monkeypatch, "rho 0.2, %d bins" % nbins, p, d_adj, d_m, w, nbins)
    full = np.ones((2, p.n), dtype=bool)
    want = reference("giant-1.0", trs[:2], full, p)
    assert want[2].tolist() == [[1, 1280, 1280, 1280]] * 2 and want[0][255] == 2 and want[1][0, 7] == 2
    d_adj, d_m = upload(E, trs[:2], full)
    both_forms(E, monkeypatch, "rho 1.0", p, d_adj, d_m, want)
    d_adj16, _ = upload(E, to_adj16(p, trs[:2]), full)
    both_forms(E, monkeypatch, "rho 1.0 adj16", p, d_adj16, d_m, want)


# ---- 3. ragged n -----------------------------------------------------------------------------------------------------------------
def test_bits_beyond_n_are_ignored(E, oracle, monkeypatch):
    import torch
    p, trs = graphs(E, oracle, 3, 6, 3, 50, "olmos", 4)
    assert (p.n, p.nw) == (150, 5)
    mem = members_of(p.n, 0.15, 4)
    want = reference("ragged", trs, mem, p)
    assert want[2][:, 0].min() >= 2
    d_adj, d_m = upload(E, trs, mem)
    both_forms(E, monkeypatch, "clear", p, d_adj, d_m, want)
    words = d_m.cpu().numpy().view(np.uint32).copy()
    words[:, -1] |= np.uint32(0xFFC00000)                                # the 10 bits beyond n = 150 = 4 * 32 + 22
    assert (words[:, -1] >> 22 == 0x3FF).all() and (E.unpack_bits(words, p.n).astype(bool) == mem).all()
    both_forms(E, monkeypatch, "set", p, d_adj, torch.from_numpy(words.view(np.int32)).cuda(), want)


# ---- 4. a shape whose state does not fit the LDS ---------------------------------------------------------------------------------
def test_natural_workspace_form(E, oracle, monkeypatch):
    p, trs = graphs(E, oracle, 3, 6, 20, 1500, "olmos", 2)
    assert (p.n, p.nk) == (30000, 16500)
    mem = members_of(p.n, 0.09, 2)
    want = reference("form2-0.09", trs, mem, p)
    assert want[2][:, 0].min() >= 1180 and np.count_nonzero(want[0][3:]) == 32
    d_adj, d_m = upload(E, trs, mem)
    both_forms(E, monkeypatch, "form 2", p, d_adj, d_m, want, natural=2)
    d_adj16, _ = upload(E, to_adj16(p, trs), mem)
    both_forms(E, monkeypatch, "form 2 adj16", p, d_adj16, d_m, want, natural=2)
    full = np.ones((1, p.n), dtype=bool)
    want = reference("form2-1.0", trs[:1], full, p)
    assert want[2].tolist() == [[1, 30000, 30000, 30000]]
    d_adj, d_m = upload(E, trs[:1], full)
    both_forms(E, monkeypatch, "form 2, one component", p, d_adj, d_m, want, natural=2)


# ---- 5. accumulation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True], ids=["lds", "workspace"])
def test_outputs_accumulate_and_an_empty_set_counts_as_a_trial(E, oracle, monkeypatch, force):
    import torch
    if force:
        monkeypatch.setenv(FORCE, "1")
    else:
        monkeypatch.delenv(FORCE, raising=False)
    dv, dc, L, M, rho, ens, T = SHAPES["3-6-olmos"]
    p, trs = graphs(E, oracle, dv, dc, L, M, ens, T)
    mem = members_of(p.n, rho, T)
    mem[5] = False                                                       # one empty trial among the others
    want = reference("accumulate", trs, mem, p)
    assert want[0][0] == 1 and want[2][5].tolist() == [0, 0, 0, 0]
    d_adj, d_m = upload(E, trs, mem)
    base_h = 1000 + np.arange(NBINS, dtype=np.int64)
    base_p = 7 + np.arange(p.L * 8, dtype=np.int64).reshape(p.L, 8)
    one = dict(hist=torch.from_numpy(base_h.copy()).cuda(), pos_hist=torch.from_numpy(base_p.copy()).cuda())
    two = dict(hist=torch.from_numpy(base_h.copy()).cuda(), pos_hist=torch.from_numpy(base_p.copy()).cuda())
    h1, p1, rows1 = run(E, p, d_adj, d_m, **one)
    T1 = 3
    _, _, rows_a = run(E, p, d_adj[:T1], d_m[:T1], **two)
    h2, p2, rows_b = run(E, p, d_adj[T1:], d_m[T1:], **two)
    same("one call", (h1, p1, rows1), (base_h + want[0], base_p + want[1], want[2]))
    same("two calls", (h2, p2, np.concatenate([rows_a, rows_b])), (base_h + want[0], base_p + want[1], want[2]))
    # all-zero members: T to hist[0] and nothing else
    h0, p0, rows0 = run(E, p, d_adj, torch.zeros_like(d_m), **one)
    bump = np.zeros(NBINS, np.int64)
    bump[0] = T
    same("empty", (h0, p0, rows0), (base_h + want[0] + bump, base_p + want[1], np.zeros((T, 4), np.int32)))


# ---- 6. behind the decoders ------------------------------------------------------------------------------------------------------
def oracle_hist(stats, nbins=NBINS):
    hist = np.zeros(nbins, np.int64)
    for st in stats:
        if len(st["sset_sizes"]) == 0:
            hist[0] += 1
        np.add.at(hist, np.minimum(st["sset_sizes"], nbins - 1), 1)
    return hist


_decoded = {}


def decoded(E, name):
    """Per run, once: the sampled tensors, the oracle's per-trial stats on their host copies, the geometry."""
    if name in _decoded:
        return _decoded[name]
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    from oracle import pd_oracle as P
    dv, dc, L, M, e, term, bounded, T = {"terminated": (3, 6, 8, 32, 0.45, True, True, 256),
                                         "widened": (3, 6, 4, 16, 0.45, False, False, 128)}[name]
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p = g.params
    d_adj, d_ch = E.sample_philox(p, 7, 0, T, e, adj16=True)
    A = E.adj16_to_global(p, d_adj.cpu().numpy()).astype(np.int64)
    bits = E.unpack_bits(d_ch.cpu().numpy(), p.n).astype(bool)
    stats = [P.sc_ldpc_trial_stats(A[t], bits[t], dv, dc, L, M, term, bounded) for t in range(T)]
    _decoded[name] = dict(g=g, p=p, T=T, d_adj=d_adj, d_ch=d_ch, A=A, stats=stats)
    return _decoded[name]


@pytest.mark.parametrize("name", ["terminated", "widened"])
def test_behind_the_sweep_decoders(E, monkeypatch, name):
    s = decoded(E, name)
    g, p, T, stats = s["g"], s["p"], s["T"], s["stats"]
    sizes = np.concatenate([st["sset_sizes"] for st in stats])
    if name == "terminated":                                             # checked on the CPU when the issue was written
        assert sum(len(st["sset_sizes"]) > 0 for st in stats) == 91 and len(np.unique(sizes)) == 43 and sizes.max() == 88
    else:
        assert p.L == 44 and {2, 3, 4, 6, 9} <= set(sizes.tolist()) and max((st["sset_sizes"] > 2).sum() for st in stats) == 2
    want_hist = oracle_hist(stats)
    args = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    runs = [("peel_sweep", E.peel_sweep(p, s["d_adj"], s["d_ch"], *args, want_lost=True))]
    runs.append(("peel_sweep_sock16", E.peel_sweep_sock16(p, s["d_adj"], E.cn_sockets(p, s["d_adj"]), s["d_ch"], *args, want_lost=True)))
    for who, res in runs:
        out = res["out"].cpu().numpy()
        lost = E.unpack_bits(res["lost"].cpu().numpy(), p.n).astype(bool)
        want = (want_hist,) + np_spectrum_batch(s["A"], lost, NBINS, p.L, p.vns_pos)[1:]
        assert (want[2][:, 2] == [st["num_lost"] for st in stats]).all() and (want[2][:, 3] == [st["num_lost_exp"] for st in stats]).all()
        both_forms(E, monkeypatch, (name, who), p, s["d_adj"], res["lost"], want)
        assert (want[2][:, 2] == out[:, 0]).all() and (want[2][:, 3] == out[:, 1]).all()       # trial[:, 2:4] == out[:, 0:2]


# ---- 7. the simulator ------------------------------------------------------------------------------------------------------------
SIM = (0.45, 3, 6, 8, 32, True, False, True, False)


def tuples_equal(a, b):
    return len(a) == len(b) == 13 and all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(a, b))


@pytest.mark.parametrize("sweep", ["first", "small"])
def test_the_simulator_counts_the_trials_of_the_tuple(E, sweep):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    kw = dict(num_repeats=300, max_fuckups=20, rng="philox", seed=7, sweep=sweep)
    t13, hist, pos_hist = PD.simulate_sc_ldpc_spectrum(*SIM, batch=64, **kw)
    assert tuples_equal(t13, PD.simulate_sc_ldpc(*SIM, batch=64, **kw))
    o1 = t13[5]
    assert 20 <= o1 < 64                                                 # the stop rule trips inside the first batch
    stats = decoded(E, "terminated")["stats"][:o1]                       # the same seed: trials 0 .. o1-1
    assert sum(st["frame_err"] for st in stats) == 20 == t13[0] * o1
    assert hist.dtype == np.int64 and (hist == oracle_hist(stats)).all() and hist[0] == o1 - 20
    assert pos_hist.shape == (8, 8) and pos_hist.sum() == hist[1:].sum()
    t13b, hist_b, pos_b = PD.simulate_sc_ldpc_spectrum(*SIM, batch=17, **kw)
    assert tuples_equal(t13b, t13) and (hist_b == hist).all() and (pos_b == pos_hist).all()
    _, hist16, _ = PD.simulate_sc_ldpc_spectrum(*SIM, batch=64, nbins=16, **kw)
    assert hist16[:15].tolist() == hist[:15].tolist() and hist16[15] == hist[15:].sum()


def test_the_simulator_on_the_reference_stream(E):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    from oracle import pd_oracle as P
    kw = dict(num_repeats=60, max_fuckups=6, rng="numpy", batch=16)
    np.random.seed(5)
    t13, hist, pos_hist = PD.simulate_sc_ldpc_spectrum(*SIM, **kw)
    np.random.seed(5)
    assert tuples_equal(t13, PD.simulate_sc_ldpc(*SIM, **kw))
    rs, stats, fu = np.random.RandomState(5), [], 0
    while fu < 6 and len(stats) < 60:
        tr, mask = P.sample_trial(rs, 0.45, 3, 6, 8, 32)
        stats.append(P.sc_ldpc_trial_stats(tr, mask, 3, 6, 8, 32, True, True))
        fu += stats[-1]["frame_err"]
    assert fu == 6 and t13[5] == len(stats) < 60 and t13[0] * t13[5] == 6
    assert (hist == oracle_hist(stats)).all() and pos_hist.sum() == hist[1:].sum()


# ---- 8. the guard ----------------------------------------------------------------------------------------------------------------
def test_a_cn_id_out_of_range_is_skipped_and_flagged(E, oracle, monkeypatch):
    import torch
    monkeypatch.delenv(FORCE, raising=False)
    dv, dc, L, M, rho, ens, T = SHAPES["3-6-olmos"]
    p, trs = graphs(E, oracle, dv, dc, L, M, ens, T)
    assert E.ss_spectrum_form(p) == 1
    mem = members_of(p.n, rho, T)
    from oracle import pd_oracle as P
    ncomp = len(P.components(trs[0], mem[0])[0])
    bridges = []                                                         # the first two members with an edge whose loss splits a component
    for j in np.flatnonzero(mem[0]):
        for i in range(dv):
            cut = trs[0].astype(np.int64)
            cut[j, i] = 10 ** 9
            if len(P.components(cut, mem[0])[0]) > ncomp:
                bridges.append((j, i))
                break
        if len(bridges) == 2:
            break
    (a, ia), (b, ib) = bridges
    bad, cut = trs[:1].copy(), trs[:1].astype(np.int64)
    bad[0, a, ia], bad[0, b, ib] = p.nk, -1
    cut[0, a, ia], cut[0, b, ib] = 10 ** 9, 10 ** 9 + 1                   # the reference with those two edges removed
    want = np_spectrum_batch(cut, mem[:1], NBINS, p.L, p.vns_pos)
    clean = np_spectrum_batch(trs[:1], mem[:1], NBINS, p.L, p.vns_pos)
    assert not (want[0] == clean[0]).all()                               # the two edges mattered
    d_adj, d_m = upload(E, bad, mem[:1])
    hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
    pos = torch.zeros((p.L, 8), dtype=torch.int64, device="cuda")
    trial = torch.empty((1, 4), dtype=torch.int32, device="cuda")
    nbytes = E.lib().scldpc_ss_spectrum_workspace_bytes(C.byref(p), 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    E.check(E.lib().scldpc_ss_spectrum_device(C.byref(p), 1, d_adj.data_ptr(), 0, d_m.data_ptr(), NBINS, hist.data_ptr(), pos.data_ptr(),
                                              trial.data_ptr(), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()                                             # the call finishes
    assert int(ws[:4].view(torch.int32).item()) == E._lib.SS_BAD_CN
    same("guard", (hist.cpu().numpy(), pos.cpu().numpy(), trial.cpu().numpy()), want)
    with pytest.raises(RuntimeError, match="SS_BAD_CN"):
        E.ss_spectrum(p, d_adj, d_m, NBINS)
