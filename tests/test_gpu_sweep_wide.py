"""The wide 4-bit sweep decoder on the GPU (-m gpu): scldpc_peel_sweep_device_sock16_wide (peel_sweep_small.hip, WIDE instances)
against the first-generation E.peel_sweep on the same device tensors and against oracle/pd_oracle.py — on a hand-built code whose
CN ids exceed 16 bits, on four device-sampled codes of more than 65 536 CNs (W1 - W4; the values asserted on the REFERENCE's rows
were found on the CPU twin of the sampler, seed 6, trials from 0), on small shapes, with the queues cut short so that the kernel
re-scans, at the edges, and through simulate_sc_ldpc(sweep="wide") and the ber_sim command line.  The code under test is never
a reference."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu
COLS = [0, 1, 2, 7]                 # lost, lost_exp, positions flagged, channel erasures: what both decoders must agree on
SEED = 6
# dv, dc, L, M, eps, terminated, bounded — the first four sampled shapes of tests/test_gpu_sweep_small.py
SMALL = [(4, 8, 12, 40, 0.47, True, True), (4, 8, 12, 40, 0.47, False, False), (3, 6, 10, 20, 0.45, True, True),
         (5, 10, 12, 40, 0.5, False, True)]
# id -> (shape, trials, the sampler the selector must name)
WIDE = {
    "W1": ((4, 8, 50, 2600, 0.48, True, True), 4, "sample_philox_wide_sock16"),
    "W2": ((4, 8, 50, 1500, 0.48, False, False), 4, "sample_philox_sock16"),
    "W3": ((3, 6, 660, 200, 0.44, True, True), 6, "sample_philox_deg_sock16"),
    "W4": ((5, 10, 50, 2500, 0.485, False, True), 6, "sample_philox_wide_sock16"),
}


@pytest.fixture(scope="module")
def PD():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import peeling_decoding
    return peeling_decoding


def geometry_args(g):
    return g.total_size, g.sweep_start, g.lost_lo, g.lost_hi


def oracle_row(tr, mask, cpp, total_size, sweep_start, lost_lo, lost_hi):
    """(lost bits, (lost, lost_exp, positions flagged)) of one trial from the oracle's closure and components (PD:656-691)."""
    from oracle import pd_oracle as P
    alive = P.peel_closure(tr, mask, total_size, sweep_start)
    lost = alive & ((tr >= lost_lo) & (tr < lost_hi)).any(axis=1) & (tr < total_size).all(axis=1)
    sizes, comp, idx = P.components(tr, lost)
    big = sizes[comp] > 2 if len(idx) else np.zeros(0, dtype=bool)
    return lost, (int(lost.sum()), int(sizes[sizes > 2].sum()), int(len(np.unique(tr[idx, 0][big] // cpp))))


def host(res):
    return res["out"].cpu().numpy(), res["lost"].cpu().numpy()


def first_and_wide(E, p, d_adj, d_cn, d_ch, args):
    """(rows, lost bits) of the first-generation decoder and of the decoder under test on the same tensors."""
    return (host(E.peel_sweep(p, d_adj, d_ch, *args, want_lost=True)),
            host(E.peel_sweep_sock16_wide(p, d_adj, d_cn, d_ch, *args, want_lost=True)))


def select(PD, p):
    E = PD.E
    kind, sampler = PD.select_sweep(p, "philox", "olmos", False, E.sock16_supported(p), E.deg_sock16_supported(p), "wide",
                                    wide_ok=E.peel_sweep_wide_supported(p), wide_sock16_ok=E.wide_sock16_supported(p))
    assert kind == "wide"
    return sampler


# ---- 1. a hand-built code above 16 bits: VNs 2k and 2k + 1 of a position share all their CNs ----------------------------------
PAIR_L, PAIR_M = 40, 3400
_paired = {}


def paired(E, dv, dc):
    """VN t of position pos sends edge i to CN (pos + i) * cpp + t // (dc / dv): every CN has degree <= dc.  With the cases
    (name, erased VNs as (position, t), call arguments, the expected row) and the oracle's answer per case, computed once."""
    if (dv, dc) in _paired:
        return _paired[(dv, dc)]
    p = E.make_params(dv, dc, PAIR_L, PAIR_M)
    cpp, nk = p.cns_pos, p.nk
    assert cpp == 1700 and nk == {(4, 8): 73100, (3, 6): 71400, (5, 10): 74800}[(dv, dc)]
    local = np.repeat((np.arange(PAIR_M) // (dc // dv))[:, None], dv, axis=1)                      # [M, dv], the same for every edge
    adj16 = np.tile(local, (PAIR_L, 1)).astype(np.uint16)
    tr = E.adj16_to_global(p, adj16).astype(np.int64)
    assert np.bincount(tr.ravel(), minlength=nk).max() <= dc
    full = (nk, 0, 0, nk)
    column = [(pos, t) for pos in range(PAIR_L) for t in (4, 5)]
    pair = [(39, 0), (39, 1)]
    assert tr[39 * PAIR_M:39 * PAIR_M + 2].min() >= 66300              # all of the pair's CNs lie beyond 16 bits
    cases = [
        ("pair", pair, full, (2, 0, 0)),
        ("half a pair", pair[:1], full, (0, 0, 0)),
        ("column", column, full, (80, 80, 40)),
        ("column and pair", column + pair, full, (82, 80, 40)),
        ("single below the sweep", [(0, 6)], (nk, dv * cpp, 0, nk), (1, 0, 0)),
        ("single swept", [(0, 6)], full, (0, 0, 0)),
        ("column on a truncated chain", column, (PAIR_L * cpp, 0, 0, PAIR_L * cpp), None),       # the oracle's row, whatever it is
    ]
    bits, rows = [], []
    for name, vns, args, want in cases:
        b = np.zeros(p.n, dtype=np.uint8)
        for pos, t in vns:
            b[pos * PAIR_M + t] = 1
        lost, row = oracle_row(tr, b.astype(bool), cpp, *args)
        assert want is None or row == want, (name, row)                  # the table of the issue, recomputed
        bits.append(b)
        rows.append((lost, row))
    trunc = rows[-1][1]
    assert 0 < trunc[0] < 80 and trunc[0] == trunc[1] and trunc[0] == 2 * trunc[2]     # the tail's VNs are not counted
    _paired[(dv, dc)] = (p, adj16, cases, bits, rows)
    return _paired[(dv, dc)]


@pytest.mark.parametrize("qcap", [None, "8"], ids=["full_queues", "qcap8"])
@pytest.mark.parametrize("dv,dc", [(4, 8), (3, 6), (5, 10)])
def test_hand_built_paired_code_above_16_bits(PD, monkeypatch, dv, dc, qcap):
    import torch
    E = PD.E
    p, adj16, cases, bits, rows = paired(E, dv, dc)
    if qcap:
        monkeypatch.setenv("SCLDPC_DEBUG_SWEEP_QCAP", qcap)
    for args in sorted({c[2] for c in cases}):                           # the channels that share their call go in one batch
        ks = [k for k, c in enumerate(cases) if c[2] == args]
        d_adj = torch.from_numpy(np.broadcast_to(adj16.view(np.int16), (len(ks),) + adj16.shape).copy()).cuda()
        d_ch = torch.from_numpy(E.pack_bits(np.stack([bits[k] for k in ks])).view(np.int32)).cuda()
        d_cn = E.cn_sockets(p, d_adj)
        (ref, ref_lost), (new, new_lost) = first_and_wide(E, p, d_adj, d_cn, d_ch, args)
        for i, k in enumerate(ks):
            name, vns = cases[k][:2]
            lost, row = rows[k]
            assert tuple(ref[i, :3]) == row and tuple(new[i, :3]) == row, (name, new[i], ref[i], row)
            assert new[i, 7] == len(vns) and (E.unpack_bits(new_lost[i:i + 1], p.n)[0] == lost).all(), name
        assert (new_lost == ref_lost).all() and (new[:, 3:5] == 0).all()
        if not qcap:
            assert (new[:, 6] == 0).all()


# ---- 2. device-sampled codes of more than 65 536 CNs ----------------------------------------------------------------------------
_cache = {}


def sampled(PD, shape, T, sampler=None):
    """Per shape, computed once and left unchanged: the tensors of the named sampler (None: sample_philox + cn_sockets), the
    first-generation decoder's rows and lost bits on them, and the host copies."""
    if shape in _cache:
        return _cache[shape]
    E = PD.E
    dv, dc, L, M, e, term, bounded = shape
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p = g.params
    if sampler is not None:
        assert select(PD, p) == sampler
    d_adj, d_cn, d_ch = PD._sample_small(sampler or "sample_philox+cn_sockets", p, SEED, 0, T, e, [], "cuda:0")
    ref, ref_lost = host(E.peel_sweep(p, d_adj, d_ch, *geometry_args(g), want_lost=True))
    A = E.adj16_to_global(p, d_adj.cpu().numpy()).astype(np.int64)
    bits = E.unpack_bits(d_ch.cpu().numpy(), p.n).astype(bool)
    # from the inputs alone: CNs holding exactly one erased VN at the outset
    ones = np.stack([np.bincount(A[t][bits[t]].ravel(), minlength=p.nk) == 1 for t in range(T)])
    _cache[shape] = dict(g=g, p=p, T=T, d_adj=d_adj, d_cn=d_cn, d_ch=d_ch, A=A, bits=bits, ones=ones, ref=ref, ref_lost=ref_lost)
    return _cache[shape]


def wide_case(PD, wid):
    shape, T, sampler = WIDE[wid]
    return shape, sampled(PD, shape, T, sampler)


@pytest.mark.parametrize("wid", list(WIDE))
def test_wide_codes_equal_first_generation_and_oracle(PD, wid):
    from oracle import pd_oracle as P
    E = PD.E
    shape, s = wide_case(PD, wid)
    dv, dc, L, M, e, term, bounded = shape
    g, p, T = s["g"], s["p"], s["T"]
    assert p.nk > 65536 and E.peel_sweep_wide_supported(p) and not E.peel_sweep_sock16_supported(p)
    out, lost = host(E.peel_sweep_sock16_wide(p, s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(g), want_lost=True))
    print(wid, "rows", out.tolist())
    assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all()
    assert (out[:, 3:5] == 0).all()
    assert (out[:, 6] == 0).all(), out[:, 6]                             # no frontier overflows at these sizes
    for t in range(T):
        st = P.sc_ldpc_trial_stats(s["A"][t], s["bits"][t], dv, dc, L, M, term, bounded)
        assert tuple(out[t, COLS]) == (st["num_lost"], st["num_lost_exp"], st["blocks_failed_exp"], s["bits"][t].sum()), (wid, t)
    # the tables of the first-generation sampler + the cn_sockets pass: the same VN rows, the same table as a set per CN
    d_adj1, d_ch1 = E.sample_philox(p, SEED, 0, T, e, adj16=True)
    d_cn1 = E.cn_sockets(p, d_adj1)
    assert (d_adj1 == s["d_adj"]).all() and (d_ch1 == s["d_ch"]).all()
    assert (np.sort(d_cn1.cpu().numpy().view(np.uint16), axis=2) == np.sort(s["d_cn"].cpu().numpy().view(np.uint16), axis=2)).all()
    again, again_lost = host(E.peel_sweep_sock16_wide(p, d_adj1, d_cn1, d_ch1, *geometry_args(g), want_lost=True))
    assert (again[:, COLS] == s["ref"][:, COLS]).all() and (again_lost == s["ref_lost"]).all()


def test_the_wide_cases_are_what_the_oracle_found(PD):
    """On the REFERENCE's rows and on the inputs alone: no test above can pass empty."""
    from oracle import pd_oracle as P
    c = lambda s: np.arange(s["p"].nk)
    shape, s = wide_case(PD, "W1")
    g, p, ref = s["g"], s["p"], s["ref"]
    assert (p.nk, p.n) == (68900, 130000)
    assert ref[:, 0].tolist() == [0, 39359, 0, 0] and ref[:, 1].tolist() == ref[:, 0].tolist() and ref[1, 2] == 40
    front = s["ones"] & (c(s) < g.total_size)
    assert ((front.sum(axis=1) >= 4366) & (front.sum(axis=1) <= 4563)).all()
    high = front[:, 65536:].sum(axis=1)
    assert ((high >= 925) & (high <= 1037)).all()

    shape, s = wide_case(PD, "W2")
    g, p, ref = s["g"], s["p"], s["ref"]
    assert (p.nk, p.n, p.L, g.total_size, g.sweep_start) == (69750, 135000, 90, 67500, 7500)
    assert ref[:, 0].tolist() == [36565, 36412, 36026, 36152] and (ref[:, 1] == ref[:, 0]).all() and (ref[:, 2] == 53).all()
    assert (s["ones"] & (c(s) < g.sweep_start)).sum(axis=1).tolist() == [802, 759, 801, 805]
    fire = (s["ones"] & (c(s) >= g.sweep_start) & (c(s) < g.total_size)).sum(axis=1)
    assert ((fire >= 2303) & (fire <= 2447)).all()
    alive = P.peel_closure(s["A"][0], s["bits"][0], g.total_size, g.sweep_start)
    assert 3740 <= (alive & (s["A"][0] >= 65536).any(axis=1)).sum() <= 3927

    shape, s = wide_case(PD, "W3")
    p, ref = s["p"], s["ref"]
    assert (p.nk, p.n) == (66200, 132000)
    assert ref[:, :2].tolist() == [[16791, 16789], [12668, 12666], [2987, 2987], [17340, 17338], [22321, 22319], [12502, 12502]]
    front = (s["ones"] & (c(s) < s["g"].total_size)).sum(axis=1)
    assert ((front >= 9300) & (front <= 9950)).all(), front             # "about 9 500 - 9 750"

    shape, s = wide_case(PD, "W4")
    g, p, ref = s["g"], s["p"], s["ref"]
    assert (p.nk, p.n, p.L, g.total_size) == (92500, 175000, 70, 87500)
    assert ref[:, 0].tolist() == [38970, 50307, 42121, 0, 53933, 54347]
    alive = P.peel_closure(s["A"][3], s["bits"][3], g.total_size, g.sweep_start)
    assert (alive & (s["A"][3] >= 65536).any(axis=1)).sum() == 16485    # trial 3: nothing lost in range, a residual on the tail


# ---- 3. small shapes through the wide form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL, ids=["%d-%d-L%d-M%d-%s%s" % (s[0], s[1], s[2], s[3], "T" if s[5] else "N", "B" if s[6] else "U")
                                              for s in SMALL])
def test_small_shapes_equal_first_generation_and_the_narrow_form(PD, shape):
    E = PD.E
    s = sampled(PD, shape, 24)
    g, p = s["g"], s["p"]
    out, lost = host(E.peel_sweep_sock16_wide(p, s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(g), want_lost=True))
    assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all()
    assert (out[:, 3:5] == 0).all() and (out[:, 6] == 0).all()
    narrow, narrow_lost = host(E.peel_sweep_sock16(p, s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(g), want_lost=True))
    assert (narrow[:, COLS] == s["ref"][:, COLS]).all() and (narrow_lost == s["ref_lost"]).all()      # a third witness
    assert (s["ref"][:, 0] > 0).any()


# ---- 4. forced overflow: the re-scan path and the frozen rule ----------------------------------------------------------------------
def short_queue_run(PD, monkeypatch, s, qcap):
    E = PD.E
    monkeypatch.setenv("SCLDPC_DEBUG_SWEEP_QCAP", qcap)
    out, lost = host(E.peel_sweep_sock16_wide(s["p"], s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(s["g"]), want_lost=True))
    monkeypatch.delenv("SCLDPC_DEBUG_SWEEP_QCAP")
    assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all()
    return out[:, 6]


@pytest.mark.parametrize("qcap", ["16", "8"])
def test_short_queues_rescan_to_the_same_result(PD, monkeypatch, qcap):
    rescans = []
    for shape in SMALL[:3]:
        s = sampled(PD, shape, 24)
        g, p = s["g"], s["p"]
        c = np.arange(p.nk)
        fireable = (s["ones"] & (c >= g.sweep_start) & (c < g.total_size)).sum(axis=1)
        assert (fireable > 16).any()                                     # the first frontier is longer than the queue
        if not shape[6]:
            assert (s["ones"] & (c < g.sweep_start)).any(axis=1).all()   # frozen CNs in every trial
        rescans.append(short_queue_run(PD, monkeypatch, s, qcap))
    print("re-scans per trial at qcap", qcap, [r.tolist() for r in rescans])
    if qcap == "16":
        assert (np.concatenate(rescans) > 0).any()


def test_short_queues_on_w2(PD, monkeypatch):
    """W2 with queues of 256 entries: every trial has frozen CNs and a first frontier longer than the queue (from the inputs)."""
    shape, s = wide_case(PD, "W2")
    g, p = s["g"], s["p"]
    c = np.arange(p.nk)
    assert ((s["ones"] & (c < g.sweep_start)).sum(axis=1) > 0).all()
    assert ((s["ones"] & (c >= g.sweep_start) & (c < g.total_size)).sum(axis=1) > 256).all()
    print("re-scans per trial on W2 at qcap 256", short_queue_run(PD, monkeypatch, s, "256").tolist())


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dv,dc,L,M,term,bounded", [(4, 8, 12, 40, True, True), (3, 6, 10, 20, False, False), (5, 10, 12, 40, True, False)])
def test_edges(PD, dv, dc, L, M, term, bounded):
    import torch
    E = PD.E
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p, T = g.params, 5
    sample = lambda e, doped=(): PD._sample_small("sample_philox+cn_sockets", p, SEED, 0, T, e, list(doped), "cuda:0")
    # eps = 0: nothing erased, every output zero
    d_adj, d_cn, d_ch = sample(0.0)
    (ref, ref_lost), (new, new_lost) = first_and_wide(E, p, d_adj, d_cn, d_ch, geometry_args(g))
    assert (new == 0).all() and (new_lost == 0).all() and (ref[:, COLS] == 0).all()
    # eps = 1: every VN erased (a CN counts dc <= 10: the nibble holds it)
    d_adj, d_cn, d_ch = sample(1.0)
    (ref, ref_lost), (new, new_lost) = first_and_wide(E, p, d_adj, d_cn, d_ch, geometry_args(g))
    assert (new[:, COLS] == ref[:, COLS]).all() and (new_lost == ref_lost).all() and (new[:, 7] == p.n).all()
    # a hard-doped position through the sampler's own argument
    d_adj, d_cn, d_ch = sample(0.5, [3])
    assert not E.unpack_bits(d_ch.cpu().numpy(), p.n)[:, 3 * M:4 * M].any()
    (ref, ref_lost), (new, new_lost) = first_and_wide(E, p, d_adj, d_cn, d_ch, geometry_args(g))
    assert (new[:, COLS] == ref[:, COLS]).all() and (new_lost == ref_lost).all() and (ref[:, 7] > 0).all()
    # total_size = 0 (nothing fires, nothing is lost), and a sweep that starts at or beyond total_size (every CN that holds one
    # VN from the outset is frozen): against the oracle
    A = E.adj16_to_global(p, d_adj.cpu().numpy()).astype(np.int64)
    bits = E.unpack_bits(d_ch.cpu().numpy(), p.n).astype(bool)
    for args in ((0, 0, 0, 0), (g.total_size, g.total_size, g.lost_lo, g.lost_hi), (g.total_size, g.total_size + 77, 0, g.total_size)):
        new, new_lost = host(E.peel_sweep_sock16_wide(p, d_adj, d_cn, d_ch, *args, want_lost=True))
        for t in range(T):
            lost, row = oracle_row(A[t], bits[t], p.cns_pos, *args)
            assert tuple(new[t, :3]) == row and new[t, 7] == bits[t].sum(), (args, t, new[t], row)
            assert (E.unpack_bits(new_lost[t:t + 1], p.n)[0] == lost).all()
        if args[0] == 0:
            assert (new[:, :3] == 0).all()
        else:
            assert (new[:, 0] > 0).all()
    # an empty batch
    empty = E.peel_sweep_sock16_wide(p, d_adj[:0].contiguous(), d_cn[:0].contiguous(), d_ch[:0].contiguous(), *geometry_args(g), want_lost=True)
    assert tuple(empty["out"].shape) == (0, 8) and tuple(empty["lost"].shape) == (0, p.nw)
    torch.cuda.synchronize()


# ---- 6. the mirror ---------------------------------------------------------------------------------------------------------------
def same13(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and len(a) == len(b) == 13


@pytest.mark.parametrize("l,r,L,M,e,term,bounded,kw", [
    (4, 8, 12, 40, 0.47, True, True, dict(num_repeats=24, batch=7)),
    (4, 8, 12, 40, 0.47, False, False, dict(num_repeats=24, batch=7)),
    (4, 8, 12, 40, 0.5, True, True, dict(num_repeats=40, batch=7, max_fuckups=3)),               # trips in the middle of a batch
    (4, 8, 16, 200, 0.52, True, True, dict(num_repeats=24, batch=7, doping_points={3: 0.5, 9: 0.25})),
    (3, 6, 10, 20, 0.45, True, True, dict(num_repeats=24, batch=7)),
    (4, 8, 50, 1500, 0.48, False, False, dict(num_repeats=6, batch=4)),                          # W2's geometry
], ids=["TB", "NU", "stop", "soft", "3-6", "W2"])
def test_simulate_sc_ldpc_wide_equals_first(PD, l, r, L, M, e, term, bounded, kw):
    first = PD.simulate_sc_ldpc(e, l, r, L, M, term, False, bounded, False, rng="philox", seed=SEED, sweep="first", **kw)
    wide = PD.simulate_sc_ldpc(e, l, r, L, M, term, False, bounded, False, rng="philox", seed=SEED, sweep="wide", **kw)
    assert same13(first, wide), (first[:8], wide[:8])
    if "max_fuckups" in kw:
        assert first[5] < kw["num_repeats"] and first[5] % kw["batch"] != 0


def test_simulate_sc_ldpc_wide_refuses_tail_biting(PD):
    with pytest.raises(ValueError, match="tail_biting"):
        PD.simulate_sc_ldpc(0.45, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", sweep="wide")


# ---- 7. the command line -----------------------------------------------------------------------------------------------------------
def test_ber_sim_cli_writes_the_same_file_either_way(PD, tmp_path):
    text = {}
    for sweep in ("first", "wide"):
        out = tmp_path / ("ber_%s.dat" % sweep)
        PD.main_simulate_sc_ldpc([str(out), "4", "8", "10", "20", "[0.5, 0.45]", "T", "U", "B", "NTB", "6", "2000", "[4]",
                                  "--rng", "philox", "--seed", "1", "--sweep", sweep])
        text[sweep] = open(out).read()
    lines = text["first"].strip().split("\n")
    assert lines[0].startswith("# SC-LDPC (4,8,L=11,M=20)") and len(lines) == 3
    assert text["wide"] == text["first"]
