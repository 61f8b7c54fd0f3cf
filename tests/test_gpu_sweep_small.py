"""The 4-bit sweep decoder on the GPU (-m gpu): scldpc_peel_sweep_device_sock16 (peel_sweep_small.hip) against the first-generation
E.peel_sweep on the same device tensors and against oracle/pd_oracle.py (peel_closure, components, sc_ldpc_trial_stats) — on a
hand-built code whose residuals are known, on device-sampled codes, with the queues cut short so that the kernel re-scans, at
the edges, and through simulate_sc_ldpc(sweep="small") and the ber_sim command line.  The code under test is never a reference."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu
COLS = [0, 1, 2, 7]                 # lost, lost_exp, positions flagged, channel erasures: what both decoders must agree on
SEED = 6                            # trials 0 .. 23 of this seed show the conditions asserted below (found on the CPU twin of the sampler)
# dv, dc, L, M, eps, terminated, bounded
SAMPLED = [(4, 8, 12, 40, 0.47, True, True), (4, 8, 12, 40, 0.47, False, False), (3, 6, 10, 20, 0.45, True, True),
           (5, 10, 12, 40, 0.5, False, True), (4, 8, 50, 1000, 0.48, True, True)]
IDS = ["%d-%d-L%d-M%d-%s%s" % (s[0], s[1], s[2], s[3], "T" if s[5] else "N", "B" if s[6] else "U") for s in SAMPLED]


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


def both(E, p, d_adj, d_cn, d_ch, args):
    """(rows, lost bits) of the first-generation decoder and of the decoder under test on the same tensors."""
    ref = E.peel_sweep(p, d_adj, d_ch, *args, want_lost=True)
    new = E.peel_sweep_sock16(p, d_adj, d_cn, d_ch, *args, want_lost=True)
    return ((ref["out"].cpu().numpy(), ref["lost"].cpu().numpy()), (new["out"].cpu().numpy(), new["lost"].cpu().numpy()))


def select(PD, p):
    E = PD.E
    kind, sampler = PD.select_sweep(p, "philox", "olmos", E.peel_sweep_sock16_supported(p), E.sock16_supported(p),
                                    E.deg_sock16_supported(p), "small")
    assert kind == "small"
    return sampler


# ---- 1. a hand-built code: VNs 2k and 2k + 1 of a position share all their CNs ---------------------------------------------
PAIR_L, PAIR_M = 8, 16


def paired_code(E, dv, dc):
    """VN t of position pos sends edge i to CN (pos + i) * cpp + t // (dc / dv): every CN has degree <= dc."""
    p = E.make_params(dv, dc, PAIR_L, PAIR_M)
    local = np.repeat((np.arange(PAIR_M) // (dc // dv))[:, None], dv, axis=1)                     # [M, dv], the same for every edge
    adj16 = np.tile(local, (PAIR_L, 1)).astype(np.uint16)
    return p, adj16


def channel(p, vns):
    bits = np.zeros(p.n, dtype=np.uint8)
    for pos, t in vns:
        bits[pos * PAIR_M + t] = 1
    return bits


def paired_cases(p, dv):
    """(name, erased VNs as (position, t), call arguments, the expected (lost, lost_exp, blocks) per pair)"""
    cpp, nk = p.cns_pos, p.nk
    full = (nk, 0, 0, nk)
    column = [(pos, t) for pos in range(PAIR_L) for t in (4, 5)]
    same = lambda v: {(4, 8): v, (3, 6): v, (5, 10): v}
    return [
        ("pair", [(3, 0), (3, 1)], full, same((2, 0, 0))),
        ("half a pair", [(3, 0)], full, same((0, 0, 0))),
        ("column", column, full, same((16, 16, 8))),
        ("column and pair", column + [(2, 8), (2, 9)], full, same((18, 16, 8))),
        ("single below the sweep", [(0, 6)], (nk, dv * cpp, 0, nk), same((1, 0, 0))),
        ("single swept", [(0, 6)], full, same((0, 0, 0))),
        ("column on a truncated chain", column, (PAIR_L * cpp, 0, 0, PAIR_L * cpp), {(4, 8): (10, 10, 5), (3, 6): (12, 12, 6), (5, 10): (8, 8, 4)}),
        ("pair and a loner", [(3, 0), (3, 1), (4, 4)], full, same((2, 0, 0))),
    ]


@pytest.mark.parametrize("qcap", [None, "8"], ids=["full_queues", "qcap8"])
@pytest.mark.parametrize("dv,dc", [(4, 8), (3, 6), (5, 10)])
def test_hand_built_paired_code(PD, monkeypatch, dv, dc, qcap):
    import torch
    E = PD.E
    if qcap:
        monkeypatch.setenv("SCLDPC_DEBUG_SWEEP_QCAP", qcap)
    p, adj16 = paired_code(E, dv, dc)
    tr = E.adj16_to_global(p, adj16).astype(np.int64)
    assert np.bincount(tr.ravel(), minlength=p.nk).max() <= dc
    cases = paired_cases(p, dv)
    for args in sorted({c[2] for c in cases}):                           # the channels that share their call go in one batch
        batch = [c for c in cases if c[2] == args]
        bits = np.stack([channel(p, c[1]) for c in batch])
        d_adj = torch.from_numpy(np.broadcast_to(adj16.view(np.int16), (len(batch),) + adj16.shape).copy()).cuda()
        d_ch = torch.from_numpy(E.pack_bits(bits).view(np.int32)).cuda()
        d_cn = E.cn_sockets(p, d_adj)
        (ref, ref_lost), (new, new_lost) = both(E, p, d_adj, d_cn, d_ch, args)
        for k, (name, vns, _, want) in enumerate(batch):
            lost, row = oracle_row(tr, bits[k].astype(bool), p.cns_pos, *args)
            assert row == want[(dv, dc)], (name, row)                    # the table of the issue, recomputed
            assert tuple(ref[k, :3]) == row and tuple(new[k, :3]) == row, (name, new[k], ref[k], row)
            assert new[k, 7] == len(vns) and (E.unpack_bits(new_lost[k:k + 1], p.n)[0] == lost).all(), name
        assert (new_lost == ref_lost).all() and (new[:, 3:5] == 0).all() and (new[:, 6] == 0).all()


# ---- 2. device-sampled codes ------------------------------------------------------------------------------------------------
_cache = {}


def sampled(PD, shape):
    """Per shape, computed once and left unchanged: the tensors of the selected sampler, the first-generation decoder's rows and
    lost bits on them, and the host copies."""
    if shape in _cache:
        return _cache[shape]
    E = PD.E
    dv, dc, L, M, e, term, bounded = shape
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p, T = g.params, (6 if M >= 1000 else 24)
    d_adj, d_cn, d_ch = PD._sample_small(select(PD, p), p, SEED, 0, T, e, [], "cuda:0")
    ref = E.peel_sweep(p, d_adj, d_ch, *geometry_args(g), want_lost=True)
    A = E.adj16_to_global(p, d_adj.cpu().numpy()).astype(np.int64)
    bits = E.unpack_bits(d_ch.cpu().numpy(), p.n).astype(bool)
    _cache[shape] = dict(g=g, p=p, T=T, d_adj=d_adj, d_cn=d_cn, d_ch=d_ch, A=A, bits=bits,
                         ref=ref["out"].cpu().numpy(), ref_lost=ref["lost"].cpu().numpy())
    return _cache[shape]


@pytest.mark.parametrize("shape", SAMPLED, ids=IDS)
def test_sampled_codes_equal_first_generation_and_oracle(PD, shape):
    from oracle import pd_oracle as P
    E = PD.E
    dv, dc, L, M, e, term, bounded = shape
    s = sampled(PD, shape)
    g, p, T = s["g"], s["p"], s["T"]
    new = E.peel_sweep_sock16(p, s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(g), want_lost=True)
    out, lost = new["out"].cpu().numpy(), new["lost"].cpu().numpy()
    assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all()
    assert (out[:, 3:5] == 0).all()
    for t in range(T):
        st = P.sc_ldpc_trial_stats(s["A"][t], s["bits"][t], dv, dc, L, M, term, bounded)
        assert tuple(out[t, COLS]) == (st["num_lost"], st["num_lost_exp"], st["blocks_failed_exp"], s["bits"][t].sum()), (shape, t)
    # the tables of the first-generation sampler + the cn_sockets pass: the same VN rows, the same table as a set per CN
    d_adj1, d_ch1 = E.sample_philox(p, SEED, 0, T, e, adj16=True)
    d_cn1 = E.cn_sockets(p, d_adj1)
    assert (d_adj1 == s["d_adj"]).all() and (d_ch1 == s["d_ch"]).all()
    assert (np.sort(d_cn1.cpu().numpy().view(np.uint16), axis=2) == np.sort(s["d_cn"].cpu().numpy().view(np.uint16), axis=2)).all()
    again = E.peel_sweep_sock16(p, d_adj1, d_cn1, d_ch1, *geometry_args(g), want_lost=True)
    assert (again["out"].cpu().numpy()[:, COLS] == s["ref"][:, COLS]).all() and (again["lost"].cpu().numpy() == s["ref_lost"]).all()


@pytest.mark.parametrize("shape", SAMPLED, ids=IDS)
def test_sampled_codes_do_not_rescan(PD, shape):
    """Column 6 (scans after the first) is 0 on the sampled shapes.  At (4,8), L = 50, M = 1000 a queue holds 768 entries and
    the first frontier is about 1170 CNs: the scan is walked a queue-full at a time from per-wave cursors, and what a wave's
    private half-queue (96 entries) cannot take spills to the idle queue, so nothing is dropped and nothing is scanned twice."""
    E = PD.E
    s = sampled(PD, shape)
    out = E.peel_sweep_sock16(s["p"], s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(s["g"]))["out"].cpu().numpy()
    assert (out[:, 6] == 0).all(), out[:, 6]


def test_the_sampled_cases_are_not_empty(PD):
    """On the REFERENCE's rows alone: a trial that decodes, a trial with a component of more than two, and at the (3,6) shape a
    trial whose lost set is partly (or wholly) made of components of at most two."""
    ref = {shape: sampled(PD, shape)["ref"] for shape in SAMPLED[:4]}
    rows = np.concatenate(list(ref.values()))
    assert (rows[:, 0] == 0).any() and (rows[:, 1] > 0).any()
    r36 = ref[SAMPLED[2]]
    assert ((r36[:, 1] >= 0) & (r36[:, 1] < r36[:, 0])).any()


# ---- 3. forced overflow: the re-scan path and the frozen rule ------------------------------------------------------------------
@pytest.mark.parametrize("qcap", ["16", "8"])
def test_short_queues_rescan_to_the_same_result(PD, monkeypatch, qcap):
    """The first three sampled shapes with queues of 16 (and of 8, the knob's floor) entries: the frontier is walked a
    queue-full at a time, a round's pushes are dropped where they exceed the queue and a scan from cursor 0 finds them again.
    Same outputs; at 16 entries column 6 > 0 on at least one trial."""
    E = PD.E
    rescans = []
    for shape in SAMPLED[:3]:
        s = sampled(PD, shape)
        g, p = s["g"], s["p"]
        # from the inputs alone: CNs holding exactly one erased VN at the outset
        c = np.arange(p.nk)
        ones = np.stack([np.bincount(s["A"][t][s["bits"][t]].ravel(), minlength=p.nk) == 1 for t in range(s["T"])])
        fireable = (ones & (c >= g.sweep_start) & (c < g.total_size)).sum(axis=1)
        assert (fireable > 16).any()                                     # the first frontier is longer than the queue
        if not shape[6]:                                                 # the unbounded chain: sweep_start = 10 positions
            assert g.sweep_start == 200 and g.total_size < p.nk and p.L == 52
            assert (ones & (c < g.sweep_start)).any(axis=1).all()        # frozen CNs in every trial: every scan must leave them out
        monkeypatch.setenv("SCLDPC_DEBUG_SWEEP_QCAP", qcap)
        new = E.peel_sweep_sock16(p, s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(g), want_lost=True)
        monkeypatch.delenv("SCLDPC_DEBUG_SWEEP_QCAP")
        out, lost = new["out"].cpu().numpy(), new["lost"].cpu().numpy()
        assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all(), shape
        rescans.append(out[:, 6])
    print("re-scans per trial at qcap", qcap, [r.tolist() for r in rescans])
    if qcap == "16":
        assert (np.concatenate(rescans) > 0).any()


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dv,dc,L,M,term,bounded", [(4, 8, 12, 40, True, True), (3, 6, 10, 20, False, False), (5, 10, 12, 40, True, False)])
def test_edges(PD, dv, dc, L, M, term, bounded):
    E = PD.E
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p, T = g.params, 5
    sampler = select(PD, p)
    # eps = 0: nothing erased, every output zero
    d_adj, d_cn, d_ch = PD._sample_small(sampler, p, SEED, 0, T, 0.0, [], "cuda:0")
    (ref, ref_lost), (new, new_lost) = both(E, p, d_adj, d_cn, d_ch, geometry_args(g))
    assert (new == 0).all() and (new_lost == 0).all() and (ref[:, COLS] == 0).all()
    # eps = 1: every VN erased (a CN counts dc <= 10: the nibble holds it)
    d_adj, d_cn, d_ch = PD._sample_small(sampler, p, SEED, 0, T, 1.0, [], "cuda:0")
    (ref, ref_lost), (new, new_lost) = both(E, p, d_adj, d_cn, d_ch, geometry_args(g))
    assert (new[:, COLS] == ref[:, COLS]).all() and (new_lost == ref_lost).all() and (new[:, 7] == p.n).all()
    # a hard-doped position through the sampler's own argument
    d_adj, d_cn, d_ch = PD._sample_small(sampler, p, SEED, 0, T, 0.5, [3], "cuda:0")
    assert not E.unpack_bits(d_ch.cpu().numpy(), p.n)[:, 3 * M:4 * M].any()
    (ref, ref_lost), (new, new_lost) = both(E, p, d_adj, d_cn, d_ch, geometry_args(g))
    assert (new[:, COLS] == ref[:, COLS]).all() and (new_lost == ref_lost).all() and (ref[:, 7] > 0).all()


# ---- 5. the mirror ---------------------------------------------------------------------------------------------------------------
def same13(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and len(a) == len(b) == 13


@pytest.mark.parametrize("l,r,L,M,e,term,bounded,kw", [
    (4, 8, 12, 40, 0.47, True, True, dict(num_repeats=24, batch=7)),
    (4, 8, 12, 40, 0.47, False, False, dict(num_repeats=24, batch=7)),
    (4, 8, 12, 40, 0.5, True, True, dict(num_repeats=40, batch=7, max_fuckups=3)),               # trips in the middle of a batch
    (4, 8, 16, 200, 0.52, True, True, dict(num_repeats=24, batch=7, doping_points={3: 0.5, 9: 0.25})),
    (3, 6, 10, 20, 0.45, True, True, dict(num_repeats=24, batch=7)),
], ids=["TB", "NU", "stop", "soft", "3-6"])
def test_simulate_sc_ldpc_small_equals_first(PD, l, r, L, M, e, term, bounded, kw):
    first = PD.simulate_sc_ldpc(e, l, r, L, M, term, False, bounded, False, rng="philox", seed=SEED, sweep="first", **kw)
    small = PD.simulate_sc_ldpc(e, l, r, L, M, term, False, bounded, False, rng="philox", seed=SEED, sweep="small", **kw)
    assert same13(first, small), (first[:8], small[:8])
    if "max_fuckups" in kw:
        assert first[5] < kw["num_repeats"] and first[5] % kw["batch"] != 0


def test_simulate_sc_ldpc_small_refuses_tail_biting(PD):
    with pytest.raises(ValueError, match="tail_biting"):
        PD.simulate_sc_ldpc(0.45, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", sweep="small")


# ---- 6. the command line -----------------------------------------------------------------------------------------------------------
def test_ber_sim_cli_writes_the_same_file_either_way(PD, tmp_path):
    text = {}
    for sweep in ("first", "small"):
        out = tmp_path / ("ber_%s.dat" % sweep)
        PD.main_simulate_sc_ldpc([str(out), "4", "8", "10", "20", "[0.5, 0.45]", "T", "U", "B", "NTB", "6", "2000", "[4]",
                                  "--rng", "philox", "--seed", "1", "--sweep", sweep])
        text[sweep] = open(out).read()
    lines = text["first"].strip().split("\n")
    assert lines[0].startswith("# SC-LDPC (4,8,L=11,M=20)") and len(lines) == 3
    assert text["small"] == text["first"]
