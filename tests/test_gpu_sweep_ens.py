"""The 4-bit sweep decoder on the tail-biting and protograph ensembles (-m gpu): scldpc_sample_philox_ensemble_device_adj16_sock
(position-local rows + CN -> socket table) and scldpc_peel_sweep_device_sock16_tb / _tb_wide (the ring instances of
peel_sweep_small.hip; protograph runs the chain's entries) against the first generation on the same code —
E.sample_philox(ensemble=...) + E.peel_sweep on int32 rows — and against the CPU twins, oracle.sample_philox(ensemble=...) and
pd_oracle.sc_ldpc_trial_stats.  The code under test is never a reference.

SEED 6, trials 0 .. 23: on the CPU twin every shape below has trials that decode completely and trials with a component of
more than two lost VNs, and every tail-biting shape has lost and released erased VNs in its last dv - 1 VN positions, whose
edges wrap (test_the_cases_are_not_empty asserts that on the reference's rows and lost bits alone)."""
import numpy as np
import pytest

from conftest import require_gpu

pytestmark = pytest.mark.gpu
COLS = [0, 1, 2, 7]                 # lost, lost_exp, positions flagged, channel erasures: what both decoders must agree on
SEED = 6
TB, PG = "tail_biting", "protograph"
# ensemble, dv, dc, L, M, eps, terminated, bounded
SHAPES = [(TB, 4, 8, 12, 40, 0.39, False, True), (TB, 4, 8, 12, 40, 0.39, True, False), (TB, 4, 8, 4, 40, 0.40, True, True),
          (TB, 3, 6, 3, 20, 0.42, True, True), (TB, 3, 6, 10, 20, 0.42, False, False), (TB, 5, 10, 12, 40, 0.36, False, True),
          (TB, 5, 10, 5, 40, 0.36, True, True), (PG, 4, 8, 12, 40, 0.47, True, True), (PG, 3, 6, 10, 20, 0.42, False, False),
          (PG, 5, 10, 12, 40, 0.47, False, True)]
FULL_SIZE = (TB, 4, 8, 50, 1000, 0.39, True, True)              # 6 trials
ALL = SHAPES + [FULL_SIZE]


def shape_id(s):
    return "%s-%d-%d-L%d-M%d-%s%s" % ("tb" if s[0] == TB else "proto", s[1], s[2], s[3], s[4], "T" if s[6] else "N", "B" if s[7] else "U")


IDS = [shape_id(s) for s in ALL]


@pytest.fixture(scope="module")
def PD():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import peeling_decoding
    return peeling_decoding


def geometry_args(g):
    return g.total_size, g.sweep_start, g.lost_lo, g.lost_hi


# ---- host side of the layout: written from the header's contract, not from the library ------------------------------------------
def cn_positions(p, ens):
    """int [L, dv]: the CN position of edge i of VN position q."""
    c = np.arange(p.L)[:, None] + np.arange(p.dv)[None, :]
    return c % p.L if ens == TB else c


def rows_to_global(p, ens, rows16):
    """uint16 bit patterns [.., n, dv] of position-local ids -> int64 global CN ids."""
    a = np.ascontiguousarray(rows16).view(np.uint16).astype(np.int64)
    off = np.repeat(cn_positions(p, ens), p.vns_pos, axis=0) * p.cns_pos                   # [n, dv]
    return a + off


def host_table(p, A):
    """The CN -> socket table of one trial from its GLOBAL rows A [n, dv]: uint16 [nk, dc], the sockets dv * t + i of every CN in
    ascending order, 0xFFFF behind them."""
    cn = A.ravel()
    sock = (p.dv * (np.arange(p.n) % p.vns_pos)[:, None] + np.arange(p.dv)[None, :]).ravel()
    order = np.lexsort((sock, cn))
    cn_s, so_s = cn[order], sock[order]
    assert np.bincount(cn_s, minlength=p.nk).max() <= p.dc
    slot = np.arange(cn_s.size) - np.searchsorted(cn_s, cn_s, side="left")
    out = np.full((p.nk, p.dc), 0xFFFF, dtype=np.uint16)
    out[cn_s, slot] = so_s
    return out


def sorted_table(d_cn):
    return np.sort(d_cn.cpu().numpy().view(np.uint16), axis=2)


def check_table(p, ens, table, A):
    """table: uint16 [T, nk, dc] sorted per CN; A: global rows [T, n, dv]."""
    for t in range(A.shape[0]):
        assert (table[t] == host_table(p, A[t])).all(), t
    if ens == TB:
        ring = p.L * p.cns_pos
        assert (table[:, :ring] != 0xFFFF).all() and (table[:, ring:] == 0xFFFF).all()


# ---- per shape, computed once and left unchanged -------------------------------------------------------------------------------
_cache = {}


def sampled(PD, shape):
    """The reference's int32 rows, channel, decoder rows and lost bits, and the tensors of the sampler under test."""
    if shape in _cache:
        return _cache[shape]
    E = PD.E
    ens, dv, dc, L, M, e, term, bounded = shape
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p, T = g.params, (6 if M >= 1000 else 24)
    d_adj32, d_ch32 = E.sample_philox(p, SEED, 0, T, e, ensemble=ens)
    ref = E.peel_sweep(p, d_adj32, d_ch32, *geometry_args(g), want_lost=True)
    d_adj, d_cn, d_ch = E.sample_philox_ens_sock16(p, ens, SEED, 0, T, e)
    A = d_adj32.cpu().numpy().astype(np.int64)
    bits = E.unpack_bits(d_ch32.cpu().numpy(), p.n).astype(bool)
    _cache[shape] = dict(g=g, p=p, T=T, ens=ens, d_adj32=d_adj32, d_ch32=d_ch32, A=A, bits=bits, ref=ref["out"].cpu().numpy(),
                         ref_lost=ref["lost"].cpu().numpy(), d_adj=d_adj, d_cn=d_cn, d_ch=d_ch)
    return _cache[shape]


def decode(E, s, wide, **kw):
    fn = E.peel_sweep_sock16_wide if wide else E.peel_sweep_sock16
    new = fn(s["p"], s["d_adj"], s["d_cn"], s["d_ch"], *geometry_args(s["g"]), want_lost=True, ensemble=s["ens"], **kw)
    return new["out"].cpu().numpy(), new["lost"].cpu().numpy()


# ---- 0. what the cases hold, from the reference alone --------------------------------------------------------------------------------
def test_the_cases_are_not_empty(PD):
    """On the references alone.  The lost set leaves out the VNs whose CNs all lie in the ignored head or tail: in the one
    shape that ignores both (unbounded, not terminated) no wrapping VN can be lost, so what is asked of the wrapping positions
    there is that the peeling (pd_oracle.peel_closure on the reference's rows) leaves some of their erased VNs and releases
    others; every other tail-biting shape shows both in the reference decoder's own lost bits."""
    from oracle import pd_oracle as P
    for shape in SHAPES:
        s = sampled(PD, shape)
        ens, dv = shape[0], shape[1]
        g, p, rows = s["g"], s["p"], s["ref"]
        assert (rows[:, 0] == 0).any() and (rows[:, 1] > 0).any(), (shape, rows[:, :2])
        lost = PD.E.unpack_bits(s["ref_lost"], p.n).astype(bool)
        if ens == TB:                                                    # the wrapping VN positions: L - dv + 1 .. L - 1
            wrap = np.arange(p.n) >= (p.L - (dv - 1)) * p.vns_pos
            assert (cn_positions(p, ens)[p.L - (dv - 1):] < p.L - (dv - 1)).any(axis=1).all()
            left = np.stack([P.peel_closure(s["A"][t], s["bits"][t], g.total_size, g.sweep_start) for t in range(s["T"])])
            assert (left & wrap).any() and (s["bits"] & ~left & wrap).any(), shape
            assert not (lost & ~left).any()
            if shape[6] or shape[7]:
                assert (lost & wrap).any() and (s["bits"] & ~lost & wrap).any(), shape
        if not shape[7]:                                                 # unbounded: frozen CNs in every trial
            c = np.arange(p.nk)
            ones = np.stack([np.bincount(s["A"][t][s["bits"][t]].ravel(), minlength=p.nk) == 1 for t in range(s["T"])])
            assert g.sweep_start > 0 and (ones & (c < min(g.sweep_start, g.total_size))).any(axis=1).all(), shape
    for shape in (SHAPES[3], SHAPES[4]):                                 # (3,6): lost sets that include components of at most two
        r = sampled(PD, shape)["ref"]
        assert ((r[:, 0] > 0) & (r[:, 1] < r[:, 0])).any(), shape


# ---- 1. the sampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_sampler_rows_channel_and_table(PD, oracle, shape):
    E = PD.E
    ens, dv, dc, L, M, e, term, bounded = shape
    s = sampled(PD, shape)
    p, T = s["p"], s["T"]
    rows = rows_to_global(p, ens, s["d_adj"].cpu().numpy())
    assert (rows == s["A"]).all() and (s["d_ch"] == s["d_ch32"]).all()
    po = oracle.Params(dv, dc, p.L, p.cns_pos, p.vns_pos)
    words = s["d_ch"].cpu().numpy().view(np.uint32)
    for t in range(T):
        ra, rc = oracle.sample_philox(po, SEED, t, e, (), ensemble=ens)
        assert (rows[t] == ra).all() and (words[t] == rc).all(), t
    table = sorted_table(s["d_cn"])
    check_table(p, ens, table, s["A"])
    if ens == PG:
        assert (table == sorted_table(E.cn_sockets(p, s["d_adj"]))).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS[:-1])
def test_sampler_doped_trial0_and_batch_split(PD, shape):
    E = PD.E
    ens, dv, dc, L, M, e, term, bounded = shape
    s = sampled(PD, shape)
    p = s["p"]
    doped = tuple(sorted({q % p.L for q in (3, 4)}))                     # positions 3 and 4 (L = 3: 0 and 1; L = 4: 0 and 3)
    d_adj, d_cn, d_ch = E.sample_philox_ens_sock16(p, ens, SEED, 1000, 5, 0.5, doped)
    r_adj, r_ch = E.sample_philox(p, SEED, 1000, 5, 0.5, doped, ensemble=ens)
    A = r_adj.cpu().numpy().astype(np.int64)
    assert (rows_to_global(p, ens, d_adj.cpu().numpy()) == A).all() and (d_ch == r_ch).all()
    bits = E.unpack_bits(d_ch.cpu().numpy(), p.n).reshape(5, p.L, M)
    assert not bits[:, list(doped)].any() and bits.any()
    check_table(p, ens, sorted_table(d_cn), A)
    assert not (A[:2] == s["A"][:2]).all()                               # trial0 = 1000 draws other codes than trial0 = 0
    parts = [E.sample_philox_ens_sock16(p, ens, SEED, t0, nt, e) for t0, nt in ((0, 7), (7, 17))]
    for k, whole in enumerate((s["d_adj"], s["d_cn"], s["d_ch"])):
        joined = np.concatenate([q[k].cpu().numpy() for q in parts])
        if k == 1:
            assert (np.sort(joined.view(np.uint16), axis=2) == sorted_table(whole)).all()
        else:
            assert (joined == whole.cpu().numpy()).all(), k


# ---- 2. the decoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_decoder_equals_first_generation_and_oracle(PD, shape, wide):
    from oracle import pd_oracle as P
    E = PD.E
    ens, dv, dc, L, M, e, term, bounded = shape
    s = sampled(PD, shape)
    if ens == TB:
        assert E.peel_sweep_tb_supported(s["p"], wide=wide)
    out, lost = decode(E, s, wide)
    assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all()
    assert (out[:, 3:5] == 0).all()
    assert (out[:, 6] == 0).all(), out[:, 6]                             # full queues: no scan after the first
    if not wide:                                                         # (the reference is the same for both forms)
        for t in range(s["T"]):
            st = P.sc_ldpc_trial_stats(s["A"][t], s["bits"][t], dv, dc, L, M, term, bounded)
            assert tuple(s["ref"][t, COLS]) == (st["num_lost"], st["num_lost_exp"], st["blocks_failed_exp"], s["bits"][t].sum()), (shape, t)


# ---- 3. short queues ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qcap", ["16", "8"])
def test_short_queues_rescan_to_the_same_result(PD, monkeypatch, qcap):
    """The first three tail-biting shapes with queues of 16 and of 8 entries (the knob's floor), narrow and wide.  From the
    inputs alone the first frontier — the CNs of [sweep_start, total_size) that hold one erased VN at the outset — is longer
    than the queue in some trial; the one exception is the L = 4 ring at 16 entries, whose longest first frontier (80 CNs at
    eps = 0.40) is exactly 16: it fills the queue to the last entry, and that is asserted instead.  Same outputs; at 16 entries
    column 6 > 0 on at least one trial."""
    E = PD.E
    rescans = []
    for shape in SHAPES[:3]:
        s = sampled(PD, shape)
        g, p = s["g"], s["p"]
        c = np.arange(p.nk)                                              # from the inputs alone: CNs holding one erased VN at the outset
        ones = np.stack([np.bincount(s["A"][t][s["bits"][t]].ravel(), minlength=p.nk) == 1 for t in range(s["T"])])
        fireable = (ones & (c >= g.sweep_start) & (c < g.total_size)).sum(axis=1)
        if shape == SHAPES[2] and qcap == "16":
            assert fireable.max() == 16, fireable
        else:
            assert (fireable > int(qcap)).any(), fireable                # the first frontier is longer than the queue
        for wide in (False, True):
            monkeypatch.setenv("SCLDPC_DEBUG_SWEEP_QCAP", qcap)
            out, lost = decode(E, s, wide)
            monkeypatch.delenv("SCLDPC_DEBUG_SWEEP_QCAP")
            assert (out[:, COLS] == s["ref"][:, COLS]).all() and (lost == s["ref_lost"]).all(), (shape, wide)
            if not wide:
                rescans.append(out[:, 6])
    print("re-scans per trial at qcap", qcap, [r.tolist() for r in rescans])
    if qcap == "16":
        assert (np.concatenate(rescans) > 0).any()


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[6], SHAPES[8]], ids=[IDS[1], IDS[3], IDS[6], IDS[8]])
def test_eps_zero_and_one(PD, shape):
    E = PD.E
    ens, dv, dc, L, M, e, term, bounded = shape
    g = PD._Geometry(dv, dc, L, M, term, bounded, [])
    p, T = g.params, 5
    for eps in (0.0, 1.0):
        r_adj, r_ch = E.sample_philox(p, SEED, 0, T, eps, ensemble=ens)
        ref = E.peel_sweep(p, r_adj, r_ch, *geometry_args(g), want_lost=True)
        d_adj, d_cn, d_ch = E.sample_philox_ens_sock16(p, ens, SEED, 0, T, eps)
        assert (d_ch == r_ch).all()
        for fn in (E.peel_sweep_sock16, E.peel_sweep_sock16_wide):
            new = fn(p, d_adj, d_cn, d_ch, *geometry_args(g), want_lost=True, ensemble=ens)
            out, lost = new["out"].cpu().numpy(), new["lost"].cpu().numpy()
            assert (out[:, COLS] == ref["out"].cpu().numpy()[:, COLS]).all() and (lost == ref["lost"].cpu().numpy()).all()
            if eps == 0.0:
                assert (out == 0).all() and (lost == 0).all()
            else:
                assert (out[:, 7] == p.n).all()                          # a CN counts dc <= 10: the nibble holds it


RING_L, RING_M = 8, 16


def ring_code(E, dv, dc):
    """VN t of position q sends edge i to CN ((q + i) mod L) * cpp + t // (dc / dv): every CN of the ring has degree dc."""
    p = E.make_params(dv, dc, RING_L, RING_M)
    local = np.repeat((np.arange(RING_M) // (dc // dv))[:, None], dv, axis=1)
    adj16 = np.tile(local, (RING_L, 1)).astype(np.uint16)
    return p, adj16, rows_to_global(p, TB, adj16)


def oracle_row(tr, mask, cpp, total_size, sweep_start, lost_lo, lost_hi):
    from oracle import pd_oracle as P
    alive = P.peel_closure(tr, mask, total_size, sweep_start)
    lost = alive & ((tr >= lost_lo) & (tr < lost_hi)).any(axis=1) & (tr < total_size).all(axis=1)
    sizes, comp, idx = P.components(tr, lost)
    big = sizes[comp] > 2 if len(idx) else np.zeros(0, dtype=bool)
    return lost, (int(lost.sum()), int(sizes[sizes > 2].sum()), int(len(np.unique(tr[idx, 0][big] // cpp))))


@pytest.mark.parametrize("qcap", [None, "8"], ids=["full_queues", "qcap8"])
@pytest.mark.parametrize("dv,dc", [(4, 8), (3, 6), (5, 10)])
def test_hand_built_ring_code(PD, monkeypatch, dv, dc, qcap):
    import torch
    E = PD.E
    p, adj16, tr = ring_code(E, dv, dc)
    assert (np.bincount(tr.ravel(), minlength=p.nk)[:RING_L * p.cns_pos] == dc).all() and tr.max() < RING_L * p.cns_pos
    assert sorted(set((tr[(RING_L - 1) * RING_M] // p.cns_pos).tolist())) == sorted([RING_L - 1] + list(range(dv - 1)))
    args = (p.nk, 0, 0, p.nk)
    cases = [("pair in the last position", [(RING_L - 1, 0), (RING_L - 1, 1)], (2, 0, 0)),
             ("column", [(pos, t) for pos in range(RING_L) for t in (4, 5)], None),
             ("column and pair", [(pos, t) for pos in range(RING_L) for t in (4, 5)] + [(RING_L - 1, 8), (RING_L - 1, 9)], None),
             ("half a pair", [(RING_L - 1, 0)], (0, 0, 0))]
    bits = np.zeros((len(cases), p.n), dtype=np.uint8)
    for k, (_, vns, _) in enumerate(cases):
        for pos, t in vns:
            bits[k, pos * RING_M + t] = 1
    B = len(cases)
    d_adj = torch.from_numpy(np.broadcast_to(adj16.view(np.int16), (B,) + adj16.shape).copy()).cuda()
    d_a32 = torch.from_numpy(np.broadcast_to(tr.astype(np.int32), (B,) + tr.shape).copy()).cuda()
    d_cn = torch.from_numpy(np.broadcast_to(host_table(p, tr).view(np.int16), (B, p.nk, p.dc)).copy()).cuda()
    d_ch = torch.from_numpy(E.pack_bits(bits).view(np.int32)).cuda()
    ref = E.peel_sweep(p, d_a32, d_ch, *args, want_lost=True)
    ref_out, ref_lost = ref["out"].cpu().numpy(), ref["lost"].cpu().numpy()
    if qcap:
        monkeypatch.setenv("SCLDPC_DEBUG_SWEEP_QCAP", qcap)
    for fn in (E.peel_sweep_sock16, E.peel_sweep_sock16_wide):
        new = fn(p, d_adj, d_cn, d_ch, *args, want_lost=True, ensemble=TB)
        out, new_lost = new["out"].cpu().numpy(), new["lost"].cpu().numpy()
        for k, (name, vns, want) in enumerate(cases):
            lost, row = oracle_row(tr, bits[k].astype(bool), p.cns_pos, *args)
            assert want is None or row == want, (name, row)
            assert tuple(ref_out[k, :3]) == row and tuple(out[k, :3]) == row, (name, out[k], ref_out[k], row)
            assert out[k, 7] == len(vns) and (E.unpack_bits(new_lost[k:k + 1], p.n)[0] == lost).all(), name
        assert (new_lost == ref_lost).all() and (out[:, 3:5] == 0).all()
    column = oracle_row(tr, bits[1].astype(bool), p.cns_pos, *args)[1]
    assert column[0] == 2 * RING_L and column[1] == 2 * RING_L and column[2] == RING_L      # one component around the whole ring


# ---- 5. the mirror -----------------------------------------------------------------------------------------------------------------
def same13(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and len(a) == len(b) == 13


MIRROR = [
    (TB, 0.39, True, True, "small", dict(num_repeats=24, batch=7)),
    (TB, 0.39, False, False, "small", dict(num_repeats=24, batch=7)),
    (TB, 0.45, True, True, "small", dict(num_repeats=40, batch=7, max_fuckups=3)),          # trips in the middle of a batch
    (TB, 0.42, True, True, "small", dict(num_repeats=24, batch=7, doping_points={3: 0.5})),
    (TB, 0.39, True, False, "wide", dict(num_repeats=24, batch=7)),
    (PG, 0.47, True, True, "small", dict(num_repeats=24, batch=7)),
    (PG, 0.47, False, False, "small", dict(num_repeats=24, batch=7)),
    (PG, 0.5, True, True, "small", dict(num_repeats=40, batch=7, max_fuckups=3)),
    (PG, 0.47, False, True, "wide", dict(num_repeats=24, batch=7)),
]


@pytest.mark.parametrize("ens,e,term,bounded,sweep,kw", MIRROR,
                         ids=["%s-%s%s-%s-%s" % ("tb" if m[0] == TB else "proto", "T" if m[2] else "N", "B" if m[3] else "U", m[4],
                                                  "stop" if "max_fuckups" in m[5] else "soft" if "doping_points" in m[5] else "run")
                              for m in MIRROR])
def test_simulate_sc_ldpc_local_tables_equals_first(PD, capfd, ens, e, term, bounded, sweep, kw):
    flags = (term, ens == PG, bounded, ens == TB)
    first = PD.simulate_sc_ldpc(e, 4, 8, 12, 40, *flags, rng="philox", seed=SEED, sweep="first", **kw)
    capfd.readouterr()
    new = PD.simulate_sc_ldpc(e, 4, 8, 12, 40, *flags, rng="philox", seed=SEED, sweep=sweep, local_tables=True, **kw)
    assert same13(first, new), (first[:8], new[:8])
    line = capfd.readouterr().err
    decoder = "peel_sweep_small (4-bit CN counts" if sweep == "small" else "peel_sweep_wide (4-bit CN counts, 32-bit queues"
    assert "sample_philox_ens_sock16 + " + decoder + (", tail-biting)" if ens == TB else ")") in line, line
    assert first[4] > 0                                                  # frames failed: the comparison is not of zeros
    if "max_fuckups" in kw:
        assert first[5] < kw["num_repeats"] and first[5] % kw["batch"] != 0


def test_simulate_sc_ldpc_refusals_on_the_device(PD):
    with pytest.raises(ValueError, match="^local_tables=True: the Olmos chain"):
        PD.simulate_sc_ldpc(0.45, 4, 8, 12, 40, True, False, True, False, num_repeats=2, rng="philox", sweep="small", local_tables=True)
    with pytest.raises(ValueError, match="^sweep='small': the tail_biting tables hold global CN ids"):      # without the switch: as before
        PD.simulate_sc_ldpc(0.45, 4, 8, 12, 40, True, False, True, True, num_repeats=2, rng="philox", sweep="small")


def test_ber_sim_cli_writes_the_same_file_either_way(PD, tmp_path):
    text = {}
    for name, extra in (("first", ["--sweep", "first"]), ("small", ["--sweep", "small", "--local-tables", "on"])):
        out = tmp_path / ("ber_%s.dat" % name)
        PD.main_simulate_sc_ldpc([str(out), "4", "8", "10", "20", "[0.42, 0.38]", "T", "U", "B", "TB", "6", "2000", "[4]",
                                  "--rng", "philox", "--seed", "1"] + extra)
        text[name] = open(out).read()
    lines = text["first"].strip().split("\n")
    assert lines[0].startswith("# SC-LDPC (4,8,L=11,M=20)") and "tail biting:True" in lines[0] and len(lines) == 3
    assert text["small"] == text["first"]
