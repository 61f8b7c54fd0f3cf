"""Every form of the eps-grid and threshold decoders (-m gpu) at the smallest shapes that still take it: peel_sweep_eps,
full_bp_eps, frame_threshold and vn_threshold on the same frames, over CN-word policy (16-bit Packed, 32-bit Wide in LDS, 32-bit
WideG in the workspace) x adjacency width (2-byte position-local rows, 4-byte global rows of the same code) x the dv = 4 and the
generic-dv code, on the terminated chain and on the truncated one.  The shapes are tests/test_eps_forms_host.py's table, which
asserts on the CPU which form each of them takes.  Every reference is computed on the CPU — host_vn_thresholds, host_bisect,
oracle.decode_bp (literal = False) and pd_oracle.peel_closure / components over the downloaded rows, keys and levels — once per
shape and chain, shared by both row widths and all four kernels, and every comparison is exact equality.  That the inputs
exercise the code (thresholds inside the window, walks of at least 100 steps, frames that fail at the top of the grid and decode
at its bottom, all three statuses) is read off the references alone.  The debug caps (a candidate list of three entries, queues
of one entry) repeat one Wide and one WideG shape with list overflows, tie rounds and queue re-scans."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_gpu_bp_eps as BPE
import test_gpu_eps as PDE
import test_gpu_thresh as TH
import test_gpu_vn_thresh as VT
from conftest import require_gpu
from test_eps_forms_host import PACKED, WIDE, WIDE_G, form
from test_eps_host import QCAP
from test_vn_thresh_host import CCAP

pytestmark = pytest.mark.gpu

SEED, TRIAL0 = 20261, 7
WINDOW = (0.50, 0.62)
ES = [0.62, 0.59, 0.57, 0.55, 0.53, 0.50]                               # descending, both ends of the window
NARROW = {"decodes at the top": (0.40, 0.50), "fails at the bottom": (0.60, 0.62)}
FRAMES_LDS, FRAMES_WORKSPACE = 8, 3

# (shape, 2-byte rows): the Packed twins with 2-byte rows only (int32 rows make them Wide)
CASES = [(s, a16) for s in list(WIDE) + list(WIDE_G) for a16 in (True, False)] + [(s, True) for s in PACKED]
# one shape per form no other test runs, 2-byte rows unless said otherwise
NEW_FORMS = {
    "Wide-A16-DV4": ((4, 8, 6, 1026), True), "Wide-A16-generic": ((5, 10, 6, 820), True),
    "WideG-A16-DV4": ((4, 8, 6, 8044), True), "WideG-A16-generic": ((3, 6, 6, 8966), True),
    "WideG-int32-generic": ((3, 6, 6, 8966), False),
}
CAPPED = {"Wide-A16": (3, 6, 6, 1366), "WideG-A16": (5, 10, 6, 7296)}


def case_id(c):
    return "%d_%d_L%d_N%d" % c[0] + ("-A16" if c[1] else "-int32")


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the eps form tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def thresholds(E, window):
    return E.erasure_threshold(window[0]), E.erasure_threshold(window[1])


# ---- the inputs: one code per frame in both row widths, its keys and its levels ---------------------------------------------------
_INPUTS, _REFS = {}, {}


def inputs(E, shape):
    """Sampled once per shape: the 2-byte rows, the int32 copy of the same graph, the keys and the levels of ES."""
    if shape in _INPUTS:
        return _INPUTS[shape]
    p = E.make_params(*shape)
    T = FRAMES_WORKSPACE if shape in WIDE_G else FRAMES_LDS
    d_adj16, d_ch = E.sample_philox(p, SEED, TRIAL0, T, ES[0], adj16=True)
    d_keys = E.channel_keys(p, SEED, TRIAL0, T)
    d_lev = E.channel_levels(p, SEED, TRIAL0, T, ES)
    synchronize()
    adj16 = d_adj16.cpu().numpy().copy()
    gadj = np.ascontiguousarray(E.adj16_to_global(p, adj16), dtype=np.int32)
    d_adj32, _ = E.to_device(gadj, d_ch.cpu().numpy())
    keys, lev = d_keys.cpu().numpy().view(np.uint32).copy(), d_lev.cpu().numpy().copy()
    assert gadj.shape == (T, p.n, p.dv) and gadj.min() >= 0 and gadj.max() < p.nk
    assert (E.global_to_adj16(p, gadj).view(np.uint16) == adj16.view(np.uint16)).all()     # one graph, two widths
    ths = [E.erasure_threshold(e) for e in ES]
    for k, th in enumerate(ths):                                         # the levels are the keys' channels at the grid's points
        assert (E.pack_bits(lev > k) == E.pack_bits(keys < th)).all(), (shape, k)
    assert (E.pack_bits(lev > 0) == d_ch.cpu().numpy().view(np.uint32)).all()
    c = dict(p=p, T=T, d_adj={True: d_adj16, False: d_adj32}, d_keys=d_keys, d_lev=d_lev, adj16=adj16, gadj=gadj, keys=keys, lev=lev,
             ths=ths)
    _INPUTS[shape] = c
    return c


def sweep_range(p, is_term):
    """(total_size, lost_lo, lost_hi) of peel_sweep_eps: the terminated chain whole; the truncated one, whose CNs from position L
    on never fire, reporting the VNs with a CN in positions 1 .. L - 2."""
    return (p.nk, 0, p.nk) if is_term else (p.L * p.cns_pos, p.cns_pos, (p.L - 1) * p.cns_pos)


def grid64(t_lo, t_hi):
    g = VT.grid_of(t_lo, t_hi, 64)
    assert len(g) == 64 and g[0] == t_lo and g[-1] == t_hi
    return g


def host_references(engine, p, gadj, keys, lev, is_term, t_lo, t_hi):
    """Everything the four kernels are held to, from numpy arrays alone (no device): the walk, the bisection, full BP's counters
    and erased bits and the sweep's counts and lost bits at every point of ES.  The references are checked against each other
    where they state the same thing."""
    from oracle import oracle as O
    from oracle import pd_oracle as P
    T, K = gadj.shape[0], len(ES)
    grid = grid64(t_lo, t_hi)
    vn = VT.host_reference(p, gadj, keys, t_lo, t_hi, is_term, grid)
    rows, bits = TH.host_rows(p, gadj, keys, t_lo, t_hi, is_term)
    po = O.Params(p.dv, p.dc, p.L, p.cns_pos, p.vns_pos)
    total, lo, hi = sweep_range(p, is_term)
    bp = [(np.zeros((T, 8), dtype=np.int64), np.zeros((T, p.nw), dtype=np.uint32)) for _ in range(K)]
    pd = [(np.zeros((T, 8), dtype=np.int64), np.zeros((T, p.nw), dtype=np.uint32)) for _ in range(K)]
    ths = [engine.erasure_threshold(e) for e in ES]
    # the oracle's expurgation compares the erased VNs of a position pair by pair (a second per failing frame and point at
    # n = 48 000): the calls of a shape run side by side, eight at a time (ctypes releases the interpreter lock)
    graphs = [O.Graph.from_vn_adj(po, gadj[t]) for t in range(T)]
    with ThreadPoolExecutor(max_workers=8) as pool:
        decoded = list(pool.map(lambda tk: O.decode_bp(graphs[tk[0]], (lev[tk[0]] > tk[1]).astype(np.uint8), max_it=0,
                                                       is_term=1 if is_term else 0, literal=False),
                                [(t, k) for t in range(T) for k in range(K)]))
    for t in range(T):
        tr = gadj[t].astype(np.int64)
        inside = ((tr >= lo) & (tr < hi)).any(axis=1) & (tr < total).all(axis=1)
        for k in range(K):
            chan = (lev[t] > k).astype(np.uint8)
            res, erased, _ = decoded[t * K + k]
            bp[k][0][t] = [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"], res["num_blocks_err_exp"], 0, 0, 0,
                           chan.sum()]
            bp[k][1][t] = engine.pack_bits(erased)
            # the walk's tau says the same as full BP at every point of the grid
            assert ((vn["tau"][t] <= ths[k]) == erased.astype(bool)).all(), (t, k)
            alive = P.peel_closure(tr, chan.astype(bool), total, 0)
            assert (alive == erased.astype(bool)).all(), (t, k)          # two oracles, one maximal stopping set
            lost = alive & inside
            sizes, comp, idx = P.components(tr, lost)
            big = sizes[comp] > 2 if len(idx) else np.zeros(0, dtype=bool)
            pd[k][0][t] = [int(lost.sum()), int(sizes[sizes > 2].sum()), int(len(np.unique((tr[idx, 0] // p.cns_pos)[big]))), 0, 0,
                           0, 0, chan.sum()]
            pd[k][1][t] = engine.pack_bits(lost)
    # the bisection and the walk agree on the threshold, the status and the critical residual
    assert (vn["rows"][:, :2] == rows[:, :2]).all() and (vn["rows"][:, 3] == rows[:, 2]).all() and (vn["rows"][:, 5] == rows[:, 5]).all()
    return dict(vn=vn, grid=grid, rows=rows, bits=bits, bp=bp, pd=pd, sweep=(total, lo, hi), t_lo=t_lo, t_hi=t_hi)


def reference(E, shape, is_term):
    if (shape, is_term) not in _REFS:
        c = inputs(E, shape)
        t_lo, t_hi = thresholds(E, WINDOW)
        assert (t_lo, t_hi) == (c["ths"][-1], c["ths"][0])
        _REFS[shape, is_term] = host_references(E, c["p"], c["gadj"], c["keys"], c["lev"], is_term, t_lo, t_hi)
    return _REFS[shape, is_term]


def assert_inputs_exercise_the_code(p, ref, is_term, what):
    """From the references alone."""
    r = ref["vn"]["rows"]
    status, steps = r[:, 1], r[:, 4]
    ne = np.stack([b[0][:, 0] for b in ref["bp"]])                       # [K, T]
    print(what, "window", WINDOW, "| status:", status.tolist(), "| steps:", steps.tolist(), "| eps*:",
          [round(int(x) / 2147483647.0, 4) for x in r[:, 0]], "| failing frames per point:", (ne > 0).sum(axis=1).tolist(),
          "| largest release of a step:", max(max(x, default=0) for x in ref["vn"]["releases"]))
    if is_term:
        assert ((status == 0) & (steps >= 100)).any()
        assert (ne[0] > 0).any() and (ne[-1] == 0).any()
    else:
        assert (status == 2).all() and p.L * p.cns_pos < p.nk and (steps >= 100).any()


# ---- the four kernels against the references ----------------------------------------------------------------------------------------
def run_four(E, c, ref, a16, is_term, what):
    """The four kernels on the frames of a shape in one row width; every comparison with the references.  Returns the rows of
    vn_threshold and frame_threshold, the counters of full_bp_eps and the rows of peel_sweep_eps."""
    import torch
    p, d_adj, K = c["p"], c["d_adj"][a16], len(ES)
    assert d_adj.dtype == (torch.int16 if a16 else torch.int32)
    t_lo, t_hi = ref["t_lo"], ref["t_hi"]
    got = E.vn_threshold(p, d_adj, c["d_keys"], t_lo, t_hi, grid=ref["grid"], is_term=is_term, want_tau=True)
    synchronize()
    vr = VT.assert_equals_reference(ref["vn"], got, what + " vn_threshold K = 64")
    ft = E.frame_threshold(p, d_adj, c["d_keys"], t_lo, t_hi, is_term=is_term, want_bits=True)
    synchronize()
    fr = TH.assert_equals_host(None, ft, what + " frame_threshold", ref["rows"], ref["bits"])
    # the siblings agree: tau == T* packs to the critical residual (status 0), tau == t_lo to what is left at t_lo (status 2)
    tau, fbits = VT.unsigned(got["tau"]), ft["bits"].cpu().numpy().view(np.uint32)
    at = np.where(vr[:, 1] == 0, vr[:, 0], np.where(vr[:, 1] == 2, t_lo, -1))
    assert (vr[:, :2] == fr[:, :2]).all() and (vr[:, 3] == fr[:, 2]).all() and (vr[:, 7] == fr[:, 7]).all()
    assert (E.pack_bits(tau == at[:, None]) == fbits).all(), what
    walk = E.full_bp_eps(p, d_adj, c["d_lev"], K, is_term=is_term, want_erased=True)
    synchronize()
    cnt = BPE.assert_equals_full_bp(dict(es=ES, refs=ref["bp"]), walk, what + " full_bp_eps")
    total, lo, hi = ref["sweep"]
    sweep = E.peel_sweep_eps(p, d_adj, c["d_lev"], K, total, lo, hi, want_lost=True)
    synchronize()
    out = PDE.assert_equals_peel_sweep(dict(es=ES, refs=ref["pd"]), sweep, what + " peel_sweep_eps")
    return got, vr, fr, cnt, out


@pytest.mark.parametrize("is_term", [True, False], ids=["terminated", "open"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_form_equals_the_cpu_references(E, monkeypatch, case, is_term):
    shape, a16 = case
    monkeypatch.delenv(QCAP, raising=False)
    monkeypatch.delenv(CCAP, raising=False)
    want = "Packed" if shape in PACKED else "WideG" if shape in WIDE_G else "Wide"
    for kernel in ("peel_sweep_eps", "full_bp_eps", "frame_threshold", "vn_threshold"):
        assert form(shape, a16, kernel) == (want, "A16" if a16 else "int32", "DV4" if shape[0] == 4 else "generic")
    c = inputs(E, shape)
    p = c["p"]
    ref = reference(E, shape, is_term)
    what = "%s %s %s" % (case_id(case), "terminated" if is_term else "open", want)
    assert_inputs_exercise_the_code(p, ref, is_term, what)
    got, vr, fr, cnt, out = run_four(E, c, ref, a16, is_term, what)
    assert (vr[:, 6] == 0).all() and (out[:, :, 6] == 0).all()           # nothing overflows without a cap
    # without tau and without a grid the rows are the same
    args = (p, c["d_adj"][a16], c["d_keys"], ref["t_lo"], ref["t_hi"])
    bare = E.vn_threshold(*args, is_term=is_term)
    synchronize()
    assert bare["tau"] is None
    VT.assert_equals_reference(ref["vn"], bare, what + " vn_threshold K = 0", counts=ref["vn"]["counts"][:, :0])
    # the inputs are as they were
    assert (c["d_adj"][True].cpu().numpy() == c["adj16"]).all() and (c["d_adj"][False].cpu().numpy() == c["gadj"]).all()
    assert (c["d_keys"].cpu().numpy().view(np.uint32) == c["keys"]).all() and (c["d_lev"].cpu().numpy() == c["lev"]).all()


# ---- narrow windows: statuses 1 and 2 on a terminated chain ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NEW_FORMS))
def test_narrow_windows_of_the_new_forms(E, monkeypatch, name):
    """[0.40, 0.50], where every frame decodes at the top (status 1), and [0.60, 0.62], where every frame fails at the bottom
    (status 2, after a walk across the window), on one shape of each form: frame_threshold and vn_threshold against the host."""
    shape, a16 = NEW_FORMS[name]
    monkeypatch.delenv(QCAP, raising=False)
    monkeypatch.delenv(CCAP, raising=False)
    assert "-".join(form(shape, a16)) == name
    c = inputs(E, shape)
    p, d_adj = c["p"], c["d_adj"][a16]
    for label, window in NARROW.items():
        t_lo, t_hi = thresholds(E, window)
        key = (shape, window)
        if key not in _REFS:
            grid = grid64(t_lo, t_hi)
            vn = VT.host_reference(p, c["gadj"], c["keys"], t_lo, t_hi, True, grid)
            rows, bits = TH.host_rows(p, c["gadj"], c["keys"], t_lo, t_hi, True)
            _REFS[key] = (grid, vn, rows, bits)
        grid, vn, rows, bits = _REFS[key]
        status = vn["rows"][:, 1]
        print(name, label, "window", window, "| status:", status.tolist(), "| steps:", vn["rows"][:, 4].tolist())
        assert (status == (1 if label == "decodes at the top" else 2)).all() and (rows[:, 1] == status).all()
        if label == "fails at the bottom":
            assert (vn["rows"][:, 4] >= 10).all()                        # the walk crosses the window before it gives up
        got = E.vn_threshold(p, d_adj, c["d_keys"], t_lo, t_hi, grid=grid, want_tau=True)
        synchronize()
        VT.assert_equals_reference(vn, got, "%s %s vn_threshold" % (name, label))
        ft = E.frame_threshold(p, d_adj, c["d_keys"], t_lo, t_hi, want_bits=True)
        synchronize()
        TH.assert_equals_host(None, ft, "%s %s frame_threshold" % (name, label), rows, bits)


# ---- the debug caps: list overflows, tie rounds and queue re-scans on Wide and WideG words -------------------------------------------
def tied_keys(E, c, what):
    """Integer keys in [0, 40) with the window [12, 24]: every step of the walk is a tie round that removes thousands of VNs,
    many of them sharing a CN, in one round.  vn_threshold and frame_threshold against the host, on the terminated chain."""
    import torch
    p, T = c["p"], c["T"]
    key = (p.dv, p.dc, p.L, p.vns_pos, "tied")
    if key not in _REFS:
        keys = np.random.RandomState(11).randint(0, 40, size=(T, p.n)).astype(np.uint32)
        grid = list(range(12, 25))
        _REFS[key] = (keys, grid, VT.host_reference(p, c["gadj"], keys, 12, 24, True, grid), TH.host_rows(p, c["gadj"], keys, 12, 24, True))
    keys, grid, vn, (rows, bits) = _REFS[key]
    d_keys = torch.from_numpy(keys.view(np.int32)).to(c["d_keys"].device)
    got = E.vn_threshold(p, c["d_adj"][True], d_keys, 12, 24, grid=grid, want_tau=True)
    synchronize()
    r = VT.assert_equals_reference(vn, got, what + " tied keys vn_threshold")
    ft = E.frame_threshold(p, c["d_adj"][True], d_keys, 12, 24, want_bits=True)
    synchronize()
    TH.assert_equals_host(None, ft, what + " tied keys frame_threshold", rows, bits)
    print(what, "tied keys | status:", r[:, 1].tolist(), "| steps:", r[:, 4].tolist(), "| largest release of a step:",
          max(max(x, default=0) for x in vn["releases"]))
    assert (r[:, 4] >= 1).all() and max(max(x, default=0) for x in vn["releases"]) > 1000


@pytest.mark.parametrize("name", list(CAPPED))
def test_small_lists_and_queues_change_no_answer(E, monkeypatch, name):
    """A candidate list of three entries (vn_threshold: chunks sized for one candidate, overflows that halve the chunk, tie
    rounds) and queues of one entry (all four kernels: a re-scan wherever a round queues two CNs) on 2-byte rows, terminated."""
    shape = CAPPED[name]
    assert "-".join(form(shape, True)[:2]) == name
    c = inputs(E, shape)
    p = c["p"]
    ref = reference(E, shape, True)
    what = "%s %d_%d_L%d_N%d" % ((name,) + shape)
    monkeypatch.delenv(QCAP, raising=False)
    monkeypatch.setenv(CCAP, "3")
    got = E.vn_threshold(p, c["d_adj"][True], c["d_keys"], ref["t_lo"], ref["t_hi"], grid=ref["grid"], want_tau=True)
    synchronize()
    r = VT.assert_equals_reference(ref["vn"], got, what + " list of 3")
    print(what, "list of 3 | scans:", r[:, 5].tolist(), "| re-scans:", r[:, 6].tolist(), "| steps:", r[:, 4].tolist())
    walked = ref["vn"]["rows"][:, 4] >= 100
    assert walked.any() and (r[walked, 5] >= ref["vn"]["rows"][walked, 4] // 3).all()      # at most three candidates of a scan
    # a chunk is sized for one candidate and holds more than three with probability 0.019 (Poisson of mean 1): over the
    # thousands of chunks of these walks some list overflows
    assert r[:, 6].sum() > 0
    tied_keys(E, c, what + " list of 3")
    monkeypatch.delenv(CCAP)
    tied_keys(E, c, what)
    # queues of one entry: a frame whose decode at the top of the window has a round that queues two CNs must re-scan
    total, lo, hi = ref["sweep"]
    assert total == p.nk
    look = range(min(c["T"], 3))
    must = [t for t in look if BPE.host_rounds(c["gadj"][t], c["keys"][t].astype(np.int64) < ref["t_hi"], p.nk, p.nk)[1] >= 2]
    assert must, "some frame's decode at the top should queue two CNs in one round"
    free = E.full_bp_eps(p, c["d_adj"][True], c["d_lev"], len(ES))
    synchronize()
    monkeypatch.setenv(QCAP, "1")
    got, vr, fr, cnt, out = run_four(E, c, ref, True, True, what + " queues of one entry")
    monkeypatch.undo()
    rounds_free = free["counters"].cpu().numpy()[:, :, 5]
    print(what, "queues of one entry | frames that must re-scan:", must, "| re-scans of vn_threshold:", vr[:, 6].tolist(),
          "frame_threshold:", fr[:, 6].tolist(), "peel_sweep_eps at the top:", out[0, :, 6].tolist(),
          "| rounds of full_bp_eps at the top:", cnt[0, :, 5].tolist(), "without the cap:", rounds_free[0].tolist())
    assert (vr[must, 6] > 0).all() and (fr[must, 6] > 0).all() and (out[0, must, 6] > 0).all()
    # (full_bp_eps counts no re-scans of its own: a re-scan finds exactly the CNs the lost queue held, so its rounds are the same)
    assert (cnt[:, :, 5] == rounds_free).all()
