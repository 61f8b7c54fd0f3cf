"""Several iteration caps from one decode for the wide form and the pairs (3,6) and (5,10) on the GPU (-m gpu):
scldpc_full_bp_caps_device_{wide,deg,deg_wide} against the CPU oracle cap for cap at small sizes, against the single-cap decoder
of the same family counter for counter (beyond 65 536 CNs too), (4,8) through the _deg forms, a caller's counters buffer, and
`bp_lim_iter --caps --caps-fused on` against single-cap runs file for file.  Everything is integer work: bit-exact, no tolerance.
Inputs are sample_philox(adj16=True) followed by cn_sockets, as in tests/test_gpu_deg.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, require_gpu
from test_gpu_caps import CAP_SETS

pytestmark = pytest.mark.gpu

# ---- 1. against the CPU oracle ----------------------------------------------------------------------------------------------
ORACLE_SHAPES = [(3, 6, 9, 24), (5, 10, 16, 200)]                       # (9, 24): n = 216, ragged; both decoded in test_gpu_deg.py
ORACLE_CAPS = (1, 2, 3, 5, 8, 40, 1000000)
# ε from below to above threshold, seed and first trial of every ε: chosen on the CPU oracle alone (no GPU) so that the reference
# shows every kind of trial test_the_oracle_cases_contain_every_kind_of_trial asks for — (9, 24) gives 31 early finishes,
# (16, 200) gives 35 trials still erased after 40 iterations; both give hundreds of the other two kinds
ORACLE_EPS, ORACLE_SEED, T_ORACLE = (0.02, 0.3, 0.42, 0.46, 0.5, 0.6), 99, 16


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def _tables(E, p, seed, trial0, T, eps):
    a, ch = E.sample_philox(p, seed, trial0, T, eps, adj16=True)
    return a, E.cn_sockets(p, a), ch


@functools.lru_cache(maxsize=None)
def _oracle_cases(shape):
    """The shape's batches with their reference, computed once: [(a, cs, ch, {is_term: int32 [K, T, 8]})], where block k is
    what decodeBP reports with MaxNumIt = ORACLE_CAPS[k] — one oracle decode per cap, nothing shared between caps."""
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    dv, dc, L, N = shape
    p = E.make_params(dv, dc, L, N)
    po = O.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    cases = []
    for i, eps in enumerate(ORACLE_EPS):
        a, cs, ch = _tables(E, p, ORACLE_SEED, 1000 * i, T_ORACLE, eps)
        A = E.adj16_to_global(p, a.cpu().numpy())
        bits = E.unpack_bits(ch.cpu().numpy(), p.n)
        graphs = [O.Graph.from_vn_adj(po, A[t]) for t in range(T_ORACLE)]
        want = {}
        for is_term in (True, False):
            ref = np.zeros((len(ORACLE_CAPS), T_ORACLE, 8), dtype=np.int32)
            for k, cap in enumerate(ORACLE_CAPS):
                for t in range(T_ORACLE):
                    res, _, _ = O.decode_bp(graphs[t], bits[t], max_it=cap, is_term=int(is_term), literal=False)
                    assert res["status"] == 0
                    ref[k, t] = [res["num_erasures"], res["num_blocks_err"], res["num_erasures_exp"], res["num_blocks_err_exp"],
                                 0, res["iterations"], 0, int(bits[t].sum())]
            ref.setflags(write=False)
            want[is_term] = ref
        cases.append((a, cs, ch, want))
    return cases


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=lambda s: "dv%d-dc%d-L%d-N%d" % s)
def test_every_cap_equals_the_cpu_oracle(E, shape, wide):
    import torch
    p = E.make_params(*shape)
    assert E.full_bp_deg_supported(p, wide=wide)
    for i, (a, cs, ch, want) in enumerate(_oracle_cases(shape)):
        for is_term in (True, False):
            got = E.full_bp_caps_deg(p, a, cs, ch, ORACLE_CAPS, is_term=is_term, wide=wide)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert got.shape == want[is_term].shape
            assert (got[:, :, 6] == 0).all()                             # status
            bad = np.argwhere(got != want[is_term])
            assert bad.size == 0, (shape, wide, ORACLE_EPS[i], is_term, bad[:4].tolist())


def test_the_oracle_cases_contain_every_kind_of_trial(E):
    """Over all cases of the reference: trials finished before the first cap (no checkpoint is ever taken), trials still erased
    at the last finite cap, a checkpoint (iterations == cap) whose expurgated count differs from the plain one, and counters
    that differ between two consecutive caps."""
    early = erased_last = exp_differs = step = 0
    last_finite = len(ORACLE_CAPS) - 2
    for shape in ORACLE_SHAPES:
        for _a, _cs, _ch, want in _oracle_cases(shape):
            for ref in want.values():
                early += int((ref[-1, :, 5] <= ORACLE_CAPS[0]).sum())
                erased_last += int(((ref[last_finite, :, 5] == ORACLE_CAPS[last_finite]) & (ref[last_finite, :, 0] > 0)).sum())
                at_cap = ref[:, :, 5] == np.array(ORACLE_CAPS)[:, None]
                exp_differs += int((at_cap & (ref[:, :, 2] != ref[:, :, 0])).sum())
                step += int((ref[1:] != ref[:-1]).any(axis=2).sum())
    assert early > 0 and erased_last > 0 and exp_differs > 0 and step > 0, (early, erased_last, exp_differs, step)


# ---- 2. against the family's single-cap decoder -------------------------------------------------------------------------------
def _single(E, p, form, a, cs, ch, cap, is_term):
    if form == "wide48":
        return E.full_bp_wide(p, a, cs, ch, max_it=cap, is_term=is_term)["counters"]
    return E.full_bp_deg(p, a, cs, ch, max_it=cap, is_term=is_term, wide=form == "degwide")["counters"]


def _fused(E, p, form, a, cs, ch, caps, is_term, **kw):
    if form == "wide48":
        return E.full_bp_caps_wide(p, a, cs, ch, caps, is_term=is_term, **kw)
    return E.full_bp_caps_deg(p, a, cs, ch, caps, is_term=is_term, wide=form == "degwide", **kw)


@functools.lru_cache(maxsize=None)
def _batches(shape, seed, T, eps_trial0):
    from fl_scaling_sc_ldpc_amd import engine as E
    p = E.make_params(*shape)
    return [(eps,) + _tables(E, p, seed, trial0, T, eps) for eps, trial0 in eps_trial0]


SMALL_FORMS = [((3, 6, 20, 200), "deg16"), ((3, 6, 20, 200), "degwide"), ((5, 10, 20, 200), "deg16"),
               ((5, 10, 20, 200), "degwide"), ((4, 8, 16, 200), "wide48")]
SMALL_EPS = tuple((eps, 1000 * i) for i, eps in enumerate((0.40, 0.45, 0.47, 0.48, 0.50)))


@pytest.mark.parametrize("caps", CAP_SETS, ids=lambda c: "caps%d_%d" % (len(c), c[-1]))
@pytest.mark.parametrize("is_term", [True, False])
@pytest.mark.parametrize("shape,form", SMALL_FORMS, ids=lambda v: v if isinstance(v, str) else "dv%d-dc%d-L%d-N%d" % v)
def test_every_cap_equals_the_single_cap_decoder(E, shape, form, is_term, caps):
    """Block k of one fused decode == the family's level decoder with max_it = caps[k] on all eight counters of every trial, on
    Philox batches from ε = 0.40 to 0.50."""
    import torch
    p = E.make_params(*shape)
    for eps, a, cs, ch in _batches(shape, 91, 64, SMALL_EPS):
        got = _fused(E, p, form, a, cs, ch, caps, is_term)
        assert tuple(got.shape) == (len(caps), 64, E.NCOUNTERS)
        for k, cap in enumerate(caps):
            ref = _single(E, p, form, a, cs, ch, cap, is_term)
            assert torch.equal(got[k], ref), (shape, form, is_term, eps, cap, (got[k] != ref).nonzero()[:4].tolist())


# beyond 65 536 CNs only the wide instances run.  (4,8): ε and first trials chosen so that the batches hold frames on both sides
# of the cap range, terminated and truncated — at 0.40 the unlimited decode takes about 40 (truncated: 95) iterations, at 0.49 the
# second frame takes 867 either way (found on the CPU oracle, asserted below on the single-cap wide decoder's iteration counts)
BIG = [((4, 8, 50, 5000), "wide48", ((0.40, 0), (0.49, 2000))),
       ((3, 6, 50, 5000), "degwide", ((0.45, 1000), (0.485, 2000))),
       ((5, 10, 50, 5000), "degwide", ((0.45, 1000), (0.495, 2000)))]
BIG_CAPS = (175, 200, 250, 300, 350)


@pytest.mark.parametrize("is_term", [True, False])
@pytest.mark.parametrize("shape,form,eps_trial0", BIG, ids=["dv4-dc8", "dv3-dc6", "dv5-dc10"])
def test_every_cap_equals_the_single_cap_decoder_beyond_65536_cns(E, shape, form, eps_trial0, is_term):
    import torch
    p = E.make_params(*shape)
    assert p.nk > 65536
    its = []
    for eps, a, cs, ch in _batches(shape, 2024, 16, eps_trial0):
        got = _fused(E, p, form, a, cs, ch, BIG_CAPS, is_term)
        for k, cap in enumerate(BIG_CAPS):
            ref = _single(E, p, form, a, cs, ch, cap, is_term)
            assert torch.equal(got[k], ref), (shape, is_term, eps, cap, (got[k] != ref).nonzero()[:4].tolist())
        its.append(_single(E, p, form, a, cs, ch, 0, is_term)[:, 5].cpu().numpy())
    its = np.concatenate(its)
    if shape[:2] == (4, 8):
        assert (its < 175).any() and (its >= 350).any(), its.tolist()


# ---- 3. (4,8) through the _deg caps forms --------------------------------------------------------------------------------------
def test_4_8_through_the_deg_caps_forms_is_the_sock16_and_wide_result(E):
    import torch
    caps = (3, 40, 175, 1000000)
    for (L, N), wide in (((50, 1000), False), ((16, 200), True)):
        p = E.make_params(4, 8, L, N)
        a, cs, ch = E.sample_philox_sock16(p, 91, 17, 32, 0.48)
        for is_term in (True, False):
            got = E.full_bp_caps_deg(p, a, cs, ch, caps, is_term=is_term, wide=wide)
            ref = (E.full_bp_caps_wide(p, a, cs, ch, caps, is_term=is_term) if wide else
                   E.full_bp_caps_cn16(p, a, cs, ch, caps, is_term=is_term, sockets=True))
            assert torch.equal(got, ref), (L, N, wide, is_term)
            assert len({tuple(r) for r in got[:, :, 5].cpu().numpy().tolist()}) > 1       # the caps bind


# ---- 4. a caller's counters buffer -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form", [((3, 6, 20, 200), "deg16"), ((5, 10, 20, 200), "degwide"), ((4, 8, 16, 200), "wide48")],
                         ids=["deg", "deg_wide", "wide"])
def test_only_the_prefix_of_a_callers_buffer_is_written(E, shape, form):
    import torch
    p = E.make_params(*shape)
    caps, T, SENTINEL = (2, 5, 40), 24, -77
    _eps, a, cs, ch = _batches(shape, 91, 64, SMALL_EPS)[3]
    a, cs, ch = a[:T], cs[:T], ch[:T]
    buf = torch.full(((len(caps) + 1) * T * E.NCOUNTERS,), SENTINEL, dtype=torch.int32, device=a.device)
    view = buf[:len(caps) * T * E.NCOUNTERS].view(len(caps), T, E.NCOUNTERS)
    out = _fused(E, p, form, a, cs, ch, caps, True, counters=view)
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(out, _fused(E, p, form, a, cs, ch, caps, True))
    assert int((out[:, :, 7] == SENTINEL).sum().item()) == 0             # every row written (column 7: channel erasures >= 0)
    assert bool((buf[len(caps) * T * E.NCOUNTERS:] == SENTINEL).all())   # the block behind it untouched


# ---- 5. the CLI, file for file -----------------------------------------------------------------------------------------------------
def _cli(outdir, argv, timeout):
    r = subprocess.run([sys.executable, "-m", "fl_scaling_sc_ldpc_amd.bp_decoding", "bp_lim_iter"] + argv +
                       ["--outdir", str(outdir)], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _files(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("argv,line", [
    (["--dv", "3", "--dc", "6", "--L", "20", "--N", "200", "--num-points", "3", "--min-frame-err", "50", "--max-frames", "4096",
      "--seed", "5", "--batch", "1024"],
     "full_bp_small level-synchronous with 5 cap checkpoints per decode (4-bit CN counts, dv = 3, dc = 6)"),
    (["--N", "5000", "--L", "50", "--num-points", "2", "--min-frame-err", "50", "--max-frames", "128", "--seed", "5",
      "--batch", "64"],
     "full_bp_small wide level-synchronous with 5 cap checkpoints per decode (4-bit CN counts, 32-bit queue entries)"),
], ids=["dv3-dc6", "wide"])
def test_cli_caps_fused_writes_the_single_cap_files(tmp_path, argv, line):
    require_gpu()
    log = _cli(tmp_path / "caps", ["0", "0", "0", "350", "--caps", "175,200,250,300", "--caps-fused", "on"] + argv, 300)
    assert line in log and "one after another" not in log, log
    got = _files(tmp_path / "caps")
    assert len(got) == 5
    for cap in (175, 200, 250, 300, 350):                                # the default single-cap runs
        d = tmp_path / ("one%d" % cap)
        _cli(d, ["0", "0", "0", str(cap), "--quiet"] + argv, 300)
        (name, text), = _files(d).items()
        assert got[name] == text, (cap, argv)
