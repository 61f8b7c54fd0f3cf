"""Buffer contracts of the device entries of include/scldpc_ensembles.h (-m gpu), as tests/test_gpu_buffer_contracts.py keeps
them for include/scldpc.h: every entry of CASES runs with engine._uninit replaced by a poison.Arena — outputs filled with 0xFF,
with 0x5A, or with what a run on other inputs left behind, between two guard zones — and
  * every element of every output equals the CPU reference (the sampler's twin, a table built on the host from its rows,
    pd_oracle's closure and components), under each fill, so a skipped element fails;
  * no guard byte changes and the inputs are bit for bit unchanged;
  * written through a view that starts one trial into a larger allocation, the trials before and behind the view stay untouched.
Columns 5 and 6 of the decoders' rows count the kernel's own rounds and scans: for them only "a count was written" is asserted.
tests/test_sweep_ens_host.py checks that CASES covers every device entry of the header.  Integer work: exact, no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import poison
from conftest import require_gpu
from test_gpu_sweep_ens import TB, PG, host_table, oracle_row, rows_to_global

pytestmark = pytest.mark.gpu

T = 5
# key -> (dv, dc, L, M, eps, terminated, bounded, seed): n = 480 (whole words) and n = 600 (ragged; sweep_start = 100, L = 30)
SHAPES = {"48-L12-M40": (4, 8, 12, 40, 0.39, True, True, 11), "36-L10-M20-U": (3, 6, 10, 20, 0.39, True, False, 19)}
COUNT_COLS = [5, 6]


def geometry(key):
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    dv, dc, L, M, eps, term, bounded, seed = SHAPES[key]
    return PD._Geometry(dv, dc, L, M, term, bounded, [])


@functools.lru_cache(maxsize=None)
def reference(key, ens, alt=False):
    """The CPU twin's code and channel for T trials (alt: another seed and eps, what a stale run leaves behind), the host-built
    tables, and the sweep's rows and lost bits from pd_oracle.  Never modified."""
    from fl_scaling_sc_ldpc_amd import engine as E
    from oracle import oracle as O
    O.build(with_reference=False)
    dv, dc, L, M, eps, term, bounded, seed = SHAPES[key]
    if alt:
        seed, eps = seed + 1000, 0.8 - eps
    g = geometry(key)
    p = g.params
    po = O.Params(dv, dc, p.L, p.cns_pos, p.vns_pos)
    tw = [O.sample_philox(po, seed, t, eps, (), ensemble=ens) for t in range(T)]
    A = np.stack([a for a, _ in tw]).astype(np.int64)
    words = np.stack([c for _, c in tw]).view(np.uint32)
    off = rows_to_global(p, ens, np.zeros((p.n, dv), dtype=np.uint16))
    rows16 = (A - off).astype(np.uint16)
    assert (rows_to_global(p, ens, rows16) == A).all() and (A - off).max() < p.cns_pos and (A - off).min() >= 0
    table = np.stack([host_table(p, A[t]) for t in range(T)])
    bits = E.unpack_bits(words, p.n).astype(bool)
    args = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    out = np.zeros((T, 8), dtype=np.int32)
    lost = np.zeros((T, p.n), dtype=np.uint8)
    for t in range(T):
        lost[t], row = oracle_row(A[t], bits[t], p.cns_pos, *args)
        out[t, :3], out[t, 7] = row, bits[t].sum()
    return dict(p=p, seed=seed, eps=eps, args=args, A=A, rows16=rows16, words=words, table=table, out=out,
                lost=poison.bitmap_expected(lost))


def device_inputs(ref):
    import torch
    return (torch.from_numpy(ref["rows16"].view(np.int16)).cuda(), torch.from_numpy(ref["table"].view(np.int16)).cuda(),
            torch.from_numpy(ref["words"].view(np.int32)).cuda())


# ---- the case table: header symbol -> (ensembles it runs on, run(E, ref, ens) -> outputs, expect(ref) -> wanted) ---------------------
def run_sampler(E, ref, ens, inputs=None):
    d_adj, d_cn, d_ch = E.sample_philox_ens_sock16(ref["p"], ens, ref["seed"], 0, T, ref["eps"])
    return {"rows": d_adj, "table": d_cn, "chan": d_ch}


def expect_sampler(ref):
    return {"rows": ref["rows16"], "table": ref["table"], "chan": ref["words"]}


def run_decoder(wide):
    def run(E, ref, ens, inputs=None):
        fn = E.peel_sweep_sock16_wide if wide else E.peel_sweep_sock16
        res = fn(ref["p"], *(inputs or device_inputs(ref)), *ref["args"], want_lost=True, ensemble=ens)
        return {"out": res["out"], "lost": res["lost"]}
    return run


def expect_decoder(ref):
    return {"out": ref["out"], "lost": ref["lost"]}


CASES = {
    "scldpc_sample_philox_ensemble_device_adj16_sock": ((TB, PG), run_sampler, expect_sampler),
    "scldpc_peel_sweep_device_sock16_tb": ((TB,), run_decoder(False), expect_decoder),
    "scldpc_peel_sweep_device_sock16_tb_wide": ((TB,), run_decoder(True), expect_decoder),
}


def covered_symbols():
    return set(CASES)


def runs():
    return [(sym, ens, key) for sym, (enss, _, _) in CASES.items() for ens in enss for key in SHAPES]


def _host(name, t):
    g = t.cpu().numpy()
    if name == "table":
        return np.sort(g.view(np.uint16), axis=2)                        # a set per CN
    return g.view({"rows": np.uint16, "chan": np.uint32, "lost": np.uint32}.get(name, g.dtype))


def compare(what, got, want):
    assert set(got) == set(want), (what, sorted(got))
    for name, w in want.items():
        g = _host(name, got[name])
        if name == "out":
            count = g[:, COUNT_COLS].astype(np.int64)
            assert ((count >= 0) & (count < 1 << 24)).all(), (what, "a round count was not written", count)
            keep = [c for c in range(8) if c not in COUNT_COLS]
            g, w = g[:, keep], w[:, keep]
        poison.assert_defined_equal("%s %s" % (what, name), g, w)


def synchronize():
    """A device fault ends the session at once: nothing more is started on a GPU that has faulted."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in the buffer-contract tests, stopping: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    from fl_scaling_sc_ldpc_amd import engine
    return engine


def test_the_table_covers_two_shapes_one_of_them_ragged(E):
    ns = [geometry(k).params.n for k in SHAPES]
    assert len(ns) == 2 and ns[0] % 32 == 0 and ns[1] % 32 != 0
    for key in SHAPES:
        p = geometry(key).params
        assert E.ens_sock16_supported(p, TB) and E.ens_sock16_supported(p, PG)
        assert E.peel_sweep_tb_supported(p) and E.peel_sweep_tb_supported(p, wide=True)
        out = reference(key, TB)["out"]
        assert (out[:, 0] == 0).any() and (out[:, 1] > 0).any(), (key, out)    # a trial that decodes and one that fails


@pytest.mark.parametrize("sym,ens,key", runs(), ids=["%s-%s@%s" % (s.replace("scldpc_", ""), e, k) for s, e, k in runs()])
def test_poisoned_outputs_red_zones_and_read_only_inputs(E, monkeypatch, sym, ens, key):
    import torch
    _, run, expect = CASES[sym]
    ref, prime = reference(key, ens), reference(key, ens, True)
    want = expect(ref)
    inputs, prime_inputs = device_inputs(ref), device_inputs(prime)
    before = [t.clone() for t in inputs]
    for mode in poison.MODES:
        arena = poison.Arena(mode)
        monkeypatch.setattr(E, "_uninit", arena)
        if mode == "stale":
            primed = run(E, prime, ens, prime_inputs)                    # another seed and eps first
            synchronize()
            arena.check_guards()
            if "out" in primed:
                primed["out"][:, COUNT_COLS] = -1                        # a stale round count would pass for a written one
            arena.recycle()
        got = run(E, ref, ens, inputs)
        synchronize()
        arena.check_guards()
        assert len(arena.records) == len(got)                            # every output came out of the arena, and nothing else
        compare((sym, ens, key, mode), got, want)
        monkeypatch.undo()
    for a, b in zip(before, inputs):
        assert torch.equal(a, b), (sym, key, "an input was written")


@pytest.mark.parametrize("sym,ens,key", runs(), ids=["%s-%s@%s" % (s.replace("scldpc_", ""), e, k) for s, e, k in runs()])
def test_a_view_one_trial_into_a_larger_allocation(E, sym, ens, key):
    """T trials written through pointers that start one trial into buffers of T + 2 trials (the entries called directly):
    trials 0 and T + 1 of every buffer keep their poison, trials 1 .. T hold the reference."""
    import torch
    ref = reference(key, ens)
    p = ref["p"]
    arena = poison.Arena(0x5A)
    mk = lambda shape, dtype: arena((T + 2,) + shape, dtype=dtype, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if sym == "scldpc_sample_philox_ensemble_device_adj16_sock":
        bufs = {"rows": mk((p.n, p.dv), torch.int16), "table": mk((p.nk, p.dc), torch.int16), "chan": mk((p.nw,), torch.int32)}
        want = expect_sampler(ref)
        E.check(E.lib().scldpc_sample_philox_ensemble_device_adj16_sock(
            C.byref(p), E.ENSEMBLES[ens], ref["seed"], 0, T, float(ref["eps"]), 0, None, bufs["rows"][1].data_ptr(),
            bufs["table"][1].data_ptr(), bufs["chan"][1].data_ptr(), stream))
    else:
        a16, cn, ch = device_inputs(ref)
        bufs = {"out": mk((8,), torch.int32), "lost": mk((p.nw,), torch.int32)}
        want = expect_decoder(ref)
        E.check(getattr(E.lib(), sym)(C.byref(p), T, a16.data_ptr(), cn.data_ptr(), ch.data_ptr(), *[int(x) for x in ref["args"]],
                                      bufs["out"][1].data_ptr(), bufs["lost"][1].data_ptr(), stream))
    synchronize()
    arena.check_guards()
    for name, buf in bufs.items():
        edge = torch.cat([buf[:1], buf[T + 1:]]).cpu().numpy().view(np.uint8)
        assert (edge == 0x5A).all(), (sym, key, name, "a trial outside the view was written")
    compare((sym, ens, key, "view"), {k: v[1:T + 1] for k, v in bufs.items()}, want)
