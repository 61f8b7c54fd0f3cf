"""The stopping-set spectrum on the CPU: the symbols of the extension header include/scldpc_ss.h, the two queries and the checks
of its device entry that are decided before any device work (placeholder pointers that are never dereferenced, as
tests/test_cov_host.py), what simulate_sc_ldpc_spectrum and the stopping_sets command line refuse or pass on, and the numpy
reference of the GPU tests (np_spectrum, over pd_oracle.components) on a hand-built graph."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E
from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

ONE = C.c_void_p(256)                                                   # non-null, aligned placeholder
OK, BAD_ARG, TOO_LARGE = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scldpc_ss.h")
ENTRY = "scldpc_ss_spectrum_device"
FORCE = "SCLDPC_DEBUG_SS_FORCE_WORKSPACE"


# ---- the reference of the GPU tests -------------------------------------------------------------------------------------------
def np_spectrum(tr, members, nbins, L, vns_pos):
    """(hist int64 [nbins], pos_hist int64 [L, 8], trial row int64 [4]) of ONE trial from pd_oracle.components: what
    include/scldpc_ss.h defines, bins formed in numpy."""
    from oracle import pd_oracle as P
    members = np.asarray(members, dtype=bool)
    hist, pos_hist = np.zeros(nbins, np.int64), np.zeros((L, 8), np.int64)
    if not members.any():
        hist[0] = 1
        return hist, pos_hist, np.zeros(4, np.int64)
    sizes, comp, idx = P.components(np.asarray(tr), members)
    lowest = np.full(len(sizes), np.iinfo(np.int64).max)
    np.minimum.at(lowest, comp, idx)
    np.add.at(hist, np.minimum(sizes, nbins - 1), 1)
    np.add.at(pos_hist, (lowest // vns_pos, np.minimum(sizes, 8) - 1), 1)
    return hist, pos_hist, np.array([len(sizes), sizes.max(), members.sum(), sizes[sizes > 2].sum()], np.int64)


def np_spectrum_batch(trs, members, nbins, L, vns_pos):
    """The sums over a batch and the rows [T, 4]."""
    parts = [np_spectrum(trs[t], members[t], nbins, L, vns_pos) for t in range(len(trs))]
    return sum(x[0] for x in parts), sum(x[1] for x in parts), np.stack([x[2] for x in parts])


def test_the_reference_on_a_hand_built_graph():
    """Eight VNs of degree 2, two per position, L = 4: {0, 3, 5} chained through CNs 10 and 11, {2, 6} sharing CN 20, {7}
    alone; 1 and 4 are not members, and VN 1 touches CNs 10 and 20, which joins nothing."""
    tr = np.array([[10, 1], [10, 20], [20, 2], [10, 11], [11, 3], [11, 4], [20, 5], [6, 7]])
    members = np.array([1, 0, 1, 1, 0, 1, 1, 1], dtype=bool)
    hist, pos_hist, row = np_spectrum(tr, members, 4, 4, 2)
    assert hist.tolist() == [0, 1, 1, 1]                                 # sizes 1, 2, 3
    want = np.zeros((4, 8), np.int64)
    want[0, 2] = 1                                                       # {0, 3, 5}: lowest member 0, position 0, size 3
    want[1, 1] = 1                                                       # {2, 6}: lowest member 2, position 1
    want[3, 0] = 1                                                       # {7}
    assert (pos_hist == want).all() and row.tolist() == [3, 3, 6, 3]
    hist2, _, _ = np_spectrum(tr, members, 3, 4, 2)
    assert hist2.tolist() == [0, 1, 2]                                   # the last bin takes everything from nbins - 1 on
    hist0, pos0, row0 = np_spectrum(tr, np.zeros(8, bool), 4, 4, 2)
    assert hist0.tolist() == [1, 0, 0, 0] and not pos0.any() and not row0.any()
    hb, pb, rows = np_spectrum_batch([tr, tr], [members, np.zeros(8, bool)], 4, 4, 2)
    assert hb.tolist() == [1, 1, 1, 1] and (pb == want).all() and rows.tolist() == [[3, 3, 6, 3], [0, 0, 0, 0]]


# ---- the header ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(scldpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTS_SS) and len(declared) == 3
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_ENSEMBLES) | set(_lib.EXPORTS_UNCOUPLED) | set(_lib.EXPORTS_UNCOUPLED_WIDE)
              | set(_lib.EXPORTS_COV))
    assert not declared & others                                         # the other headers' coverage rules are as they were
    for name in declared:
        assert hasattr(L, name), name
    assert '#include "scldpc.h"' in text and L.scldpc_abi_version() == 2
    assert "scldpc_ss.h" in open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "Makefile")).read()
    assert "#define SCLDPC_SS_MAX_BINS 4096" in text and _lib.SS_MAX_BINS == 4096 == E.SS_MAX_BINS
    assert "#define SCLDPC_SS_POS_SIZES 8" in text and _lib.SS_POS_SIZES == 8
    assert "#define SCLDPC_SS_BAD_CN 1" in text and _lib.SS_BAD_CN == 1


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "scldpc_ss.h"\nint main(void){'
                   'int (*f)(const scldpc_code_params *) = scldpc_ss_spectrum_form;'
                   'int64_t (*w)(const scldpc_code_params *, int32_t) = scldpc_ss_spectrum_workspace_bytes;'
                   'int (*g)(const scldpc_code_params *, int32_t, const void *, int32_t, const uint32_t *, int32_t, int64_t *,'
                   ' int64_t *, int32_t *, void *, int64_t, void *) = scldpc_ss_spectrum_device;'
                   'return (f==0)+(w==0)+(g==0)+SCLDPC_SS_MAX_BINS-4096+SCLDPC_SS_POS_SIZES-8+SCLDPC_SS_BAD_CN-1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- the queries and the checks, without a device ------------------------------------------------------------------------------
def err():
    return _lib.lib().scldpc_last_error().decode()


def test_form_and_workspace_answer_without_a_device(monkeypatch):
    monkeypatch.delenv(FORCE, raising=False)
    lib = _lib.lib()
    small, mid, bench = E.make_params(3, 6, 10, 128), E.make_params(3, 6, 20, 1500), E.make_params(4, 8, 50, 1000)
    assert E.ss_spectrum_form(small) == 1 and E.ss_spectrum_form(mid) == 2 and E.ss_spectrum_form(bench) == 2
    assert (mid.n, mid.nk) == (30000, 16500) and (bench.n, bench.nk) == (50000, 26500)
    # form 1: the status slot alone; form 2: a slice of parent[n] + cn_rep[ncn] int32 per trial, rounded to 256 bytes
    for T in (0, 1, 77):
        assert lib.scldpc_ss_spectrum_workspace_bytes(C.byref(small), T) == 256
        assert lib.scldpc_ss_spectrum_workspace_bytes(C.byref(mid), T) == 256 + T * 4 * 46528
        assert lib.scldpc_ss_spectrum_workspace_bytes(C.byref(bench), T) == 256 + T * 4 * 76544
    assert 46528 == -(-(30000 + 16500) // 64) * 64 and 76544 == -(-(50000 + 26500) // 64) * 64
    # the largest trial whose state still fits the LDS beside the member words and the fixed regions is form 1, the next is not
    # (3,6), L = 10: 16 M words of state + 4096 bins + 80 + 8 + M / 3.2 member words against 40 960 words of LDS
    assert E.ss_spectrum_form(E.make_params(3, 6, 10, 2250)) == 1 and E.ss_spectrum_form(E.make_params(3, 6, 10, 2260)) == 2
    monkeypatch.setenv(FORCE, "1")                                       # read per call
    assert E.ss_spectrum_form(small) == 2
    assert lib.scldpc_ss_spectrum_workspace_bytes(C.byref(small), 3) == 256 + 3 * 4 * (-(-(1280 + 768) // 64) * 64)
    monkeypatch.setenv(FORCE, "0")
    assert E.ss_spectrum_form(small) == 1


def test_the_queries_refuse_bad_input():
    lib = _lib.lib()
    p = E.make_params(3, 6, 10, 128)
    assert lib.scldpc_ss_spectrum_workspace_bytes(C.byref(p), -1) == -1
    assert err() == "scldpc_ss_spectrum_workspace_bytes: negative ntrials"
    bad = E.CodeParams(3, 6, 10, 64, 127)                                # dv * vns_pos != dc * cns_pos
    assert lib.scldpc_ss_spectrum_workspace_bytes(C.byref(bad), 1) == -1 and "must equal" in err()
    assert lib.scldpc_ss_spectrum_form(C.byref(bad)) == BAD_ARG and "must equal" in err()
    assert lib.scldpc_ss_spectrum_form(None) == BAD_ARG and "null" in err()
    nine = E.CodeParams(9, 18, 4, 8, 16)
    assert lib.scldpc_ss_spectrum_form(C.byref(nine)) == TOO_LARGE and "dv <= 8" in err()
    huge = E.make_params(3, 6, 64, 1 << 20)                              # 2 M words of member bits: beyond one CU's LDS
    assert lib.scldpc_ss_spectrum_form(C.byref(huge)) == TOO_LARGE and "LDS" in err()
    with pytest.raises(E.ScldpcError, match="LDS"):
        E.ss_spectrum_form(huge)


def call(p=None, T=1, adj=ONE, kind=0, members=ONE, nbins=16, hist=ONE, pos=ONE, trial=ONE, ws=ONE, wsb=None):
    p = E.make_params(3, 6, 10, 128) if p is None else p
    if wsb is None:
        wsb = max(_lib.lib().scldpc_ss_spectrum_workspace_bytes(C.byref(p), max(T, 0)), 0)
    rc = _lib.lib().scldpc_ss_spectrum_device(C.byref(p), T, adj, kind, members, nbins, hist, pos, trial, ws, wsb, None)
    return rc, err()


def test_the_entry_refuses_with_a_text_and_no_device(monkeypatch):
    monkeypatch.delenv(FORCE, raising=False)
    # in the header's order: parameters, ntrials, nbins, adj_kind — each judged even for an empty batch
    rc, msg = call(p=E.CodeParams(3, 6, 10, 64, 127), T=-1, nbins=0, kind=7)
    assert rc == BAD_ARG and "must equal" in msg
    rc, msg = call(T=-1, nbins=0, kind=7)
    assert rc == BAD_ARG and msg == ENTRY + ": negative ntrials"
    for nbins in (1, 0, -4, 4097):
        rc, msg = call(nbins=nbins, kind=7, T=0)
        assert rc == BAD_ARG and msg == "%s: 2 <= nbins <= 4096 (got nbins = %d)" % (ENTRY, nbins)
    for kind in (-1, 2, 7):
        rc, msg = call(kind=kind, T=0)
        assert rc == BAD_ARG and "adj_kind is 0" in msg and msg.endswith("got %d" % kind)
    rc, msg = call(p=E.make_params(4, 8, 4, 16384), kind=1, T=0)         # 65536 sockets per position
    assert rc == TOO_LARGE and "vns_pos * dv <= 65535 (got 65536)" in msg
    assert call(p=E.make_params(4, 8, 4, 16384), kind=0, T=0)[0] == OK   # global ids: no such limit
    # an empty batch is fine with any buffers and touches nothing
    assert call(T=0, adj=None, members=None, hist=None, pos=None, trial=None, ws=None, wsb=0)[0] == OK
    for kw in (dict(adj=None), dict(members=None), dict(hist=None), dict(ws=None)):
        rc, msg = call(**kw)
        assert rc == BAD_ARG and msg == ENTRY + ": null buffer", kw
    rc, msg = call(ws=C.c_void_p(260))
    assert rc == BAD_ARG and "16-byte aligned" in msg
    rc, msg = call(wsb=255)
    assert rc == BAD_ARG and msg == "%s: workspace of 255 bytes, 256 needed" % ENTRY
    mid = E.make_params(3, 6, 20, 1500)
    rc, msg = call(p=mid, T=2, wsb=256 + 2 * 4 * 46528 - 1)
    assert rc == BAD_ARG and msg == "%s: workspace of %d bytes, %d needed" % (ENTRY, 256 + 8 * 46528 - 1, 256 + 8 * 46528)


# ---- the simulator and the command line ------------------------------------------------------------------------------------
def test_the_simulator_refuses_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("sample_philox", "peel_sweep", "peel_sweep_sock16", "peel_sweep_sock16_wide", "ss_spectrum", "to_device",
                 "local_device", "_require_gpu", "sample_philox_ens_sock16"):
        monkeypatch.setattr(E, name, no_device)
    f = lambda **kw: PD.simulate_sc_ldpc_spectrum(0.45, 3, 6, 8, 32, True, False, True, kw.pop("tb", False), 10, 5, rng="philox", **kw)
    for nbins in (1, 0, -3, 4097, 2.5, None, "16"):
        with pytest.raises(ValueError, match="spectrum: 2 <= nbins <= 4096"):
            f(nbins=nbins)
    with pytest.raises(ValueError, match="^spectrum: a tail-biting run on position-local tables"):
        f(tb=True, local_tables=True, sweep="small")
    with pytest.raises(ValueError, match="^spectrum: "):
        f(tb=True, local_tables=True)


def test_simulate_sc_ldpc_keeps_its_signature_and_the_spectrum_adds_nbins():
    import inspect
    a, b = inspect.signature(PD.simulate_sc_ldpc), inspect.signature(PD.simulate_sc_ldpc_spectrum)
    assert list(b.parameters)[:-1] == list(a.parameters) and list(b.parameters)[-1] == "nbins"
    assert b.parameters["nbins"].default == 256
    for k, v in a.parameters.items():
        assert b.parameters[k].default == v.default or k == "doping_points", k
    assert list(a.parameters)[-3:] == ["device", "sweep", "local_tables"] and a.parameters["max_fuckups"].default == 2000


ARGV = ["3", "6", "8", "32", "[0.44, 0.45]", "T", "U", "B", "NTB", "300", "20", "[]"]


def test_the_command_line_writes_the_rows_and_the_spectrum(monkeypatch, tmp_path):
    seen = []

    def fake(e, l, r, L, M, term, proto, bounded, tb, reps, fu, doping, **kw):
        seen.append(((e, l, r, L, M, term, proto, bounded, tb, reps, fu, doping), kw))
        t13 = (0.5, 0.25, 0.1, 0.05, 3, 12, 7, 3072, np.zeros(reps), np.zeros(reps), 2, 96, 2 / 96)
        return t13, np.arange(kw.get("nbins", 256), dtype=np.int64) + int(e * 100), np.full((L, 8), int(e * 100), np.int64)
    monkeypatch.setattr(PD, "simulate_sc_ldpc_spectrum", fake)
    monkeypatch.setattr(PD, "simulate_sc_ldpc", lambda *a, **k: pytest.fail("stopping_sets runs the spectrum simulator"))
    out = tmp_path / "o.txt"
    PD.main_stopping_sets([str(out)] + ARGV + ["--nbins", "32", "--rng", "philox", "--seed", "5", "--batch", "64", "--sweep", "small",
                                               "--device", "cpu"])
    assert [s[0] for s in seen] == [(e, 3, 6, 8, 32, True, False, True, False, 300, 20, []) for e in (0.44, 0.45)]
    assert seen[0][1] == dict(nbins=32, rng="philox", seed=5, batch=64, sweep="small", device="cpu")
    lines = out.read_text().splitlines()
    assert lines[0].startswith("# SC-LDPC (3,6,L=8,M=32)") and len(lines) == 3
    assert lines[1].split() == ["0.44", "0.5", "0.25", "0.1", "0.05", "3", "12", "7", "3072", "2", "96", str(2 / 96)]
    with open(str(out) + ".spectrum.pkl", "rb") as f:
        es, hist, pos_hist = PD._ArraysOnly(f).load()                    # numpy arrays only
    assert es.tolist() == [0.44, 0.45] and hist.shape == (2, 32) and pos_hist.shape == (2, 8, 8)
    assert hist[1].tolist() == list(range(45, 77)) and (pos_hist[0] == 44).all() and hist.dtype == np.int64 == pos_hist.dtype


def test_nbins_and_pick_go_where_they_belong(monkeypatch, tmp_path):
    monkeypatch.setattr(PD, "simulate_sc_ldpc_spectrum", lambda *a, **k: pytest.fail("ran"))
    monkeypatch.setattr(PD, "simulate_sc_ldpc", lambda *a, **k: pytest.fail("ran"))
    out = str(tmp_path / "o.txt")
    with pytest.raises(SystemExit, match="--nbins sizes the histogram of stopping_sets"):
        PD.main_simulate_sc_ldpc([out] + ARGV + ["--nbins", "32"])
    with pytest.raises(SystemExit, match="--pick chooses the random-pick decoder"):
        PD.main_stopping_sets([out] + ARGV + ["--pick", "first"])
    assert not os.path.exists(out) and not os.path.exists(out + ".spectrum.pkl")
    src = open(PD.__file__).read()
    assert 'prog == "stopping_sets"' in src and "main_stopping_sets(sys.argv[2:])" in src
