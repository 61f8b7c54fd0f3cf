"""`bp_lim_iter --caps` on CPU: the C-ABI's argument checks, the option's parsing, and the driver — one decode with a
checkpoint per cap, every cap with its own ordered stop — writing, cap for cap, the file a single-cap run writes, on one
rank and on two gloo ranks in both shard modes (device work faked as in tests/fakes.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fakes import FakeSimulator

from fl_scaling_sc_ldpc_amd import bp_decoding as B
from fl_scaling_sc_ldpc_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
BAD_ITER = 120          # a frame of CapsFake.bad_frames breaks decodeBP's invariant in this iteration


def caps_counters(key, frames, cap, n, L, bad=()):
    """Counter rows of a decode with MaxNumIt = cap, a pure function of (key, frame, cap).  A frame converges after c
    iterations; with a smaller cap it stops with c - cap more erasures, so failures only shrink as the cap grows.  A frame
    in `bad` breaks the invariant in iteration BAD_ITER: caps above it see status -1 (a cap at or below it does not)."""
    rows = np.zeros((len(frames), E.NCOUNTERS), dtype=np.int32)
    for t, f in enumerate(frames):
        h = (int(f) * 2654435761 + key * 40503 + 777) & 0xFFFFFFFF
        conv = 1 + h % 400                                        # iterations to the fixpoint
        ne = ((1 + h % 5) if (h >> 9) % 4 == 0 else 0) + max(0, conv - cap)
        ne = min(ne, n)
        ee = max(0, ne - 2 * ((h >> 3) % 2))
        it, status = min(cap, conv), 0
        if int(f) in bad and cap > BAD_ITER:
            it, status = BAD_ITER + 1, -1
        rows[t] = [ne, min(L, 1 + ne // 3) if ne else 0, ee, 1 if ee else 0, 0, it, status, n // 2]
    return rows


class CapsFake(FakeSimulator):
    """FakeSimulator with per-cap counters: decode_batch gives the single-cap rows of self.max_it, decode_batch_caps the
    rows of every cap of self.caps for the same frames."""
    bad_frames = ()
    fused_calls = 0

    def _bad(self, sim):
        return {f for (s, f) in self.bad_frames if s == sim}

    def decode_batch(self, nb, want_rows=False):
        sim, idx = self._frames
        cnt = caps_counters(sim + 1000 * self.index, idx, self.max_it, self.p.n, self.p.L, self._bad(sim))
        self.d_cnt[:nb] = torch.from_numpy(cnt)
        return {"counters": self.d_cnt[:nb], "rows": None, "erased": None}

    def decode_batch_caps(self, nb):
        type(self).fused_calls += 1
        sim, idx = self._frames
        return torch.from_numpy(np.stack([caps_counters(sim + 1000 * self.index, idx, k, self.p.n, self.p.L, self._bad(sim))
                                          for k in self.caps]))


def _lib():
    from fl_scaling_sc_ldpc_amd import _lib
    return _lib, _lib.lib()


# ---- C-ABI -------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_caps_without_a_device():
    _l, L = _lib()
    p = _l.CodeParams(4, 8, 20, 100, 200)

    def call(caps, ncaps=None, ntrials=1, fn=L.scldpc_full_bp_caps_device_cn16, params=p):
        arr = (C.c_int32 * max(1, len(caps or [])))(*(caps or [])) if caps is not None else None
        return fn(C.byref(params), ntrials, None, None, None, len(caps or []) if ncaps is None else ncaps, arr, 1, None, None)

    for fn in (L.scldpc_full_bp_caps_device_cn16, L.scldpc_full_bp_caps_device_sock16):
        assert call([], ncaps=0, fn=fn) == -1
        assert call(list(range(1, 18)), fn=fn) == -1                 # 17 caps
        assert b"caps" in L.scldpc_last_error()
        assert call([5, 3], fn=fn) == -1                             # not increasing
        assert call([3, 3], fn=fn) == -1                             # duplicate
        assert call([0, 3], fn=fn) == -1                             # below one
        assert b"strictly increasing" in L.scldpc_last_error()
        assert call(None, ncaps=2, fn=fn) == -1                      # caps NULL
        assert call([3, 5], fn=fn) == -1                             # null buffers with ntrials > 0
        assert call([3, 5], ntrials=-1, fn=fn) == -1
        assert call([3, 5], ntrials=0, fn=fn) == 0                   # empty batch
        assert call(list(range(1, 17)), ntrials=0, fn=fn) == 0       # 16 caps
        assert call([1000000], ntrials=0, fn=fn) == 0
    big = _l.CodeParams(4, 8, 100, 500, 1000)                        # n = 100 000: the socket table only
    assert call([3], ntrials=0, params=big) == -2
    assert b"_sock16" in L.scldpc_last_error()
    assert call([3], ntrials=0, params=big, fn=L.scldpc_full_bp_caps_device_sock16) == 0


def test_engine_checks_caps_like_the_library():
    assert E.check_caps([175, 200, 250]) == (175, 200, 250)
    for bad in ([], list(range(1, 18)), [5, 3], [3, 3], [0, 3], [-1]):
        with pytest.raises(ValueError):
            E.check_caps(bad)


# ---- CLI -----------------------------------------------------------------------------------------------------------
def test_only_bp_lim_iter_takes_caps(capsys):
    opts = B._parser("bp_lim_iter").parse_args(["0", "0", "0", "350", "--caps", "175,200,250,300"])
    assert opts.caps == [175, 200, 250, 300] and opts.MAX_IT == 350
    assert B._parser("bp_lim_iter").parse_args(["0", "0", "0", "350"]).caps is None
    with pytest.raises(SystemExit):
        B._parser("bp_lim_iter").parse_args(["0", "0", "0", "350", "--caps", "175,x"])
    with pytest.raises(SystemExit):
        B._parser("sw_lim_iter").parse_args(["0", "4", "0", "5", "5", "--caps", "3,4"])
    with pytest.raises(SystemExit):
        B._parser("bp_traj").parse_args(["0", "0", "0", "50", "1", "--caps", "3,4"])


def test_sequential_reasons():
    p = E.make_params(4, 8, 10, 10)
    assert B.caps_sequential_reason(p, "philox", 0, "flooding") is None
    assert "glibc" in B.caps_sequential_reason(p, "glibc", 0, "flooding")
    assert "NUM_DOPED" in B.caps_sequential_reason(p, "philox", 2, "flooding")
    assert "fixpoint" in B.caps_sequential_reason(p, "philox", 0, "fixpoint")
    assert "dv = 4" in B.caps_sequential_reason(E.make_params(3, 6, 10, 10), "philox", 0, "flooding")


def _run(monkeypatch, outdir, argv, bad=()):
    monkeypatch.setattr(B, "Simulator", CapsFake)
    monkeypatch.setattr(CapsFake, "bad_frames", tuple(bad))
    opts = B._parser("bp_lim_iter").parse_args(list(argv) + ["--outdir", str(outdir), "--quiet", "--seed", "3"])
    try:
        return B.run_program("bp_lim_iter", opts.INDEX, opts.W, opts.NUM_DOPED, opts.MAX_IT, None, opts)
    except SystemExit as e:
        return e.code


def _files(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


BASE = ["1", "0", "0", "350", "--L", "10", "--N", "10", "--num-points", "3", "--min-frame-err", "40", "--max-frames", "300"]
CAPS = "175,200,50,300"


def _single_cap_files(monkeypatch, tmp_path, argv, its, tag, bad=()):
    want = {}
    for v in its:
        d = tmp_path / ("%s_one%d" % (tag, v))
        a = list(argv)
        a[3] = str(v)
        rc = _run(monkeypatch, d, a, bad)
        want.update(_files(d))
        want[("rc", v)] = rc
    return want


@pytest.mark.parametrize("batch", [7, 64, 2048])
def test_fused_caps_write_the_single_cap_files(monkeypatch, tmp_path, batch):
    argv = BASE + ["--batch", str(batch)]
    want = _single_cap_files(monkeypatch, tmp_path, argv, (50, 175, 200, 300, 350), "b%d" % batch)
    assert all(want[("rc", v)] == 0 for v in (50, 175, 200, 300, 350))
    CapsFake.fused_calls = 0
    d = tmp_path / ("b%d_caps" % batch)
    assert _run(monkeypatch, d, argv + ["--caps", CAPS]) == 0
    assert CapsFake.fused_calls > 0
    got = _files(d)
    assert sorted(got) == sorted(k for k in want if isinstance(k, str)) and len(got) == 5
    for name, text in got.items():
        assert text == want[name], name
    # the caps really stop at different frames: the small caps fail more and stop early
    f = {name: [int(r.split()[9]) for r in text.strip().split("\n")[1:]] for name, text in got.items()}
    assert len({tuple(v) for v in f.values()}) > 1


def test_max_it_zero_and_cap_one_share_a_checkpoint(monkeypatch, tmp_path):
    argv = list(BASE)
    argv[3] = "0"
    want = _single_cap_files(monkeypatch, tmp_path, argv, (0, 1, 3), "z")
    d = tmp_path / "z_caps"
    assert _run(monkeypatch, d, argv + ["--caps", "1,3"]) == 0
    got = _files(d)
    assert len(got) == 3 and all(text == want[name] for name, text in got.items())


def test_a_broken_invariant_stops_only_its_caps(monkeypatch, tmp_path):
    """Frame 11 of point 1 breaks the invariant in iteration BAD_ITER: the caps above it stop writing where their single-cap
    runs abort (after point 0), the caps at or below it write every point, and the process leaves with -1 at the end."""
    bad = [(1, 11)]
    want = _single_cap_files(monkeypatch, tmp_path, BASE, (50, 175, 200, 300, 350), "bad", bad)
    assert want[("rc", 50)] == 0 and all(want[("rc", v)] == -1 for v in (175, 200, 300, 350))
    d = tmp_path / "bad_caps"
    assert _run(monkeypatch, d, BASE + ["--caps", CAPS], bad) == -1
    got = _files(d)
    assert len(got) == 5 and all(text == want[name] for name, text in got.items())
    assert len(got["SC_LDPC_4_8_L10_M5_BP_SW0_175it_Random_BLER_1.dat"].strip().split("\n")) == 2
    assert len(got["SC_LDPC_4_8_L10_M5_BP_SW0_50it_Random_BLER_1.dat"].strip().split("\n")) == 4


@pytest.mark.parametrize("extra,what", [(["--rng", "glibc"], "--rng glibc"), ("doped", "NUM_DOPED")])
def test_glibc_and_doping_run_the_caps_one_after_another(monkeypatch, tmp_path, capsys, extra, what):
    argv = list(BASE) + ["--max-frames", "60"]
    if extra == "doped":
        argv[2] = "2"
        argv.insert(4, "4")                                       # NUM_DOPED = 2: positions MAX_IT (the argv quirk) and 4
        extra = []
    argv += extra
    want = _single_cap_files(monkeypatch, tmp_path, argv, (50, 175, 350), "seq")
    CapsFake.fused_calls = 0
    d = tmp_path / "seq_caps"
    monkeypatch.setattr(B, "Simulator", CapsFake)
    opts = B._parser("bp_lim_iter").parse_args(argv + ["--caps", "50,175", "--outdir", str(d), "--seed", "3"])
    capsys.readouterr()
    assert B.run_program("bp_lim_iter", opts.INDEX, opts.W, opts.NUM_DOPED, opts.MAX_IT, None, opts) == 0
    log = capsys.readouterr().err
    assert "[scldpc] kernels: --caps runs 3 single-cap passes one after another" in log and what in log
    assert CapsFake.fused_calls == 0
    got = _files(d)
    assert len(got) == 3 and all(text == want[name] for name, text in got.items())


# ---- two gloo ranks ------------------------------------------------------------------------------------------------
def _caps_worker(rank, world, port, outdir, argv, bad, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import test_caps_host as T
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    B.Simulator = T.CapsFake
    T.CapsFake.bad_frames = tuple(bad)
    opts = B._parser("bp_lim_iter").parse_args(list(argv) + ["--outdir", outdir, "--quiet", "--seed", "3"])
    try:
        rc = B.run_program("bp_lim_iter", opts.INDEX, opts.W, opts.NUM_DOPED, opts.MAX_IT, None, opts)
    except SystemExit as e:
        rc = e.code
    q.put((rank, rc, T.CapsFake.fused_calls))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _spawn(world, port, outdir, argv, bad=()):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_caps_worker, args=(r, world, port, outdir, argv, bad, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    out = {r: (rc, n) for r, rc, n in (q.get(timeout=180) for _ in range(world))}
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    return out


@pytest.mark.parametrize("bad", [(), ((2, 5),)])
def test_two_ranks_write_the_one_rank_files(tmp_path, bad):
    argv = BASE + ["--batch", "16", "--num-points", "5", "--caps", CAPS]
    port = 35100 + os.getpid() % 1000 + (50 if bad else 0)
    rc_want = -1 if bad else 0
    one = str(tmp_path / "one")
    assert _spawn(1, port, one, argv, bad)[0][0] == rc_want
    want = _files(one)
    assert len(want) == 5
    for k, shard in enumerate(("frames", "points")):
        d = str(tmp_path / shard)
        out = _spawn(2, port + 7 * (k + 1), d, argv + ["--shard", shard], bad)
        assert all(rc == rc_want and n > 0 for rc, n in out.values()), (shard, out)   # both ranks took the fused path
        assert _files(d) == want, shard                                               # part files removed too
