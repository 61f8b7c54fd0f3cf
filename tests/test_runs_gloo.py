"""Simulator(runs=True) and `--runs` on two gloo ranks (CPU; the engine calls replaced by pure functions of the GLOBAL trial
index, test_runs_host.FakeChain, as tests/test_ss_gloo.py does for its sibling): with the frames of a point sharded both ranks
return the arrays of a single rank, whatever the batch, and the pass sees exactly the frames the point consumed — also where the
stop rule cuts a round short inside one rank's share; with the points sharded rank 0 writes the pickle and the .dat of a single
rank."""
import os
import pickle
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
# (min_frame_err, max_frames, batch): a cut inside rank 1's share of a round; a cut inside rank 0's (rank 1's unused); no cut;
# another batch; rounds nobody looked at, then rounds that were read
CASES = [(10, 40, 16), (6, 40, 16), (0, 37, 4), (10, 40, 5), (9, 64, 4)]
CLI = ["0", "4", "0", "4", "4", "--L", "12", "--N", "100", "--num-points", "5", "--max-frames", "40", "--min-frame-err", "6", "--batch", "16",
       "--seed", "1", "--quiet", "--eps-ini", "0.45", "--eps-delta", "0.01", "--runs"]


def _worker(rank, world, port, outdir, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    from test_runs_host import FakeChain
    seen = []
    FakeChain(seen).install(BP)
    BP.E.init_distributed = lambda: False
    p = BP.E.make_params(4, 8, 12, 100)
    out = []
    for ferr, frames, batch in CASES:
        sim = BP.Simulator(p, decoder="sw", W=4, max_it=4, init_it=4, batch=batch, seed=1, device="cpu", runs=True)
        del seen[:]
        pt = sim.run_point(2, 0.44, ferr, frames)
        plain = BP.Simulator(p, decoder="sw", W=4, max_it=4, init_it=4, batch=batch, seed=1, device="cpu").run_point(2, 0.44, ferr, frames)
        assert plain.runs is None and plain.run == pt.run
        out.append((pt.f, {k: v.tolist() for k, v in pt.runs.items()}, sorted(i for c in seen for i in c)))
    files = {}
    for shard in ("points", "frames"):
        d = os.path.join(outdir, "w%d_%s" % (world, shard))
        assert BP.main("sw_lim_iter", CLI + ["--shard", shard, "--outdir", d]) == 0
        if world > 1:
            dist.barrier()
        names = sorted(os.listdir(d))
        files[shard] = [(n, open(os.path.join(d, n), "rb").read()) for n in names]
    q.put((rank, out, files))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_return_what_one_rank_returns(tmp_path):
    sys.path.insert(0, HERE)
    from test_runs_host import FakeChain
    ctx = mp.get_context("spawn")
    port = 41500 + os.getpid() % 2000
    res = {}
    for world in (1, 2):
        q = ctx.Queue()
        procs = [ctx.Process(target=_worker, args=(r, world, port + world, str(tmp_path), q)) for r in range(world)]
        for pr in procs:
            pr.start()
        got = [q.get(timeout=120) for _ in range(world)]
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
        res[world] = {g[0]: g[1:] for g in got}
    one, files1 = res[1][0]
    for k, (ferr, frames, batch) in enumerate(CASES):
        f, runs, seen = one[k]
        assert seen == list(range(f)), (k, f, seen)                     # the pass saw exactly the frames the point consumed
        want = FakeChain.want(range(f))
        assert all(runs[name] == want[name].tolist() for name in want), k
        for rank in (0, 1):
            assert res[2][rank][0][k][:2] == one[k][:2], (k, rank)       # both ranks return a single rank's arrays
        assert sorted(res[2][0][0][k][2] + res[2][1][0][k][2]) == list(range(f)), k
    assert 16 < one[0][0] < 32                                           # a cut inside rank 1's share of the first round
    assert one[1][0] < 16 and res[2][1][0][1][2] == []                   # a cut inside rank 0's share: rank 1 fed nothing
    assert one[2][0] == 37 and one[3][:2] == one[0][:2]                 # no cut; batch 5 against batch 16
    # the command line: both shard modes, on one rank and on two, leave the same .dat and the same pickle
    (dat, dat_bytes), (pkl, pkl_bytes) = files1["frames"]
    assert pkl == dat + ".runs.pkl" and len(pickle.loads(pkl_bytes)) == 5
    for world in (1, 2):
        for shard in ("points", "frames"):
            for rank in range(world):
                got = res[world][rank][1][shard]
                assert [n for n, _ in got] == [dat, pkl], (world, shard, rank)
                assert got[0][1] == dat_bytes
                a, b = pickle.loads(got[1][1]), pickle.loads(pkl_bytes)
                assert len(a) == len(b) == 5
                for x, y in zip(a, b):
                    assert sorted(x) == sorted(y) and x["eps"] == y["eps"] and x["frames"] == y["frames"]
                    assert all(np.array_equal(x[n], y[n]) and x[n].dtype == np.int64 for n in ("pos", "run_hist", "fail_hist"))
