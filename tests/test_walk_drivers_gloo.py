"""The W > 1 branch of the drivers that decode one sampled code per frame, on CPU under gloo: engine.gather_frames against the
plain concatenation, and run_thresholds / run_vn_thresholds over the engine fakes of tests/test_thresh_host.py and
tests/test_vn_thresh_host.py (rows that are a pure function of the frame number): two ranks return, on both ranks, what one rank
returns, value for value, with a full round, a partial round and a round that leaves one rank without a frame."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(150, 64), (65, 64), (1, 64)]          # frames, batch; on two ranks the last round of (65, 64) and (1, 64) is [1, 0]


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(worker, world, *args):
    """{rank: what worker(rank, world, port, q, *args) put on q}, every rank a spawned process that ended well."""
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + args) for r in range(world)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    return got


def join(rank, world, port):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)


def leave(world):
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ---- engine.gather_frames ---------------------------------------------------------------------------------------------------------
def frames_of(shape, dim, total, lo, hi):
    """Frames lo … hi - 1 of a tensor of `total` frames along `dim`: every element names its frame and its place."""
    full = list(shape)
    full[dim] = total
    t = torch.arange(int(np.prod(full)), dtype=torch.int32).reshape(full) * 7 + 3
    return t.narrow(dim, lo, hi - lo).contiguous()


GATHERS = [((0, 8), 0, [3, 2]), ((4, 0, 8), 1, [2, 3]), ((0, 8), 0, [1, 0])]        # shape (0 at dim), dim, sizes


def _gather_worker(rank, world, port, q):
    join(rank, world, port)
    from fl_scaling_sc_ldpc_amd import engine as E
    out = []
    for shape, dim, sizes in GATHERS:
        lo = sum(sizes[:rank])
        part = frames_of(shape, dim, sum(sizes), lo, lo + sizes[rank]) if sizes[rank] else None       # an idle rank passes None
        got = E.gather_frames(dist, part, sizes, dim, shape=shape, dtype=torch.int32, device="cpu")
        want = frames_of(shape, dim, sum(sizes), 0, sum(sizes))
        out.append(bool(got.is_contiguous() and got.dtype == want.dtype and got.shape == want.shape and (got == want).all()))
    q.put((rank, out))
    leave(world)


def test_gather_frames_equals_the_concatenation_on_both_ranks():
    got = run_ranks(_gather_worker, 2)
    assert got == {0: [True] * len(GATHERS), 1: [True] * len(GATHERS)}


def test_gather_frames_on_one_rank_returns_its_argument():
    from fl_scaling_sc_ldpc_amd import engine as E
    part = frames_of((0, 8), 0, 5, 0, 5)
    assert E.gather_frames(None, part, [5]) is part and E.gather_frames(dist, part, [5], dim=1) is part
    assert E.gather_frames(None, None, [0], shape=(0, 8)) is None


# ---- run_thresholds and run_vn_thresholds -----------------------------------------------------------------------------------------
def _driver_worker(rank, world, port, q, which):
    join(rank, world, port)
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP, engine as E
    import test_thresh_host
    import test_vn_thresh_host
    p = E.make_params(4, 8, 12, 16)
    es = [0.47, 0.40, 0.50, 0.43]
    out = []
    with pytest.MonkeyPatch.context() as mpatch:
        if which == "frame":
            fake = test_thresh_host.FakeEngine(mpatch, index=3, seed=9, doped=(2,))
        else:
            fake = test_vn_thresh_host.FakeEngine(mpatch, index=3, seed=9, doped=(2,))
        for frames, batch in CASES:
            if which == "frame":
                res = BP.run_thresholds(p, 0.40, 0.50, frames, seed=9, index=3, doped=(2,), batch=batch, device="cpu", want_bits=True)
                out.append([res.rows, res.bits])
            else:
                res = BP.run_vn_thresholds(p, 0.40, 0.50, frames, seed=9, es=es, index=3, doped=(2,), batch=batch, device="cpu",
                                           want_tau=True)
                out.append([res.rows, res.pos_thresh, res.counts, res.tau])
        decoded = sum(r[1] for r in fake.rounds)
    q.put((rank, (out, decoded)))
    leave(world)


@pytest.mark.parametrize("which", ["frame", "vn"])
def test_two_ranks_equal_one_rank(which):
    (one, decoded), = run_ranks(_driver_worker, 1, which).values()
    two = run_ranks(_driver_worker, 2, which)
    total = sum(frames for frames, _ in CASES)
    assert decoded == total and two[0][1] + two[1][1] == total and min(two[0][1], two[1][1]) > 0       # the frames are shared
    for i, (frames, batch) in enumerate(CASES):
        assert all(a.shape[0] == frames for a in one[i]) and (one[i][0][:, 1] >= 0).all()
        for rank in (0, 1):
            for a, b in zip(one[i], two[rank][0][i]):
                assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (which, frames, batch, rank)
    assert len(set(one[0][0][:, 1].tolist())) == 3                                 # the 150 frames show every status
