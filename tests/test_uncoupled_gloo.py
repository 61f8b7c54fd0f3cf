"""simulate_peeling_decoder_ldpc_uncoupled(rng="philox") on two gloo ranks (CPU; the two engine calls replaced by pure functions
of the GLOBAL trial index, as tests/test_distributed_gloo.py does for the sibling): both ranks return what a single rank returns,
and rng="numpy" on two ranks raises."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _fake_engine(PD):
    import types
    calls = []

    def sample_philox_uncoupled(p, seed, trial0, ntrials, eps, max_attempts, device="cpu", out=None):
        calls.append((trial0, ntrials))
        ids = torch.arange(trial0, trial0 + ntrials, dtype=torch.int64)
        return ids, ids, (1 + ids % 13).to(torch.int32)

    def peel_pick(p, d_adj, d_chan, total_size, num_steps, mt_state=None, seed=0, trial0=0, want_r1=True, moments=None):
        assert mt_state is None and int(d_adj[0]) == trial0 and total_size == p.cns_pos and moments is None
        T = d_adj.shape[0]
        steps = torch.arange(num_steps + 1, dtype=torch.int64)[None, :]
        r1 = ((d_adj[:, None] * 7919 + steps * 104729 + seed) % 23) * ((steps + d_adj[:, None]) % 5 != 0)
        out = torch.zeros((T, 4), dtype=torch.int32)
        out[:, 0] = (50 + d_adj % 11).to(torch.int32)
        out[:, 1] = (d_adj % 7).to(torch.int32)
        return {"out": out, "r1": r1.to(torch.int32) if want_r1 else None, "moments": None}

    def r1_moments(d_r1, moments=None):
        r = d_r1.to(torch.int64)
        moments[0] += (r != 0).sum(0)
        moments[1] += r.sum(0)
        moments[2] += (r * r).sum(0)
        return moments

    PD.E = types.SimpleNamespace(sample_philox_uncoupled=sample_philox_uncoupled, peel_pick=peel_pick, r1_moments=r1_moments,
                                 CodeParams=PD.E.CodeParams)
    return calls


def _worker(rank, world, port, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    numpy_error = None
    if world > 1:
        try:
            PD.simulate_peeling_decoder_ldpc_uncoupled(0.4, 3, 6, 20, 3, device="cpu")
        except ValueError as e:
            numpy_error = str(e)
    calls = _fake_engine(PD)
    f = PD.simulate_peeling_decoder_ldpc_uncoupled
    first, r1, plrs, nv = f(0.4, 3, 6, 20, 11, device="cpu", rng="philox", seed=3, batch=3)
    _, mom, plrs2, nv2 = f(0.4, 3, 6, 20, 11, device="cpu", rng="philox", seed=3, batch=4, want_moments=True)
    assert first is None
    q.put((rank, r1.tolist(), plrs.tolist(), nv, mom.tolist(), plrs2.tolist(), nv2, calls, numpy_error))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_return_what_one_rank_returns():
    ctx = mp.get_context("spawn")
    port = 36500 + os.getpid() % 2000
    res = {}
    for world in (1, 2):
        q = ctx.Queue()
        procs = [ctx.Process(target=_worker, args=(r, world, port + world, q)) for r in range(world)]
        for pr in procs:
            pr.start()
        got = [q.get(timeout=120) for _ in range(world)]
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
        res[world] = {g[0]: g[1:] for g in got}
    one = res[1][0]
    for rank in (0, 1):
        assert res[2][rank][:6] == one[:6], rank
        assert "single rank only" in res[2][rank][7]                     # rng="numpy" is one sequential stream
    assert one[2] == [50 + t % 11 for t in range(11)] and one[1] == [(50 + t % 11 - t % 7) / 20 for t in range(11)]
    assert one[6] == [(0, 3), (3, 3), (6, 3), (9, 2), (0, 4), (4, 4), (8, 3)]
    # contiguous shares by global trial index: 6 + 5 of the 11 trials
    assert res[2][0][6] == [(0, 3), (3, 3), (0, 4), (4, 2)] and res[2][1][6] == [(6, 3), (9, 2), (6, 4), (10, 1)]
