"""simulate_pd_covariance on two gloo ranks (CPU; the engine calls replaced by pure functions of the GLOBAL trial index, as
tests/test_uncoupled_gloo.py does for its sibling; r1_gram faked with an int64 einsum): both ranks return the gram, moments
and plrs of a single rank, a different batch returns the same, and moments / plrs are those of
simulate_peeling_decoder_ldpc(rng="philox", want_moments=True, moments_from="rows")."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
REPS, STEPS = 11, [0, 3, 4, 17, 110]                 # (4,8), L = 10, M = 20, e = 0.45: num_pd_steps = 110


def _fake_engine(PD):
    import types
    calls = []

    def sample_philox(p, seed, trial0, ntrials, eps, doped=(), device="cpu", out=None, adj16=False, ensemble="olmos"):
        calls.append((trial0, ntrials))
        ids = torch.arange(trial0, trial0 + ntrials, dtype=torch.int64)
        return ids, ids

    def peel_pick(p, d_adj, d_chan, total_size, num_steps, mt_state=None, seed=0, trial0=0, want_r1=True, moments=None):
        assert mt_state is None and int(d_adj[0]) == trial0 and moments is None and want_r1
        T = d_adj.shape[0]
        steps = torch.arange(num_steps + 1, dtype=torch.int64)[None, :]
        r1 = ((d_adj[:, None] * 7919 + steps * 104729 + seed) % 23) * ((steps + d_adj[:, None]) % 5 != 0)
        out = torch.zeros((T, 4), dtype=torch.int32)
        out[:, 0] = (50 + d_adj % 11).to(torch.int32)
        out[:, 1] = (d_adj % 7).to(torch.int32)
        return {"out": out, "r1": r1.to(torch.int32), "moments": None}

    def r1_moments(d_r1, moments=None):
        r = d_r1.to(torch.int64)
        moments[0] += (r != 0).sum(0)
        moments[1] += r.sum(0)
        moments[2] += (r * r).sum(0)
        return moments

    def r1_gram(d_r1, steps, gram=None):
        x = d_r1.to(torch.int64)[:, torch.as_tensor(steps).to(torch.int64)]
        m = (x != 0).to(torch.int64)
        gram[0] += torch.einsum("ti,tj->ij", m, m)
        gram[1] += torch.einsum("ti,tj->ij", x, m)
        gram[2] += torch.einsum("ti,tj->ij", x, x)
        return gram

    PD.E = types.SimpleNamespace(sample_philox=sample_philox, peel_pick=peel_pick, r1_moments=r1_moments, r1_gram=r1_gram,
                                 CodeParams=PD.E.CodeParams)
    return calls


def _worker(rank, world, port, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    calls = _fake_engine(PD)
    f = lambda **kw: PD.simulate_pd_covariance(0.45, 4, 8, 10, 20, False, False, REPS, STEPS, seed=3, device="cpu", **kw)
    steps, gram, mom, plrs = f(batch=3)
    steps2, gram2, mom2, plrs2 = f(batch=4)
    _, mom_ref, plrs_ref = PD.simulate_peeling_decoder_ldpc(0.45, 4, 8, 10, 20, False, False, REPS, [], rng="philox", seed=3, batch=3,
                                                            device="cpu", want_moments=True, moments_from="rows")
    _, r1, _ = PD.simulate_peeling_decoder_ldpc(0.45, 4, 8, 10, 20, False, False, REPS, [], rng="philox", seed=3, batch=5, device="cpu")
    q.put((rank, steps.tolist(), gram.tolist(), mom.tolist(), plrs.tolist(), (steps2.tolist(), gram2.tolist(), mom2.tolist(), plrs2.tolist()),
           mom_ref.tolist(), plrs_ref.tolist(), r1.tolist(), calls[:7]))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_and_another_batch_return_what_one_rank_returns():
    import numpy as np
    ctx = mp.get_context("spawn")
    port = 37500 + os.getpid() % 2000
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
    steps, gram, mom, plrs, other_batch, mom_ref, plrs_ref, r1, calls = one
    assert steps == STEPS
    assert other_batch == (steps, gram, mom, plrs)                       # batch = 4 against batch = 3
    assert mom == mom_ref and plrs == plrs_ref                           # the want_moments call, value for value
    x = np.array(r1, dtype=np.int64)[:, STEPS]
    m = (x != 0).astype(np.int64)
    assert np.array(gram).tolist() == np.stack([m.T @ m, x.T @ m, x.T @ x]).tolist() and np.array(gram).any()
    for k in range(3):                                                   # the diagonal is the moments at the steps
        assert np.diag(np.array(gram)[k]).tolist() == np.array(mom)[k][STEPS].tolist()
    for rank in (0, 1):
        assert res[2][rank][:7] == one[:7], rank
    assert calls == [(0, 3), (3, 3), (6, 3), (9, 2), (0, 4), (4, 4), (8, 3)]
    # contiguous shares by global trial index: 6 + 5 of the 11 trials
    assert res[2][0][8][:4] == [(0, 3), (3, 3), (0, 4), (4, 2)] and res[2][1][8][:4] == [(6, 3), (9, 2), (6, 4), (10, 1)]
