"""simulate_sc_ldpc_spectrum on two gloo ranks (CPU; the engine calls replaced by pure functions of the GLOBAL trial index, as
tests/test_cov_gloo.py does for its sibling; ss_spectrum faked with a histogram of the trial's id): both ranks return the
tuple, hist and pos_hist of a single rank, another batch returns the same, the tuple is simulate_sc_ldpc's, and the spectrum
counts exactly the o1 trials of the tuple — also where the stop rule cuts a round short inside one rank's share."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
NBINS = 32
ARGS = (0.45, 4, 8, 10, 20, True, False, True, False)
# (num_repeats, max_fuckups, batch): no cut; a cut far into a round; the other ranks' shares unused; another batch; asynchronous rounds
CASES = [(37, 2000, 4), (50, 9, 8), (50, 3, 8), (50, 9, 5), (37, 40, 4)]


def size_of(ids):
    """The one component a fake failed trial is made of."""
    h = (ids * 2654435761 + 12345) & 0xFFFFFFFF
    return torch.where((h >> 7) % 3 != 0, 1 + h % 97, torch.zeros_like(h))


def _fake_engine(PD):
    import types
    calls = []

    def sample_philox(p, seed, trial0, ntrials, eps, doped=(), device="cpu", out=None, adj16=False, ensemble="olmos"):
        ids = torch.arange(trial0, trial0 + ntrials, dtype=torch.int64)
        return ids, ids

    def peel_sweep(p, d_adj, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
        lost = size_of(d_adj)
        out = torch.zeros((d_adj.shape[0], 8), dtype=torch.int32)
        out[:, 0] = lost.to(torch.int32)
        out[:, 1] = torch.where(lost > 2, lost, torch.zeros_like(lost)).to(torch.int32)
        out[:, 2] = (lost > 2).to(torch.int32)
        return {"out": out, "lost": d_adj.clone() if want_lost else None}  # the "lost bits" of the fake: the trial's id

    def accumulate_peel(d_out, run, max_fuckups=0):        # literal loop of PD:668-699 over the rows, in trial order
        r = run.numpy()
        for row in d_out.numpy():
            if max_fuckups > 0 and r[1] >= max_fuckups:
                break
            r[0] += 1; r[1] += row[0] >= 1; r[2] += row[0]; r[3] += row[1] > 0; r[4] += row[1]; r[5] += row[2]
        return run

    def ss_spectrum(p, d_adj, d_members, nbins, hist=None, pos_hist=None, want_trial=False):
        assert (d_adj == d_members).all() and d_adj.numel() > 0 and not want_trial
        calls.append(d_members.tolist())
        s = size_of(d_members)
        hist += torch.bincount(torch.clamp(s, max=nbins - 1), minlength=nbins)
        for t, x in zip(d_members.tolist(), s.tolist()):
            if x:
                pos_hist[t % p.L, min(x, 8) - 1] += 1
        return {"hist": hist, "pos_hist": pos_hist, "trial": None}

    PD.E = types.SimpleNamespace(sample_philox=sample_philox, peel_sweep=peel_sweep, accumulate_peel=accumulate_peel,
                                 ss_spectrum=ss_spectrum, CodeParams=PD.E.CodeParams, NPEELRUN=PD.E.NPEELRUN,
                                 PEELRUN_NAMES=PD.E.PEELRUN_NAMES, SS_MAX_BINS=PD.E.SS_MAX_BINS, SS_POS_SIZES=PD.E.SS_POS_SIZES)
    return calls


def _worker(rank, world, port, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    calls = _fake_engine(PD)
    out = []
    for reps, maxf, batch in CASES:
        kw = dict(num_repeats=reps, max_fuckups=maxf, rng="philox", seed=3, batch=batch, device="cpu")
        del calls[:]
        t13, hist, pos_hist = PD.simulate_sc_ldpc_spectrum(*ARGS, nbins=NBINS, **kw)
        seen = sorted(t for c in calls for t in c)
        t13_plain = PD.simulate_sc_ldpc(*ARGS, **kw)
        same = all((torch.as_tensor(a) == torch.as_tensor(b)).all() for a, b in zip(t13, t13_plain))
        out.append(([float(x) for x in t13[:8]] + [float(x) for x in t13[10:]], hist.tolist(), pos_hist.tolist(), bool(same), seen))
    q.put((rank, out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_and_another_batch_return_what_one_rank_returns():
    ctx = mp.get_context("spawn")
    port = 39500 + os.getpid() % 2000
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
        res[world] = {g[0]: g[1] for g in got}
    one = res[1][0]
    for k, (reps, maxf, batch) in enumerate(CASES):
        t13, hist, pos_hist, same, seen = one[k]
        o1 = int(t13[5])
        assert same                                                      # the tuple is simulate_sc_ldpc's
        assert seen == list(range(o1)), (k, o1, seen)                    # the pass saw exactly the trials of the tuple
        s = size_of(torch.arange(o1))
        want = torch.bincount(torch.clamp(s, max=NBINS - 1), minlength=NBINS)
        assert hist == want.tolist() and sum(hist) == o1 and hist[0] == o1 - int(t13[0] * o1 + 0.5)
        assert sum(map(sum, pos_hist)) == o1 - hist[0] and len(pos_hist) == 10 and len(pos_hist[0]) == 8
        for rank in (0, 1):
            assert res[2][rank][k][:4] == one[k][:4], (k, rank)
        # the two ranks' passes together saw those trials once each
        assert sorted(res[2][0][k][4] + res[2][1][k][4]) == list(range(o1)), k
    assert one[0][0][5] == 37 and one[1][0][5] < 50 and one[2][0][5] < 8  # no cut; a cut; a cut inside rank 0's first share
    assert one[3][:3] == one[1][:3]                                      # batch 5 against batch 8
    assert one[4][0][5] == 37                                            # rounds that nobody looked at, then rounds that were read
