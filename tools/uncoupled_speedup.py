"""What the device rejection sampler (sampler_uncoupled.hip) and batched Philox picks gain for random-pick peeling on the
uncoupled (l,r) ensemble, simulate_peeling_decoder_ldpc_uncoupled.

  old path:  rng="numpy"   ldpc.gen_slots' redraw loop on the host, one trial per launch           (--old-trials, default 8)
  new path:  rng="philox"  sample_philox_uncoupled + peel_pick, a batch per launch                 (--new-trials, default 8192)

at (3,6), M = 1000, e = 0.42, in trials per second; the new path's split into the sampler's launch and the pick kernel's, the
sampler's attempts per second and mean attempts per trial.  At (4,8), M = 1000, e = 0.48 the new path alone (512 trials): the
host loop needs about exp(10.5) = 36 000 redraws of 4000 sockets per graph there and does not finish a trial.
The paths ALTERNATE over --reps repetitions, all values are kept; host clock around work that ends in a device synchronise;
every path warmed up first.  The two paths draw from different generators, so their outputs are not equal trial by trial: the
new path's graphs are checked on the way (every row dv distinct CNs, every CN dc sockets, attempts >= 1) and the mean plr of
both is recorded.  Prints one JSON line; --out writes it too."""
import argparse
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAIN = (3, 6, 1000, 0.42)
HARD = (4, 8, 1000, 0.48)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def graphs_ok(p, d_adj, d_att):
    """every row dv distinct CNs, every CN dc sockets, every trial accepted (device-side checks)"""
    import torch
    s = torch.sort(d_adj, dim=2).values
    distinct = not bool((s[:, :, 1:] == s[:, :, :-1]).any())
    T = d_adj.shape[0]
    flat = d_adj.reshape(T, -1).to(torch.int64) + torch.arange(T, device=d_adj.device)[:, None] * p.cns_pos
    regular = bool((torch.bincount(flat.reshape(-1), minlength=T * p.cns_pos) == p.dc).all())
    return distinct and regular and bool((d_att >= 1).all())


def sampler_and_pick(l, r, M, e, T, reps, max_attempts, seed=11):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    cpp, steps = l * M // r, int(M * (e + 0.1))
    p = E.CodeParams(l, r, 1, cpp, M)
    E.sample_philox_uncoupled(p, seed, 0, min(T, 64), e, max_attempts)                 # warm-up
    t = {"sampler": [], "pick": []}
    attempts, ok = [], True
    for k in range(reps):
        dt, (d_adj, d_ch, d_att) = timed(lambda: E.sample_philox_uncoupled(p, seed, k * T, T, e, max_attempts))
        t["sampler"].append(dt)
        ok = ok and graphs_ok(p, d_adj, d_att)
        attempts.append(int(d_att.to(torch.int64).sum().item()))
        if k == 0:
            E.peel_pick(p, d_adj, d_ch, cpp, steps, seed=seed, trial0=0)               # warm-up
        t["pick"].append(timed(lambda: E.peel_pick(p, d_adj, d_ch, cpp, steps, seed=seed, trial0=k * T))[0])
    return t, attempts, ok


def ms(ts):
    return {"median": round(1e3 * float(np.median(ts)), 3), "all": [round(1e3 * x, 3) for x in ts]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-trials", type=int, default=8)
    ap.add_argument("--new-trials", type=int, default=8192)
    ap.add_argument("--hard-trials", type=int, default=512)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "uncoupled_speedup measures on the GPU"
    sim = PD.simulate_peeling_decoder_ldpc_uncoupled

    l, r, M, e = MAIN
    np.random.seed(5); random.seed(5)
    sim(e, l, r, M, 1)                                                                 # warm-up of both paths
    sim(e, l, r, M, 256, rng="philox", seed=11)
    old, new, plr = [], [], {"numpy": [], "philox": []}
    for k in range(opts.reps):
        dt, res = timed(lambda: sim(e, l, r, M, opts.old_trials))
        old.append(dt); plr["numpy"].append(float(res[2].mean()))
        dt, res = timed(lambda: sim(e, l, r, M, opts.new_trials, rng="philox", seed=11 + k))
        new.append(dt); plr["philox"].append(float(res[2].mean()))
    t, attempts, ok = sampler_and_pick(l, r, M, e, opts.new_trials, opts.reps, 1 << 20)
    old_rate = [opts.old_trials / x for x in old]
    new_rate = [opts.new_trials / x for x in new]
    main_res = {
        "l": l, "r": r, "M": M, "eps": e, "old_trials": opts.old_trials, "new_trials": opts.new_trials,
        "old_s": ms(old), "new_s": ms(new),
        "old_trials_per_s": round(float(np.median(old_rate)), 2), "new_trials_per_s": round(float(np.median(new_rate)), 1),
        "speedup_trials_per_s": round(float(np.median(new_rate) / np.median(old_rate)), 1),
        "new_faster_in_every_repetition": bool(min(new_rate) > max(old_rate)),
        "ms_per_batch": {"sampler": ms(t["sampler"]), "pick": ms(t["pick"])},
        "attempts_per_trial": round(float(np.mean(attempts)) / opts.new_trials, 1),
        "expected_attempts_per_trial": round(math.exp((l - 1) * (r - 1) / 2.0), 1),
        "sampler_attempts_per_s": round(float(np.median([a / x for a, x in zip(attempts, t["sampler"])])), 0),
        "plr_mean": {k: round(float(np.mean(v)), 5) for k, v in plr.items()}, "graphs_ok": ok}

    l, r, M, e = HARD
    t, attempts, ok = sampler_and_pick(l, r, M, e, opts.hard_trials, opts.reps, 1 << 22)
    whole = []
    for k in range(opts.reps):
        whole.append(timed(lambda: sim(e, l, r, M, opts.hard_trials, rng="philox", seed=21 + k, batch=opts.hard_trials,
                                       max_attempts=1 << 22))[0])
    hard_res = {
        "l": l, "r": r, "M": M, "eps": e, "trials": opts.hard_trials,
        "old_path": "not measured: the host loop does not finish a trial (about exp(10.5) = 36 000 redraws per graph)",
        "new_s": ms(whole), "new_trials_per_s": round(opts.hard_trials / float(np.median(whole)), 1),
        "ms_per_batch": {"sampler": ms(t["sampler"]), "pick": ms(t["pick"])},
        "attempts_per_trial": round(float(np.mean(attempts)) / opts.hard_trials, 1),
        "expected_attempts_per_trial": round(math.exp((l - 1) * (r - 1) / 2.0), 1),
        "sampler_attempts_per_s": round(float(np.median([a / x for a, x in zip(attempts, t["sampler"])])), 0),
        "graphs_ok": ok}

    res = {"what": "simulate_peeling_decoder_ldpc_uncoupled: rng='philox' (device rejection sampler + batched Philox picks) vs "
                   "rng='numpy' (host redraw loop, one trial per launch): trials/s, ms per batch by kernel, attempts/s",
           "config": {"reps": opts.reps, "attempts_per_launch_constant": PD.UNCOUPLED_ATTEMPTS_PER_LAUNCH},
           "shapes": {"3_6_M1000": main_res, "4_8_M1000": hard_res},
           "new_path_not_faster_on": [] if main_res["new_faster_in_every_repetition"] else ["3_6_M1000"],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
