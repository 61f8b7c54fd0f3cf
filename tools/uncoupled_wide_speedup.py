"""What the wide rejection sampler (sampler_uncoupled_wide.hip) gives simulate_peeling_decoder_ldpc_uncoupled beyond the first
sampler's 8192 sockets, and how the two samplers compare where both run.

  (i)  the new ground: (3,6), M = 10000 and M = 5000, e = 0.42
         old path:  rng="numpy"   ldpc.gen_slots' redraw loop on the host, one trial per launch     (--old-trials, default 2)
         new path:  rng="philox"  sample_philox_uncoupled_wide + peel_pick, batches of --new-trials (default 8192)
       in trials per second; the new path's split into the sampler's launch and the pick kernel's, the sampler's attempts per
       second and mean attempts per trial (about exp(5) = 148 is expected).
  (ii) first against wide where both run: (3,6), M = 1000 and M = 2730, the sampler launch alone, the same seeds; the three
       outputs of the two are asserted equal before anything is timed.

The two paths ALTERNATE over --reps repetitions in one process, all values are kept; host clock around work that ends in a device
synchronise; every path warmed up first.  In (i) the two paths draw from different generators, so their outputs are not equal
trial by trial: the new path's graphs are checked on the way (every row dv distinct CNs, every CN dc sockets, attempts >= 1) and
the mean plr of both is recorded.  Prints one JSON line; --out writes it too."""
import argparse
import json
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.uncoupled_speedup import timed, graphs_ok, ms  # noqa: E402

NEW_GROUND = [(3, 6, 10000, 0.42), (3, 6, 5000, 0.42)]
BOTH = [(3, 6, 1000, 0.42), (3, 6, 2730, 0.42)]
MAX_ATTEMPTS = 1 << 20


def new_ground(l, r, M, e, opts):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    sim = PD.simulate_peeling_decoder_ldpc_uncoupled
    T = opts.new_trials
    np.random.seed(5); random.seed(5)
    sim(e, l, r, M, 1)                                                                 # warm-up of both paths
    sim(e, l, r, M, 64, rng="philox", seed=11)
    old, new, plr = [], [], {"numpy": [], "philox": []}
    for k in range(opts.reps):
        dt, res = timed(lambda: sim(e, l, r, M, opts.old_trials))
        old.append(dt); plr["numpy"].append(float(res[2].mean()))
        dt, res = timed(lambda: sim(e, l, r, M, T, rng="philox", seed=11 + k, batch=T))
        new.append(dt); plr["philox"].append(float(res[2].mean()))
        print("# (%d,%d) M=%d rep %d: host loop %.2f s for %d trials, philox %.2f s for %d" % (l, r, M, k, old[-1], opts.old_trials,
                                                                                                new[-1], T), file=sys.stderr, flush=True)
    cpp, steps = l * M // r, int(M * (e + 0.1))
    p = E.CodeParams(l, r, 1, cpp, M)
    t, attempts, ok = {"sampler": [], "pick": []}, [], True
    for k in range(opts.reps):
        dt, (d_adj, d_ch, d_att) = timed(lambda: E.sample_philox_uncoupled_wide(p, 11, k * T, T, e, MAX_ATTEMPTS))
        t["sampler"].append(dt)
        ok = ok and graphs_ok(p, d_adj, d_att)
        attempts.append(int(d_att.to(torch.int64).sum().item()))
        t["pick"].append(timed(lambda: E.peel_pick(p, d_adj, d_ch, cpp, steps, seed=11, trial0=k * T))[0])
        del d_adj, d_ch, d_att
    old_rate = [opts.old_trials / x for x in old]
    new_rate = [T / x for x in new]
    return {
        "l": l, "r": r, "M": M, "eps": e, "sockets": l * M, "old_trials": opts.old_trials, "new_trials": T, "batch": T,
        "old_s": ms(old), "new_s": ms(new),
        "old_trials_per_s": round(float(np.median(old_rate)), 3), "new_trials_per_s": round(float(np.median(new_rate)), 1),
        "speedup_trials_per_s": round(float(np.median(new_rate) / np.median(old_rate)), 1),
        "new_faster_in_every_repetition": bool(min(new_rate) > max(old_rate)),
        "ms_per_batch": {"sampler": ms(t["sampler"]), "pick": ms(t["pick"])},
        "attempts_per_trial": round(float(np.mean(attempts)) / T, 1),
        "expected_attempts_per_trial": round(math.exp((l - 1) * (r - 1) / 2.0), 1),
        "sampler_attempts_per_s": round(float(np.median([a / x for a, x in zip(attempts, t["sampler"])])), 0),
        "plr_mean": {k: round(float(np.mean(v)), 5) for k, v in plr.items()}, "graphs_ok": ok}


def first_against_wide(l, r, M, e, opts):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    T = opts.new_trials
    p = E.CodeParams(l, r, 1, l * M // r, M)
    assert E.uncoupled_supported(p) and E.uncoupled_wide_supported(p)
    a = E.sample_philox_uncoupled(p, 11, 0, T, e, MAX_ATTEMPTS)                        # warm-up, and the equality
    b = E.sample_philox_uncoupled_wide(p, 11, 0, T, e, MAX_ATTEMPTS)
    torch.cuda.synchronize()
    assert all(bool((x == y).all()) for x, y in zip(a, b)), "the two samplers disagree"
    assert bool((a[2] >= 1).all())
    del a, b
    first, wide, attempts = [], [], []
    for k in range(opts.reps):
        dt, out = timed(lambda: E.sample_philox_uncoupled(p, 11, k * T, T, e, MAX_ATTEMPTS))
        first.append(dt)
        attempts.append(int(out[2].to(torch.int64).sum().item()))
        del out
        dt, out = timed(lambda: E.sample_philox_uncoupled_wide(p, 11, k * T, T, e, MAX_ATTEMPTS))
        wide.append(dt)
        assert int(out[2].to(torch.int64).sum().item()) == attempts[-1]
        del out
    return {
        "l": l, "r": r, "M": M, "eps": e, "sockets": l * M, "trials": T, "outputs_equal": True,
        "first_s": ms(first), "wide_s": ms(wide),
        "attempts_per_trial": round(float(np.mean(attempts)) / T, 1),
        "first_attempts_per_s": round(float(np.median([a / x for a, x in zip(attempts, first)])), 0),
        "wide_attempts_per_s": round(float(np.median([a / x for a, x in zip(attempts, wide)])), 0),
        "wide_over_first_time": round(float(np.median(wide) / np.median(first)), 3),
        "wide_faster_in_every_repetition": bool(max(wide) < min(first))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-trials", type=int, default=2)
    ap.add_argument("--new-trials", type=int, default=8192)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "uncoupled_wide_speedup measures on the GPU"
    shapes_i = {"%d_%d_M%d" % s[:3]: new_ground(*s, opts) for s in NEW_GROUND}
    shapes_ii = {"%d_%d_M%d" % s[:3]: first_against_wide(*s, opts) for s in BOTH}
    res = {"what": "simulate_peeling_decoder_ldpc_uncoupled beyond 8192 sockets: rng='philox' (wide device rejection sampler + "
                   "batched Philox picks) vs rng='numpy' (host redraw loop, one trial per launch): trials/s, ms per batch by "
                   "kernel, attempts/s; and sample_philox_uncoupled vs sample_philox_uncoupled_wide, the launch alone, where both run",
           "config": {"reps": opts.reps, "host_loop_trials_per_repetition": opts.old_trials,
                      "wide_attempts_per_launch_constant": PD.UNCOUPLED_WIDE_ATTEMPTS_PER_LAUNCH,
                      "wide_by_default": PD.UNCOUPLED_WIDE_BY_DEFAULT},
           "new_ground": shapes_i, "first_against_wide": shapes_ii,
           "new_path_not_faster_on": [k for k, v in shapes_i.items() if not v["new_faster_in_every_repetition"]],
           "wide_not_faster_on": [k for k, v in shapes_ii.items() if not v["wide_faster_in_every_repetition"]],
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
