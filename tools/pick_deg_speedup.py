"""What the ring build of the CN words (cn_build.hip, dv CN positions in LDS) and two trials per wave (peel_pick_multi_kernel) gain
for random-pick peeling on the pairs (3,6) and (5,10), at BASELINE config 3's size and at M = 2000, rows on.

  old path:  sample_philox(adj16) + peel_pick         (simulate_peeling_decoder_ldpc(rng="philox", pick="first"))
  new path:  sample_philox(adj16) + peel_pick_deg     (pick="multi")

The (4,8) row is a control: there both entries run the same kernels, so it shows the noise floor.  Per repetition one batch
(--batch, default 8192: the cap of the simulator's own batch rule; the batch used is recorded) is sampled once and decoded both
ways (the paths ALTERNATE over --reps repetitions, all values are kept; host clock around work that ends in a device synchronise;
every shape warmed up first), and the r1 rows and plrs of the two are compared for equality.
"build" is the decoder's call with num_steps = 0 (the CN words and the degree-1 bitmap, no pick), "pick" the whole call minus
that.  A simulate_peeling_decoder_ldpc pass of --trials trials is run both ways and (r1, plrs) compared.

Each shape is measured by a child process of its own under `timeout -k 10`; the first child that ends with a non-zero status ends
the run with that status (nothing more is started).  Prints one JSON line; --out writes it too.  pick_deg_becomes_default is the
rule of peeling_decoding.PICK_DEG_BY_DEFAULT: on every shape but the control every repetition of the new path is faster than
every repetition of the old one, with equal outputs."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name: l, r, L, M, ε, terminated
SHAPES = {
    "3_6_L50_M10000_N": (3, 6, 50, 10000, 0.45, False),
    "4_8_L50_M10000_N": (4, 8, 50, 10000, 0.45, False),                  # BASELINE config 3's size; the control
    "5_10_L50_M10000_N": (5, 10, 50, 10000, 0.45, False),
    "3_6_L50_M2000_N": (3, 6, 50, 2000, 0.45, False),
    "5_10_L50_M2000_N": (5, 10, 50, 2000, 0.45, False),
}
CONTROL = "4_8_L50_M10000_N"
BATCH = 8192                # the cap of simulate_peeling_decoder_ldpc's own batch rule; profiles/pick_deg_speedup_b2048.json: --batch 2048


def measure(name, reps, trials, batch):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "pick_deg_speedup measures on the GPU"
    l, r, L, M, eps, term = SHAPES[name]
    cpp = int(l / r * M)
    npos = L + l - 1 if term else L
    total_size, steps = cpp * npos, int(M * npos * (eps + 0.1))
    p, B = E.CodeParams(l, r, L, cpp, M), batch
    kind, why = PD.select_pick(p, total_size, "philox", "olmos", "rows", E.peel_pick_deg_supported(p, total_size), "multi")
    assert kind == "multi", why
    a = torch.empty((B, p.n, l), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    decode = {"old": lambda n: E.peel_pick(p, a, ch, total_size, n, seed=11, trial0=0),
              "new": lambda n: E.peel_pick_deg(p, a, ch, total_size, n, seed=11, trial0=0)}
    E.sample_philox(p, 11, 0, B, eps, out=(a, ch))
    for which in ("old", "new"):                                         # warm-up of every kernel
        decode[which](0), decode[which](steps)
    t = {k: [] for k in ("sample", "old_build", "old_call", "new_build", "new_call")}
    equal = True
    for k in range(reps):
        t["sample"].append(timed(lambda: E.sample_philox(p, 11, k * B, B, eps, out=(a, ch)))[0])
        res = {}
        for which in ("old", "new"):
            t[which + "_build"].append(timed(lambda: decode[which](0))[0])
            dt, res[which] = timed(lambda: decode[which](steps))
            t[which + "_call"].append(dt)
        equal = equal and bool(torch.equal(res["old"]["r1"], res["new"]["r1"])) and bool(torch.equal(res["old"]["out"], res["new"]["out"]))
        picks = float(res["old"]["out"][:, 1].float().mean().item())
        del res
    kw = dict(num_repeats=trials, rng="philox", seed=11, batch=B)
    sim = {pick: PD.simulate_peeling_decoder_ldpc(eps, l, r, L, M, term, False, pick=pick, **kw) for pick in ("first", "multi")}
    sims_equal = bool(np.array_equal(sim["first"][1], sim["multi"][1]) and np.array_equal(sim["first"][2], sim["multi"][2]))

    def ms(ts):
        return {"median": round(1e3 * float(np.median(ts)), 3), "all": [round(1e3 * x, 3) for x in ts]}

    old = [s + c for s, c in zip(t["sample"], t["old_call"])]
    new = [s + c for s, c in zip(t["sample"], t["new_call"])]
    return {"l": l, "r": r, "L": L, "M": M, "eps": eps, "terminated": term, "cns": p.nk, "total_size": total_size, "steps": steps,
            "batch": B, "picks_per_trial": round(picks, 1),
            "ms_per_batch": {"sample": ms(t["sample"]),
                             "old_build": ms(t["old_build"]), "old_pick": ms([c - b for c, b in zip(t["old_call"], t["old_build"])]),
                             "new_build": ms(t["new_build"]), "new_pick": ms([c - b for c, b in zip(t["new_call"], t["new_build"])]),
                             "old_sample_and_decode": ms(old), "new_sample_and_decode": ms(new)},
            "old_trials_per_s": round(B / float(np.median(old)), 1), "new_trials_per_s": round(B / float(np.median(new)), 1),
            "speedup_sample_and_decode": round(float(np.median(old) / np.median(new)), 3),
            "speedup_decode": round(float(np.median(t["old_call"]) / np.median(t["new_call"])), 3),
            "every_new_rep_beats_every_old_rep": bool(max(t["new_call"]) < min(t["old_call"])),
            "plr_mean": round(float(sim["first"][2].mean()), 6), "simulate_passes_equal": sims_equal,
            "outputs_equal": bool(equal and sims_equal), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=64, help="trials of the simulate_peeling_decoder_ldpc pass that is compared")
    ap.add_argument("--batch", type=int, default=BATCH, help="trials per batch (reduce it where memory requires)")
    ap.add_argument("--limit", type=int, default=170, help="seconds a shape's child process may take")
    ap.add_argument("--shapes", nargs="*", choices=sorted(SHAPES), default=None)
    ap.add_argument("--one", choices=sorted(SHAPES), default=None, help="measure this shape in this process (the children's mode)")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    if opts.one:
        print(json.dumps(measure(opts.one, opts.reps, opts.trials, opts.batch)), flush=True)
        return 0
    shapes = {}
    for name in (opts.shapes or SHAPES):
        r = subprocess.run(["timeout", "-k", "10", str(opts.limit), sys.executable, os.path.abspath(__file__), "--one", name,
                            "--reps", str(opts.reps), "--trials", str(opts.trials), "--batch", str(opts.batch)], stdout=subprocess.PIPE)
        if r.returncode != 0:
            print("pick_deg_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
        print("pick_deg_speedup: %s done" % name, file=sys.stderr, flush=True)
    judged = {k: s for k, s in shapes.items() if k != CONTROL}
    not_faster = sorted(k for k, s in judged.items() if not s["every_new_rep_beats_every_old_rep"])
    res = {"what": "cn_build ring + peel_pick_multi (peel_pick_deg) vs peel_pick behind sample_philox(adj16) "
                   "(simulate_peeling_decoder_ldpc, rng='philox', rows on): ms per batch by stage, trials/s",
           "config": {"batch": opts.batch, "reps": opts.reps, "simulate_trials": opts.trials, "control": CONTROL},
           "shapes": shapes, "new_path_not_faster_on": not_faster,
           "pick_deg_becomes_default": bool(len(shapes) == len(SHAPES) and not not_faster
                                            and all(s["outputs_equal"] for s in shapes.values()))}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
