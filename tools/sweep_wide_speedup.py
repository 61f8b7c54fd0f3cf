"""What the wide 4-bit sweep decoder (peel_sweep_small.hip, WIDE instances: 32-bit queue entries, one trial per CU) and the sampler
that writes its CN -> socket table gain over the first-generation path of simulate_sc_ldpc's throughput mode at more than 65 536
CNs per trial, in batches of 2048 trials (--batch; the batch used is recorded).

  old path:  sample_philox(adj16) + peel_sweep                        (simulate_sc_ldpc(rng="philox", sweep="first"))
  new path:  the sampler select_sweep names + peel_sweep_sock16_wide   (sweep="wide")

Both are timed end to end (sample + decode, --trials trials per pass) and by stage (sampler alone, decoder alone).  Host clock
around work that ends in a device synchronise; every shape warmed up first; the paths ALTERNATE over --reps repetitions and all
values are kept.  On every repetition a batch of both paths is compared: the VN rows, the channel words, columns 0-2 and 7 of
the decoders' rows and the lost bitmaps.  A simulate_sc_ldpc pass of --trials trials is run both ways and the two 13-tuples
compared.  Per shape: sampler ms, decoder ms, pass s, the end-to-end ratio, re-scans per trial (column 6 over the compared
batches) and the frame error rate.

Each shape is measured by a child process of its own under `timeout -k 10`; the first child that ends with a non-zero status ends
the run with that status (nothing more is started).  Prints one JSON line; --out writes it too.  sweep_wide_becomes_default is
the rule of peeling_decoding.SWEEP_WIDE_BY_DEFAULT: on every shape every repetition of the new path is faster than every
repetition of the old one, with equal outputs."""
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

# name: l, r, L (the caller's), M, ε, terminated, bounded
SHAPES = {
    "4_8_L50_M5000_T_B": (4, 8, 50, 5000, 0.48, True, True),              # 132 500 CNs
    "4_8_L50_M2000_N_U": (4, 8, 50, 2000, 0.48, False, False),            # 90 positions, 93 000 CNs
    "4_8_L100_M1000_N_U": (4, 8, 100, 1000, 0.48, False, False),          # 140 positions, 71 500 CNs
    "3_6_L50_M5000_T_B": (3, 6, 50, 5000, 0.42, True, True),              # 130 000 CNs
    "5_10_L50_M4000_T_B": (5, 10, 50, 4000, 0.49, True, True),            # 108 000 CNs, S = 20 000 sockets per position
}
BATCH = 2048
COLS = [0, 1, 2, 7]


def measure(name, reps, trials, batch):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "sweep_wide_speedup measures on the GPU"
    l, r, L, M, eps, term, bounded = SHAPES[name]
    g = PD._Geometry(l, r, L, M, term, bounded, [])
    p, B = g.params, batch
    kind, sampler = PD.select_sweep(p, "philox", "olmos", False, E.sock16_supported(p), E.deg_sock16_supported(p), "wide",
                                    wide_ok=E.peel_sweep_wide_supported(p), wide_sock16_ok=E.wide_sock16_supported(p))
    assert kind == "wide", sampler
    geo = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    a = torch.empty((B, p.n, l), dtype=torch.int16, device="cuda")
    cs = torch.empty((B, p.nk, r), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def old_sample(b0):
        E.sample_philox(p, 11, b0, B, eps, out=(a, ch))

    def new_sample(b0):
        if sampler == "sample_philox_sock16":
            E.sample_philox_sock16(p, 11, b0, B, eps, out=(a, cs, ch))
        elif sampler == "sample_philox_deg_sock16":
            E.sample_philox_deg_sock16(p, 11, b0, B, eps, out=(a, cs, ch))
        elif sampler == "sample_philox_wide_sock16":
            E.sample_philox_wide_sock16(p, 11, b0, B, eps, out=(a, cs, ch))
        else:
            E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
            E.cn_sockets(p, a, out=cs)

    def old_decode(want_lost=False):
        return E.peel_sweep(p, a, ch, *geo, want_lost=want_lost)

    def new_decode(want_lost=False):
        return E.peel_sweep_sock16_wide(p, a, cs, ch, *geo, want_lost=want_lost)

    sample = {"old": old_sample, "new": new_sample}
    decode = {"old": old_decode, "new": new_decode}

    def path(which):
        def run():
            for b0 in range(0, trials, B):
                sample[which](b0)
                decode[which]()
        return run

    def batch_of(which, b0):
        a.fill_(-1), ch.fill_(-1)
        sample[which](b0)
        res = decode[which](want_lost=True)
        torch.cuda.synchronize()
        return a.clone(), ch.clone(), res["out"][:, COLS].clone(), res["lost"].clone(), res["out"].clone()

    def same_batch(b0):
        old, new = batch_of("old", b0), batch_of("new", b0)
        return all(bool(torch.equal(x, y)) for x, y in zip(old[:4], new[:4])), old[4], new[4]

    equal, out_old, out_new = same_batch(0)                              # warm-up of every kernel
    rescans = [out_new[:, 6].float().mean().item()]
    t = {"old": [], "new": []}
    stage = {"old_sampler": [], "new_sampler": [], "old_decoder": [], "new_decoder": []}
    nrep = 8
    for k in range(reps):
        for which in ("old", "new"):
            t[which].append(timed(path(which)))
        same, _, new_rows = same_batch((k + 1) * B)
        equal = same and equal
        rescans.append(new_rows[:, 6].float().mean().item())
        for which in ("old", "new"):                                     # the decoder on the batch its own sampler left
            stage[which + "_sampler"].append(timed(lambda: [sample[which](0) for _ in range(nrep)]) / nrep)
            stage[which + "_decoder"].append(timed(lambda: [decode[which]() for _ in range(nrep)]) / nrep)
    kw = dict(num_repeats=trials, max_fuckups=10 ** 9, rng="philox", seed=11, batch=B)
    t13 = {sweep: PD.simulate_sc_ldpc(eps, l, r, L, M, term, False, bounded, False, sweep=sweep, **kw) for sweep in ("first", "wide")}
    tuples_equal = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(t13["first"], t13["wide"]))

    def stats(ts):
        med = float(np.median(ts))
        return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                "all_s": [round(x, 4) for x in ts], "trials_per_s": round(trials / med, 1)}

    def show13(x):
        return [float(v) for k, v in enumerate(x) if k not in (8, 9)]    # entries 8 and 9 are arrays of zeros (PD:700)

    o, n = out_old.cpu().numpy(), out_new.cpu().numpy()
    return {"l": l, "r": r, "L": L, "M": M, "eps": eps, "terminated": term, "bounded": bounded, "positions": p.L, "cns": p.nk,
            "total_size": g.total_size, "sweep_start": g.sweep_start, "sampler": sampler, "batch": B, "trials_per_pass": trials,
            "old_path": stats(t["old"]), "new_path": stats(t["new"]),
            "speedup_end_to_end": round(float(np.median(t["old"]) / np.median(t["new"])), 3),
            "stages_ms_per_batch": {k: {"median": round(1e3 * float(np.median(v)), 3), "all": [round(1e3 * x, 3) for x in v]}
                                    for k, v in stage.items()},
            "first_batch": {"failed_trials": int((o[:, 0] > 0).sum()), "old_rounds_mean": round(float(o[:, 5].mean()), 1),
                            "new_rounds_mean": round(float(n[:, 5].mean()), 1), "new_rescans_mean": round(float(n[:, 6].mean()), 2)},
            "rescans_per_trial": round(float(np.mean(rescans)), 4), "fer": round(float((o[:, 0] > 0).mean()), 4),
            "tuple13_first": show13(t13["first"]), "tuple13_wide": show13(t13["wide"]), "tuples_equal": bool(tuples_equal),
            "every_new_rep_beats_every_old_rep": bool(max(t["new"]) < min(t["old"])),
            "outputs_equal": bool(equal and tuples_equal), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=8192, help="trials per timed pass and per simulate_sc_ldpc pass")
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
            print("sweep_wide_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
        print("sweep_wide_speedup: %s done" % name, file=sys.stderr, flush=True)
    not_faster = sorted(k for k, s in shapes.items() if not s["every_new_rep_beats_every_old_rep"])
    res = {"what": "wide 4-bit sweep decoder + the sampler that writes its CN -> socket table vs sample_philox(adj16) + peel_sweep "
                   "(simulate_sc_ldpc, rng='philox'): sample + decode, and by stage",
           "config": {"batch": opts.batch, "reps": opts.reps, "trials_per_pass": opts.trials},
           "shapes": shapes, "new_path_not_faster_on": not_faster,
           "sweep_wide_becomes_default": bool(len(shapes) == len(SHAPES) and not not_faster
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
