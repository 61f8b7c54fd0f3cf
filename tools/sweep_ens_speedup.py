"""What the position-local tables of the tail-biting and protograph ensembles and the 4-bit sweep decoder on them
(simulate_sc_ldpc(sweep="small", local_tables=True)) gain over the first-generation path of the same run, in batches of 2048
trials.

  old path:  sample_philox(ensemble=...) (int32 rows, global CN ids) + peel_sweep      (sweep="first")
  new path:  sample_philox_ens_sock16 + peel_sweep_sock16(ensemble=...)                 (sweep="small", local_tables=True)

Both are timed end to end (sample + decode, --trials trials per pass) and by stage (sampler alone, decoder alone).  Host clock
around work that ends in a device synchronise; every shape warmed up first; the paths ALTERNATE over --reps repetitions and all
values are kept.  On every repetition a batch of both paths is compared: the VN rows (the new path's plus their position
offsets), the channel words, columns 0-2 and 7 of the decoders' rows and the lost bitmaps.  A simulate_sc_ldpc pass of --trials
trials is run both ways and the two 13-tuples compared.

Each shape is measured by a child process of its own under `timeout -k 10`; the first child that ends with a non-zero status ends
the run with that status (nothing more is started).  Prints one JSON line; --out writes it too.  local_tables_becomes_default is
the rule of peeling_decoding.LOCAL_TABLES_BY_DEFAULT: on every shape every repetition of the new path is faster than every
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

# name: ensemble, l, r, L, M, ε, terminated, bounded (ε: near each tail-biting pair's threshold, so that trials both decode and
# fail; 0.47 for the protograph chains)
SHAPES = {
    "tb_4_8_L50_M1000": ("tail_biting", 4, 8, 50, 1000, 0.39, True, True),
    "tb_4_8_L50_M2000": ("tail_biting", 4, 8, 50, 2000, 0.39, True, True),
    "tb_3_6_L50_M1000": ("tail_biting", 3, 6, 50, 1000, 0.43, True, True),
    "tb_5_10_L50_M1000": ("tail_biting", 5, 10, 50, 1000, 0.35, True, True),
    "proto_4_8_L50_M1000": ("protograph", 4, 8, 50, 1000, 0.47, True, True),
    "proto_4_8_L50_M2000": ("protograph", 4, 8, 50, 2000, 0.47, True, True),
    "proto_3_6_L50_M1000": ("protograph", 3, 6, 50, 1000, 0.47, True, True),
    "proto_5_10_L50_M1000": ("protograph", 5, 10, 50, 1000, 0.47, True, True),
}
BATCH = 2048
COLS = [0, 1, 2, 7]


def measure(name, reps, trials):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "sweep_ens_speedup measures on the GPU"
    ens, l, r, L, M, eps, term, bounded = SHAPES[name]
    g = PD._Geometry(l, r, L, M, term, bounded, [])
    p, B = g.params, BATCH
    kind, sampler = PD.select_sweep(p, "philox", ens, E.peel_sweep_sock16_supported(p), False, False, "small", local_tables=True,
                                    ens_sock16_ok=E.ens_sock16_supported(p, ens),
                                    tb_ok=ens == "tail_biting" and E.peel_sweep_tb_supported(p))
    assert kind == "small", sampler
    geo = (g.total_size, g.sweep_start, g.lost_lo, g.lost_hi)
    a32 = torch.empty((B, p.n, l), dtype=torch.int32, device="cuda")
    a = torch.empty((B, p.n, l), dtype=torch.int16, device="cuda")
    # position offset of every edge: the new path's rows + these are the old path's
    cpos = torch.arange(p.L, device="cuda")[:, None] + torch.arange(l, device="cuda")[None, :]
    if ens == "tail_biting":
        cpos = cpos % p.L
    offs = (cpos * p.cns_pos).repeat_interleave(M, dim=0).to(torch.int32)
    cs = torch.empty((B, p.nk, r), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def old_sample(b0):
        E.sample_philox(p, 11, b0, B, eps, out=(a32, ch), ensemble=ens)

    def new_sample(b0):
        E.sample_philox_ens_sock16(p, ens, 11, b0, B, eps, out=(a, cs, ch))

    def old_decode(want_lost=False):
        return E.peel_sweep(p, a32, ch, *geo, want_lost=want_lost)

    def new_decode(want_lost=False):
        return E.peel_sweep_sock16(p, a, cs, ch, *geo, want_lost=want_lost, ensemble=ens)

    sample = {"old": old_sample, "new": new_sample}
    decode = {"old": old_decode, "new": new_decode}

    def path(which):
        def run():
            for b0 in range(0, trials, B):
                sample[which](b0)
                decode[which]()
        return run

    def batch_of(which, b0):
        a.fill_(-1), a32.fill_(-1), ch.fill_(-1)
        sample[which](b0)
        res = decode[which](want_lost=True)
        torch.cuda.synchronize()
        rows = a32.clone() if which == "old" else (a.to(torch.int32) & 0xFFFF) + offs[None]
        return rows, ch.clone(), res["out"][:, COLS].clone(), res["lost"].clone(), res["out"].clone()

    def same_batch(b0):
        old, new = batch_of("old", b0), batch_of("new", b0)
        return all(bool(torch.equal(x, y)) for x, y in zip(old[:4], new[:4])), old[4], new[4]

    equal, out_old, out_new = same_batch(0)                              # warm-up of every kernel
    t = {"old": [], "new": []}
    stage = {"old_sampler": [], "new_sampler": [], "old_decoder": [], "new_decoder": []}
    nrep = 8
    for k in range(reps):
        for which in ("old", "new"):
            t[which].append(timed(path(which)))
        equal = same_batch((k + 1) * B)[0] and equal
        for which in ("old", "new"):                                     # the decoder on the batch its own sampler left
            stage[which + "_sampler"].append(timed(lambda: [sample[which](0) for _ in range(nrep)]) / nrep)
            stage[which + "_decoder"].append(timed(lambda: [decode[which]() for _ in range(nrep)]) / nrep)
    kw = dict(num_repeats=trials, max_fuckups=10 ** 9, rng="philox", seed=11, batch=B)
    flags = (term, ens == "protograph", bounded, ens == "tail_biting")
    t13 = {sweep: PD.simulate_sc_ldpc(eps, l, r, L, M, *flags, sweep=sweep, local_tables=sweep == "small", **kw)
           for sweep in ("first", "small")}
    tuples_equal = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(t13["first"], t13["small"]))

    def stats(ts):
        med = float(np.median(ts))
        return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                "all_s": [round(x, 4) for x in ts], "trials_per_s": round(trials / med, 1)}

    def show13(x):
        return [float(v) for k, v in enumerate(x) if k not in (8, 9)]    # entries 8 and 9 are arrays of zeros (PD:700)

    o, n = out_old.cpu().numpy(), out_new.cpu().numpy()
    return {"ensemble": ens, "l": l, "r": r, "L": L, "M": M, "eps": eps, "terminated": term, "bounded": bounded, "positions": p.L, "cns": p.nk,
            "total_size": g.total_size, "sweep_start": g.sweep_start, "sampler": sampler, "batch": B, "trials_per_pass": trials,
            "old_path": stats(t["old"]), "new_path": stats(t["new"]),
            "speedup_end_to_end": round(float(np.median(t["old"]) / np.median(t["new"])), 3),
            "stages_ms_per_batch": {k: {"median": round(1e3 * float(np.median(v)), 3), "all": [round(1e3 * x, 3) for x in v]}
                                    for k, v in stage.items()},
            "first_batch": {"failed_trials": int((o[:, 0] > 0).sum()), "old_rounds_mean": round(float(o[:, 5].mean()), 1),
                            "new_rounds_mean": round(float(n[:, 5].mean()), 1), "new_rescans_mean": round(float(n[:, 6].mean()), 2), "new_rescans_max": int(n[:, 6].max()),
                            "trials_that_rescan": int((n[:, 6] > 0).sum())},
            "tuple13_first": show13(t13["first"]), "tuple13_small": show13(t13["small"]), "tuples_equal": bool(tuples_equal),
            "every_new_rep_beats_every_old_rep": bool(max(t["new"]) < min(t["old"])),
            "outputs_equal": bool(equal and tuples_equal), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=16384, help="trials per timed pass and per simulate_sc_ldpc pass")
    ap.add_argument("--limit", type=int, default=170, help="seconds a shape's child process may take")
    ap.add_argument("--shapes", nargs="*", choices=sorted(SHAPES), default=None)
    ap.add_argument("--one", choices=sorted(SHAPES), default=None, help="measure this shape in this process (the children's mode)")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    if opts.one:
        print(json.dumps(measure(opts.one, opts.reps, opts.trials)), flush=True)
        return 0
    shapes = {}
    for name in (opts.shapes or SHAPES):
        r = subprocess.run(["timeout", "-k", "10", str(opts.limit), sys.executable, os.path.abspath(__file__), "--one", name,
                            "--reps", str(opts.reps), "--trials", str(opts.trials)], stdout=subprocess.PIPE)
        if r.returncode != 0:
            print("sweep_ens_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
        print("sweep_ens_speedup: %s done" % name, file=sys.stderr, flush=True)
    not_faster = sorted(k for k, s in shapes.items() if not s["every_new_rep_beats_every_old_rep"])
    res = {"what": "tail-biting / protograph: sample_philox_ens_sock16 + the 4-bit sweep decoder vs sample_philox(ensemble) + "
                   "peel_sweep (simulate_sc_ldpc, rng='philox'): sample + decode, and by stage",
           "config": {"batch": BATCH, "reps": opts.reps, "trials_per_pass": opts.trials},
           "shapes": shapes, "new_path_not_faster_on": not_faster,
           "local_tables_becomes_default": bool(len(shapes) == len(SHAPES) and not not_faster
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
