"""What the classical ring window decoder saves `bp_lim_iter --window classical` runs: (4,8) at L = 100, N = 2000, W = 10 with 20
iterations per window (the shape of the bench's C4), and each of (3,6), (4,8), (5,10) at L = 50, N = 1000, W = 20 with 6
iterations per window, ε at the pair's waterfall, in batches of 2048 frames.

  old path (Simulator(decoder="swc", ring=False)): sample_philox(adj16) + sw_bp(classical, whole-chain kernel)
  new path (Simulator(decoder="swc", ring=True)):  the CN -> socket table from the sampler ((4,8)) or the cn_sockets pass,
                                                   + sw_bp(classical, ring=True)               (window state in LDS)

Both paths are the Simulator's own fill_batch + decode_batch.  Host clock around work that ends in a device synchronise; every
shape warmed up first; the two paths ALTERNATE over --reps repetitions and all values are kept.  The decoders are also timed
alone.  The counters of the two paths are compared on the way (outputs_equal).

Each shape is measured by a child process of its own under a time limit; the first child that fails or runs out of time ends
the run with its exit status (nothing more is started).  Prints one JSON line; --out writes it too.
classical_ring_becomes_default is the rule of bp_decoding.CLASSICAL_RING_BY_DEFAULT: on every shape every repetition of the
new path is faster end to end than every repetition of the old one, with equal counters."""
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

# name: dv, dc, L, N, W, max_it, ε, frames per timed pass
SHAPES = {
    "4_8_L100_N2000_W10_20it": (4, 8, 100, 2000, 10, 20, 0.47, 8192),
    "4_8_L50_N1000_W20_6it": (4, 8, 50, 1000, 20, 6, 0.47, 16384),
    "3_6_L50_N1000_W20_6it": (3, 6, 50, 1000, 20, 6, 0.46, 16384),
    "5_10_L50_N1000_W20_6it": (5, 10, 50, 1000, 20, 6, 0.47, 16384),
}
BATCH = 2048


def measure(name, reps):
    import torch
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "classical_ring_speedup measures on the GPU"
    dv, dc, L, N, W, max_it, eps, F = SHAPES[name]
    p = E.make_params(dv, dc, L, N)
    assert E.swc_ring_supported(p, W), "the classical ring window decoder does not take this configuration"
    sims = {ring: B.Simulator(p, decoder="swc", W=W, max_it=max_it, batch=BATCH, seed=11, device="cuda:0", ring=ring)
            for ring in (False, True)}
    assert sims[False].path.decoder == "swc_chain" and sims[True].path.decoder == "swc_ring"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def stats(ts, frames):
        med = float(np.median(ts))
        return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                "all_s": [round(x, 4) for x in ts], "trials_per_s": round(frames / med, 1)}

    def path(sim):
        for b0 in range(0, F, BATCH):
            sim.fill_batch(0, eps, b0, BATCH)
            sim.decode_batch(BATCH)

    # warm-up of every kernel and the counters of the two paths compared (one batch)
    for sim in sims.values():
        sim.fill_batch(0, eps, 0, BATCH)
        sim.decode_batch(BATCH)
    torch.cuda.synchronize()
    ro, rn = sims[False].d_cnt, sims[True].d_cnt
    equal = bool(torch.equal(ro, rn))
    iters = float(ro[:, 5].double().mean().item())
    fer = float((ro[:, 0] > 0).double().mean().item())
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(timed(lambda: path(sims[False])))
        t_new.append(timed(lambda: path(sims[True])))
    nrep = max(2, F // BATCH // 2)
    stage = {"sw_ring": [], "sw_bp": []}
    for _ in range(reps):
        stage["sw_ring"].append(timed(lambda: [sims[True].decode_batch(BATCH) for _ in range(nrep)]) / nrep)
        stage["sw_bp"].append(timed(lambda: [sims[False].decode_batch(BATCH) for _ in range(nrep)]) / nrep)
    so, sn = stats(t_old, F), stats(t_new, F)
    return {"dv": dv, "dc": dc, "L": L, "N": N, "W": W, "max_it": max_it, "eps": eps, "batch": BATCH,
            "frames_per_pass": F, "mean_iterations": round(iters, 1), "frame_error_rate": round(fer, 4),
            "old_kernels": sims[False].kernel_choice(), "new_kernels": sims[True].kernel_choice(),
            "old_path": so, "new_path": sn, "speedup_end_to_end": round(so["median_s"] / sn["median_s"], 3),
            "stages_ms_per_batch": {k: {"median": round(1e3 * float(np.median(v)), 3), "all": [round(1e3 * x, 3) for x in v]}
                                    for k, v in stage.items()},
            "speedup_decoder_only": round(float(np.median(stage["sw_bp"]) / np.median(stage["sw_ring"])), 3),
            "every_new_rep_beats_every_old_rep": bool(max(t_new) < min(t_old)), "outputs_equal": equal,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--one", choices=sorted(SHAPES), default=None, help="measure this shape in this process (the children's mode)")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    if opts.one:
        print(json.dumps(measure(opts.one, opts.reps)), flush=True)
        return 0
    shapes = {}
    for name in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(opts.reps)],
                               stdout=subprocess.PIPE, timeout=opts.limit)
        except subprocess.TimeoutExpired:
            print("classical_ring_speedup: %s ran out of its %d s; nothing more is started" % (name, opts.limit), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("classical_ring_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode),
                  file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
    res = {"what": "classical window: whole-chain kernel vs CN -> socket table + classical ring window decoder (sample + decode)",
           "config": {"batch": BATCH, "reps": opts.reps},
           "shapes": shapes,
           "classical_ring_becomes_default": bool(all(s["every_new_rep_beats_every_old_rep"] and s["outputs_equal"]
                                                      for s in shapes.values()))}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
