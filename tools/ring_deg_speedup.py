"""What the ring window decoder saves sw_lim_iter runs with the degree pairs (3,6) and (5,10): for each pair, L = 50, N = 1000,
W = 20 with 6 iterations per window and 60 in the first (the reference's sw_lim_iter arguments), and L = 100, N = 2000, W = 10
with 20 iterations (the shape of the bench's C4), ε at the pair's waterfall, in batches of 2048 frames.

  old path (Simulator(ring=False)): sample_philox(adj16) + sw_bp(ring=False)                      (whole-chain kernel)
  new path (Simulator(ring=True)):  sample_philox(adj16) + cn_sockets + sw_bp(ring=True, deg=True) (window state in LDS)

Host clock around work that ends in a device synchronise; every shape warmed up first; the two paths ALTERNATE over --reps
repetitions and all values are kept.  The decoders and the table pass are also timed alone.  The counters of the two paths
are compared on the way (outputs_equal).

Each shape is measured by a child process of its own under a time limit; the first child that fails or runs out of time ends
the run with its exit status (nothing more is started).  Prints one JSON line; --out writes it too.  ring_deg_becomes_default
is the rule of bp_decoding.RING_DEG_BY_DEFAULT: on every shape every repetition of the new path is faster end to end than
every repetition of the old one, with equal counters."""
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

# name: dv, dc, L, N, W, max_it, init_it, ε, frames per timed pass
SHAPES = {
    "3_6_L50_N1000_W20_6it_60init": (3, 6, 50, 1000, 20, 6, 60, 0.46, 32768),
    "5_10_L50_N1000_W20_6it_60init": (5, 10, 50, 1000, 20, 6, 60, 0.47, 32768),
    "3_6_L100_N2000_W10_20it": (3, 6, 100, 2000, 10, 20, 0, 0.46, 16384),
    "5_10_L100_N2000_W10_20it": (5, 10, 100, 2000, 10, 20, 0, 0.47, 16384),
}
BATCH = 2048


def measure(name, reps):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "ring_deg_speedup measures on the GPU"
    dv, dc, L, N, W, max_it, init_it, eps, F = SHAPES[name]
    p = E.make_params(dv, dc, L, N)
    assert E.sw_ring_deg_supported(p, W), "the ring window decoder does not take this configuration"
    B = BATCH
    a = torch.empty((B, p.n, dv), dtype=torch.int16, device="cuda")
    cs = torch.empty((B, p.nk, dc), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, E.NCOUNTERS), dtype=torch.int32, device="cuda")

    def chain(**kw):
        return E.sw_bp(p, a, ch, W, max_it, init_it, ring=False, **kw)

    def ring(**kw):
        return E.sw_bp(p, a, ch, W, max_it, init_it, ring=True, d_cn_sock=cs, deg=True, **kw)

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

    def old_path():
        for b0 in range(0, F, B):
            E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
            chain(counters=cnt)

    def new_path():
        for b0 in range(0, F, B):
            E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
            E.cn_sockets(p, a, out=cs)
            ring(counters=cnt)

    # warm-up of every kernel and the outputs of the two paths compared (one batch)
    E.sample_philox(p, 11, 0, B, eps, out=(a, ch))
    E.cn_sockets(p, a, out=cs)
    ro, rn = chain(want_erased=True), ring(want_erased=True)
    torch.cuda.synchronize()
    equal = bool(torch.equal(ro["counters"], rn["counters"])) and bool(torch.equal(ro["erased"], rn["erased"]))
    iters = float(ro["counters"][:, 5].double().mean().item())
    fer = float((ro["counters"][:, 0] > 0).double().mean().item())
    del ro, rn
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(timed(old_path))
        t_new.append(timed(new_path))
    nrep = max(2, F // B // 2)
    stage = {"sampler": [], "cn_sockets": [], "sw_ring": [], "sw_bp": []}
    for _ in range(reps):
        stage["sampler"].append(timed(lambda: [E.sample_philox(p, 11, 0, B, eps, out=(a, ch)) for _ in range(nrep)]) / nrep)
        stage["cn_sockets"].append(timed(lambda: [E.cn_sockets(p, a, out=cs) for _ in range(nrep)]) / nrep)
        stage["sw_ring"].append(timed(lambda: [ring(counters=cnt) for _ in range(nrep)]) / nrep)
        stage["sw_bp"].append(timed(lambda: [chain(counters=cnt) for _ in range(nrep)]) / nrep)
    so, sn = stats(t_old, F), stats(t_new, F)
    return {"dv": dv, "dc": dc, "L": L, "N": N, "W": W, "max_it": max_it, "init_it": init_it, "eps": eps, "batch": B,
            "frames_per_pass": F, "mean_iterations": round(iters, 1), "frame_error_rate": round(fer, 4),
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
            print("ring_deg_speedup: %s ran out of its %d s; nothing more is started" % (name, opts.limit), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("ring_deg_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
    res = {"what": "(3,6) and (5,10) square window: whole-chain kernel vs cn_sockets + ring window decoder (sample + decode)",
           "config": {"batch": BATCH, "reps": opts.reps},
           "shapes": shapes,
           "ring_deg_becomes_default": bool(all(s["every_new_rep_beats_every_old_rep"] and s["outputs_equal"]
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
