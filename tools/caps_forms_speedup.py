"""What `bp_lim_iter --caps --caps-fused on` saves where the one decode is new: trials of more than 65536 CNs (the wide form) and
the pairs (3,6) and (5,10), with the caps of the published BP_Full_{175,200,250,300,350}it family, one ε point per shape, a fixed
number of frames and no stop rule.

  (a) five single-cap passes one after another: per cap, Simulator.run_point on the path a default run takes for the shape
      (what `--caps` does for these shapes without the switch)
  (b) one fused pass: Simulator(caps=…, fused_caps=True).run_point_caps — the frames sampled once, decoded once with a
      checkpoint at every cap

Host clock around work that ends in a device synchronise (run_point reads its counters back); every shape and both ways warmed
up first, with the run counters of every cap compared; (a) and (b) alternate over --reps repetitions and the median is kept,
every repetition is printed with it.  Prints one JSON line; --out writes it too.  The number is recorded, not gated:
CAPS_FORMS_BY_DEFAULT is decided elsewhere."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# dv, dc, L, N, ε, frames, batch: ε a little below each pair's threshold, where the caps of the family bind for most frames
# frames: enough for a timed pass of about a second or more
SHAPES = [(4, 8, 50, 5000, 0.48, 16384, 2048), (3, 6, 50, 1000, 0.47, 131072, 16384), (5, 10, 50, 1000, 0.48, 131072, 16384),
          (3, 6, 50, 5000, 0.47, 16384, 2048)]
CAPS = (175, 200, 250, 300, 350)


def measure(shape, reps, scale):
    import torch
    from fl_scaling_sc_ldpc_amd import bp_decoding as B
    from fl_scaling_sc_ldpc_amd import engine as E
    dv, dc, L, N, eps, frames, batch = shape
    frames = max(batch, int(frames * scale))
    p = E.make_params(dv, dc, L, N)
    kw = dict(decoder="full", is_term=True, batch=batch, seed=11, device="cuda:0")
    singles = [B.Simulator(p, max_it=cap, **kw) for cap in CAPS]
    fused = B.Simulator(p, max_it=CAPS[-1], caps=CAPS, fused_caps=True, **kw)

    def single_cap_passes():
        out = [dict(s.run_point(0, eps, 0, frames).run) for s in singles]
        torch.cuda.synchronize()
        return out

    def fused_pass():
        out = [dict(pt.run) for pt in fused.run_point_caps(0, eps, 0, frames)]
        torch.cuda.synchronize()
        return out

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    ra, rb = single_cap_passes(), fused_pass()                           # warm-up, and the outputs of both ways compared
    assert ra == rb, (shape, ra, rb)
    assert all(r["frames"] == frames for r in rb)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(single_cap_passes))
        tb.append(timed(fused_pass))
    print("(%d,%d) L = %d N = %d: %s / %s s" % (dv, dc, L, N, [round(x, 3) for x in ta], [round(x, 3) for x in tb]),
          file=sys.stderr, flush=True)
    return {"dv": dv, "dc": dc, "L": L, "N": N, "eps": eps, "frames": frames, "batch": batch,
            "single_cap_path": singles[0].kernel_choice(), "fused_path": fused.kernel_choice(),
            "frame_err_per_cap": [r["frame_err"] for r in rb],
            "single_cap_passes_s": round(float(np.median(ta)), 4), "single_cap_passes_s_all": [round(x, 4) for x in ta],
            "fused_pass_s": round(float(np.median(tb)), 4), "fused_pass_s_all": [round(x, 4) for x in tb],
            "speedup": round(float(np.median(ta) / np.median(tb)), 3), "outputs_equal": True}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the frames of every shape")
    ap.add_argument("--shapes", default=None, help="indices into the shape list, e.g. 0,2 (default: all)")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "caps_forms_speedup measures on the GPU"
    picked = [SHAPES[int(i)] for i in opts.shapes.split(",")] if opts.shapes else SHAPES
    res = {"what": "bp_lim_iter --caps --caps-fused on: five single-cap passes vs one fused pass (sample + decode + accumulate)",
           "caps": list(CAPS), "reps": opts.reps, "device": torch.cuda.get_device_name(0),
           "shapes": [measure(shape, opts.reps, opts.scale) for shape in picked]}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
