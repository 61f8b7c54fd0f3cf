"""What bp_lim_iter's whole eps grid from one sampled code costs per batch of frames (bp_decoding.run_grid_fused's round:
sample_philox + engine.channel_levels + engine.full_bp_eps, csrc/full_bp_eps.hip) beside the loop it replaces, one sampler and one
fixpoint decode per eps point:

  * fused   one first-generation sampler launch at max(es), one levels launch, one decoder launch that walks the 26 points;
  * loop    for every eps: Simulator(schedule="fixpoint").fill_batch + decode_batch — whatever path select_path gives
            `bp_lim_iter 0 0 0 1000000 --schedule fixpoint` at the shape (its label is recorded).

Both sides decode the frames of point 0 (the same codes at every eps), so their counters can be compared: columns 0-4, 6, 7 of every
point, in every repetition.  Shapes: BASELINE config 2's — (4,8), L = 50, N = 1000 — then (3,6) and (5,10) at N = 1000 and (4,8)
at N = 5000, where the CN words of full_bp_eps live in the workspace; the shipped grid 0.48 - k * 0.00125, k < 26; batches of 2048
frames (no stop rule: every point sees every frame).  Device events around whole variants, two warm-ups of every variant, --reps
alternating repetitions, all values kept.  The per-launch times of the fused path are taken in passes of their own, and the
decoder's split between stage 0 and the later stages from K = 1 against K = 26 (no timers inside the kernel).  Prints one JSON
line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ES = [0.48 - k * 0.00125 for k in range(26)]
SHAPES = {                                                                # name: (dv, dc, L, N)
    "4-8-N1000": (4, 8, 50, 1000),
    "3-6-N1000": (3, 6, 50, 1000),
    "5-10-N1000": (5, 10, 50, 1000),
    "4-8-N5000": (4, 8, 50, 5000),
}
COLS = [0, 1, 2, 3, 4, 6, 7]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "bp_eps_fused_speed measures on the GPU"
    B, K = opts.batch, len(ES)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, res

    def ms(ts):
        return {"median": round(1e3 * float(np.median(ts)), 3), "all": [round(1e3 * x, 3) for x in ts]}

    shapes = {}
    for name in opts.shapes.split(","):
        dv, dc, L, N = SHAPES[name]
        p = E.make_params(dv, dc, L, N)
        a16 = p.cns_pos <= 65536
        sim = BP.Simulator(p, max_it=1000000, schedule="fixpoint", batch=B, seed=11, device="cuda:0")
        d_adj = torch.empty((B, p.n, p.dv), dtype=torch.int16 if a16 else torch.int32, device="cuda:0")
        d_ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda:0")
        d_lev = torch.empty((B, p.n), dtype=torch.uint8, device="cuda:0")
        d_cnt = torch.empty((K, B, 8), dtype=torch.int32, device="cuda:0")
        d_loop = torch.empty((K, B, 8), dtype=torch.int32, device="cuda:0")

        def fused(k, es=ES):
            key = BP.trial_key(0, 0, k * B)
            E.sample_philox(p, 11, key, B, es[0], (), out=(d_adj, d_ch))
            E.channel_levels(p, 11, key, B, es, (), out=d_lev)
            return E.full_bp_eps(p, d_adj, d_lev, len(es), counters=d_cnt[:len(es)])["counters"]

        def loop(k):
            for i, e in enumerate(ES):
                sim.fill_batch(0, e, k * B, B)
                d_loop[i].copy_(sim.decode_batch(B)["counters"])
            return d_loop

        variants = {"fused": fused, "loop": loop}
        for k in range(2):                                               # warm-up of every variant, in the order of the timed loop
            for fn in variants.values():
                fn(k)
            fused(k, ES[:1])
        times = {v: [] for v in variants}
        equal, faster = True, True
        for k in range(opts.reps):                                       # alternating: one repetition of every variant in turn
            outs = {}
            for v, fn in variants.items():
                dt, out = event_timed(lambda: fn(k))
                times[v].append(dt)
                outs[v] = out[:, :, COLS].cpu().numpy()
            equal = equal and bool((outs["loop"] == outs["fused"]).all())
            faster = faster and times["fused"][-1] < times["loop"][-1]
        failing = (outs["fused"][:, :, 0] > 0).sum(axis=1).tolist()
        # the launches of the fused path, each in passes of its own; the decoder at K = 1 for the split; the loop's two calls at eps[0]
        t_sample, t_levels, t_dec, t_dec1, t_fill, t_decode = [], [], [], [], [], []
        for k in range(opts.reps):
            key = BP.trial_key(0, 0, k * B)
            t_sample.append(event_timed(lambda: E.sample_philox(p, 11, key, B, ES[0], (), out=(d_adj, d_ch)))[0])
            t_levels.append(event_timed(lambda: E.channel_levels(p, 11, key, B, ES, (), out=d_lev))[0])
            t_dec.append(event_timed(lambda: E.full_bp_eps(p, d_adj, d_lev, K, counters=d_cnt))[0])
            d_lev1 = E.channel_levels(p, 11, key, B, ES[:1])
            t_dec1.append(event_timed(lambda: E.full_bp_eps(p, d_adj, d_lev1, 1, counters=d_cnt[:1]))[0])
            t_fill.append(event_timed(lambda: sim.fill_batch(0, ES[0], k * B, B))[0])
            t_decode.append(event_timed(lambda: sim.decode_batch(B))[0])
        med = {v: float(np.median(t)) for v, t in times.items()}
        shapes[name] = {
            "shape": {"dv": dv, "dc": dc, "L": L, "N": N, "n": p.n, "ncn": p.nk},
            "loop_kernels": sim.kernel_choice(),
            "failing_frames_per_point_of_last_batch": failing,
            "ms_per_batch": {v: ms(t) for v, t in times.items()},
            "loop_over_fused": round(med["loop"] / med["fused"], 3),
            "fused_faster_in_every_repetition": faster,
            "fused_launches_ms": {"sample_philox": ms(t_sample), "channel_levels": ms(t_levels), "full_bp_eps_K26": ms(t_dec),
                                  "full_bp_eps_K1": ms(t_dec1)},
            "loop_launches_at_eps0_ms": {"fill_batch": ms(t_fill), "decode_batch": ms(t_decode)},
            "decoder_split_ms": {"stage_0": round(1e3 * float(np.median(t_dec1)), 3),
                                 "stages_1_to_25": round(1e3 * float(np.median(t_dec) - np.median(t_dec1)), 3)},
            "workspace_bytes": E.full_bp_eps_workspace_bytes(p, B, a16),
            "outputs_equal": equal}
        del sim, d_adj, d_ch, d_lev, d_cnt, d_loop
        torch.cuda.empty_cache()
    result = {"what": "26 eps points per batch of 2048 frames: sample_philox + channel_levels + full_bp_eps against the per-eps loop "
                      "of fill_batch + decode_batch that bp_lim_iter --schedule fixpoint runs",
              "config": {"es": [round(e, 5) for e in ES], "batch": B, "reps": opts.reps, "is_term": True, "columns_compared": COLS},
              "shapes": shapes, "outputs_equal": bool(all(s["outputs_equal"] for s in shapes.values())),
              "shapes_where_fused_is_not_faster_in_every_repetition":
                  [n for n, s in shapes.items() if not s["fused_faster_in_every_repetition"]],
              "device": torch.cuda.get_device_name(0)}
    line = json.dumps(result)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0 if result["outputs_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
