"""What a whole eps grid from one sampled code costs per batch (simulate_sc_ldpc_curve: sample_philox + engine.channel_levels +
engine.peel_sweep_eps, csrc/peel_sweep_eps.hip) beside the loop it replaces, one sample_philox + one sweep decode per eps:

  * fused        one sampler launch at max(es), one levels launch, one decoder launch that walks the nine points;
  * loop_first   for every eps: sample_philox + peel_sweep (sweep="first": what ber_sim --rng philox runs today);
  * loop_small / loop_wide   the same loop on the 4-bit sweep decoder where select_sweep takes the shape (sweep="small" /
                 "wide", local tables for the tail-biting chain): the fastest path a user has today.

Shapes: BASELINE config 1's — (4,8), L = 50, M = 1000, terminated, bounded — then (3,6) and (5,10) at M = 1000, (4,8) at M = 5000
and the tail-biting (4,8) at M = 1000; es = 0.48, 0.475, ..., 0.44 (nine points); batches of 2048 trials (no stop rule: every
point sees every trial).  Device events around whole variants, two warm-ups of every variant, --reps alternating repetitions, all
values kept, columns 0, 1, 2, 7 of every point compared between the variants in every repetition.  The per-launch times of the
fused path are taken in passes of their own, and the decoder's split between stage 0 and the later stages from K = 1 against
K = 9 (no timers inside the kernel).  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ES = [round(0.48 - 0.005 * i, 3) for i in range(9)]
SHAPES = {                                                                # name: (l, r, L, M, ensemble)
    "4-8-M1000": (4, 8, 50, 1000, "olmos"),
    "3-6-M1000": (3, 6, 50, 1000, "olmos"),
    "5-10-M1000": (5, 10, 50, 1000, "olmos"),
    "4-8-M5000": (4, 8, 50, 5000, "olmos"),
    "4-8-M1000-tb": (4, 8, 50, 1000, "tail_biting"),
}
COLS = [0, 1, 2, 7]


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
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "eps_fused_speed measures on the GPU"
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
        l, r, L, M, ens = SHAPES[name]
        g = PD._Geometry(l, r, L, M, True, True, [])
        p = g.params
        a16 = ens == "olmos"
        geo = (g.total_size, 0, g.lost_lo, g.lost_hi)

        def fused(k, es=ES):
            d_adj, _ = E.sample_philox(p, 11, k * B, B, max(es), [], adj16=a16, ensemble=ens)
            d_lev = E.channel_levels(p, 11, k * B, B, es)
            return E.peel_sweep_eps(p, d_adj, d_lev, len(es), g.total_size, g.lost_lo, g.lost_hi)["out"]

        def loop_first(k):
            outs = []
            for e in ES:
                d_adj, d_ch = E.sample_philox(p, 11, k * B, B, e, [], adj16=a16, ensemble=ens)
                outs.append(E.peel_sweep(p, d_adj, d_ch, *geo)["out"])
            return torch.stack(outs)

        variants = {"fused": fused, "loop_first": loop_first}
        not_applicable = {}
        for form in ("small", "wide"):
            try:
                kind, sampler = PD._sweep_choice(p, "philox", ens, form, True if ens != "olmos" else None)
            except ValueError as err:
                not_applicable["loop_" + form] = str(err)
                continue
            dec = E.peel_sweep_sock16 if kind == "small" else E.peel_sweep_sock16_wide
            ens_kw = {"ensemble": ens} if sampler == "sample_philox_ens_sock16" else {}

            def loop_4bit(k, dec=dec, sampler=sampler, ens_kw=ens_kw):
                outs = []
                for e in ES:
                    d_adj, d_cn, d_ch = PD._sample_small(sampler, p, 11, k * B, B, e, [], "cuda:0", ens)
                    outs.append(dec(p, d_adj, d_cn, d_ch, *geo, **ens_kw)["out"])
                return torch.stack(outs)
            variants["loop_" + form] = loop_4bit

        for v in [v for v in variants if v not in ("fused", "loop_first")]:      # a 4-bit decoder may still refuse the geometry
            try:
                variants[v](0)
            except (E.ScldpcError, ValueError) as err:
                not_applicable[v] = str(err)
                del variants[v]
        for k in range(2):                                               # warm-up of every variant, in the order of the timed loop
            for fn in variants.values():
                fn(k)
            fused(k, ES[:1])
        times = {v: [] for v in variants}
        equal, faster = True, {v: True for v in variants if v != "fused"}
        for k in range(opts.reps):                                       # alternating: one repetition of every variant in turn
            outs = {}
            for v, fn in variants.items():
                dt, out = event_timed(lambda: fn(k))
                times[v].append(dt)
                outs[v] = out[:, :, COLS].cpu().numpy()
            for v in faster:
                equal = equal and bool((outs[v] == outs["fused"]).all())
                faster[v] = faster[v] and times["fused"][-1] < times[v][-1]
        failing = (outs["fused"][:, :, 0] > 0).sum(axis=1).tolist()
        # the launches of the fused path, each in passes of its own; the decoder at K = 1 for the split
        t_sample, t_levels, t_dec, t_dec1, t_first_dec = [], [], [], [], []
        for k in range(opts.reps):
            dt, (d_adj, d_ch) = event_timed(lambda: E.sample_philox(p, 11, k * B, B, ES[0], [], adj16=a16, ensemble=ens))
            t_sample.append(dt)
            dt, d_lev = event_timed(lambda: E.channel_levels(p, 11, k * B, B, ES))
            t_levels.append(dt)
            dt, _ = event_timed(lambda: E.peel_sweep_eps(p, d_adj, d_lev, K, g.total_size, g.lost_lo, g.lost_hi))
            t_dec.append(dt)
            d_lev1 = E.channel_levels(p, 11, k * B, B, ES[:1])
            dt, _ = event_timed(lambda: E.peel_sweep_eps(p, d_adj, d_lev1, 1, g.total_size, g.lost_lo, g.lost_hi))
            t_dec1.append(dt)
            dt, _ = event_timed(lambda: E.peel_sweep(p, d_adj, d_ch, *geo))
            t_first_dec.append(dt)
        med = {v: float(np.median(t)) for v, t in times.items()}
        shapes[name] = {
            "shape": {"l": l, "r": r, "L": L, "M": M, "ensemble": ens, "n": p.n, "ncn": p.nk},
            "failing_trials_per_point_of_last_batch": failing,
            "ms_per_batch": {v: ms(t) for v, t in times.items()},
            "not_applicable": not_applicable,
            "loop_over_fused": {v: round(med[v] / med["fused"], 3) for v in med if v != "fused"},
            "fused_faster_in_every_repetition": faster,
            "fused_launches_ms": {"sample_philox": ms(t_sample), "channel_levels": ms(t_levels), "peel_sweep_eps_K9": ms(t_dec),
                                  "peel_sweep_eps_K1": ms(t_dec1), "peel_sweep_at_eps0_for_comparison": ms(t_first_dec)},
            "decoder_split_ms": {"stage_0": round(1e3 * float(np.median(t_dec1)), 3),
                                 "stages_1_to_8": round(1e3 * float(np.median(t_dec) - np.median(t_dec1)), 3)},
            "workspace_bytes": E.peel_sweep_eps_workspace_bytes(p, B, a16),
            "outputs_equal": equal}
    result = {"what": "nine eps points per batch of 2048 trials: sample_philox + channel_levels + peel_sweep_eps against the per-eps "
                      "loops of sample + sweep decode it replaces",
              "config": {"es": ES, "batch": B, "reps": opts.reps, "terminated": True, "bounded": True, "columns_compared": COLS},
              "shapes": shapes, "outputs_equal": bool(all(s["outputs_equal"] for s in shapes.values())),
              "shapes_where_fused_is_not_faster_than_the_fastest_loop_in_every_repetition":
                  [n for n, s in shapes.items() if not all(s["fused_faster_in_every_repetition"].values())],
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
