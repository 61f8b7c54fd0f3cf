"""What the exact erasure threshold of every frame costs per batch of frames (bp_decoding.run_thresholds' round: sample_philox +
engine.channel_keys + engine.frame_threshold, csrc/frame_threshold.hip) beside the one stand-in a user had before, a bisection
driven from the host:

  * device   one first-generation sampler launch, one keys launch, one decoder launch that decodes at t_hi and bisects inside the
             residual;
  * host     the same sampler and keys launches, then 2 + ceil(log2(t_hi - t_lo)) rounds (about 30): every frame's channel formed
             with torch from the keys and that frame's current threshold (t_hi, t_lo, then its own mid), one
             engine.full_bp_fixpoint (engine.full_bp without a cap where that one does not take the shape) over the batch, and the
             frames' windows halved from its num_erasures.

Both sides work on the same frames, so their answers can be compared: thresh and status of every frame, in every repetition.
The decoder's time stands beside engine.full_bp_eps with one point at eps_hi on the same codes — what stage 0 alone costs — and the
stages per frame (column 5) are recorded.  Shapes: BASELINE config 2's — (4,8), L = 50, N = 1000 — then (3,6) and (5,10) at
N = 1000 and (4,8) at N = 5000, where the CN words live in the workspace; window [0.44, 0.48]; batches of 2048 frames.  Device
events around whole variants, two warm-ups of every variant, --reps alternating repetitions, all values kept; the launches of the
device path are timed in passes of their own.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPS_LO, EPS_HI = 0.44, 0.48
SHAPES = {                                                                # name: (dv, dc, L, N)
    "4-8-N1000": (4, 8, 50, 1000),
    "3-6-N1000": (3, 6, 50, 1000),
    "5-10-N1000": (5, 10, 50, 1000),
    "4-8-N5000": (4, 8, 50, 5000),
}


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
    assert torch.cuda.is_available(), "thresholds_speed measures on the GPU"
    B = opts.batch
    t_lo, t_hi = E.erasure_threshold(EPS_LO), E.erasure_threshold(EPS_HI)
    halvings = int(np.ceil(np.log2(t_hi - t_lo)))

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
        d_adj = torch.empty((B, p.n, p.dv), dtype=torch.int16 if a16 else torch.int32, device="cuda:0")
        d_ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda:0")
        d_keys = torch.empty((B, p.n), dtype=torch.int32, device="cuda:0")
        d_rows = torch.empty((B, 8), dtype=torch.int32, device="cuda:0")
        d_cnt = torch.empty((1, B, 8), dtype=torch.int32, device="cuda:0")
        d_fix = torch.empty((B, 8), dtype=torch.int32, device="cuda:0")
        d_pad = torch.zeros((B, p.nw * 32), dtype=torch.bool, device="cuda:0")
        shifts = torch.arange(32, dtype=torch.int32, device="cuda:0")

        def sample(k):
            key = BP.trial_key(0, 0, k * B)
            E.sample_philox(p, 11, key, B, EPS_HI, (), out=(d_adj, d_ch))
            E.channel_keys(p, 11, key, B, (), out=d_keys)

        def device(k):
            sample(k)
            return E.frame_threshold(p, d_adj, d_keys, t_lo, t_hi, rows=d_rows)["rows"]

        def fails(thr):
            """Which frames fail at their threshold thr [B]: the channel with torch (no key is doped here: all are below 2^31),
            then the fixpoint decoder."""
            d_pad[:, :p.n] = d_keys < thr[:, None]
            words = (d_pad.view(B, p.nw, 32).to(torch.int32) << shifts).sum(dim=-1, dtype=torch.int32)
            if p.dv == 4:
                cnt = E.full_bp_fixpoint(p, d_adj, words, counters=d_fix)["counters"]
            else:
                cnt = E.full_bp(p, d_adj, words, max_it=0, counters=d_fix)["counters"]
            return cnt[:, 0] > 0

        def host(k):
            sample(k)
            lo = torch.full((B,), t_lo, dtype=torch.int32, device="cuda:0")
            hi = torch.full((B,), t_hi, dtype=torch.int32, device="cuda:0")
            top, bottom = fails(hi).clone(), fails(lo).clone()
            for _ in range(halvings):
                mid = lo + (hi - lo) // 2
                f = fails(mid)
                hi = torch.where(f, mid, hi)
                lo = torch.where(f, lo, mid)
            status = torch.where(~top, 1, torch.where(bottom, 2, 0))
            thresh = torch.where(status == 0, hi, torch.where(status == 2, lo * 0 + t_lo, lo * 0 - 1))
            return torch.stack([thresh, status.to(torch.int32)], dim=1)

        variants = {"device": device, "host": host}
        for k in range(2):                                               # warm-up of every variant, in the order of the timed loop
            for fn in variants.values():
                fn(k)
        times = {v: [] for v in variants}
        equal, faster, stages = True, True, []
        for k in range(opts.reps):                                       # alternating: one repetition of every variant in turn
            outs = {}
            for v, fn in variants.items():
                dt, out = event_timed(lambda: fn(k))
                times[v].append(dt)
                outs[v] = out.cpu().numpy().copy()
            equal = equal and bool((outs["device"][:, :2] == outs["host"]).all())
            faster = faster and times["device"][-1] < times["host"][-1]
            stages.append(outs["device"][:, 5])
        status = outs["device"][:, 1]
        # the launches of the device path, each in passes of its own; full_bp_eps with the one point eps_hi on the same codes
        t_sample, t_keys, t_dec, t_stage0 = [], [], [], []
        stage0_agrees = True
        for k in range(opts.reps):
            key = BP.trial_key(0, 0, k * B)
            t_sample.append(event_timed(lambda: E.sample_philox(p, 11, key, B, EPS_HI, (), out=(d_adj, d_ch)))[0])
            t_keys.append(event_timed(lambda: E.channel_keys(p, 11, key, B, (), out=d_keys))[0])
            t_dec.append(event_timed(lambda: E.frame_threshold(p, d_adj, d_keys, t_lo, t_hi, rows=d_rows))[0])
            d_lev1 = E.channel_levels(p, 11, key, B, [EPS_HI])
            t_stage0.append(event_timed(lambda: E.full_bp_eps(p, d_adj, d_lev1, 1, counters=d_cnt))[0])
            r, c = d_rows.cpu().numpy(), d_cnt[0].cpu().numpy()
            stage0_agrees = stage0_agrees and bool(((r[:, 1] != 1) == (c[:, 0] > 0)).all() and (r[:, 7] == c[:, 7]).all())
        med = {v: float(np.median(t)) for v, t in times.items()}
        st = np.concatenate(stages)
        shapes[name] = {
            "shape": {"dv": dv, "dc": dc, "L": L, "N": N, "n": p.n, "ncn": p.nk},
            "host_decoder": "full_bp_fixpoint" if p.dv == 4 else "full_bp(max_it=0)",
            "host_decodes_per_batch": 2 + halvings,
            "status_0_1_2_of_last_batch": [int((status == s).sum()) for s in (0, 1, 2)],
            "stages_per_frame": {"mean": round(float(st.mean()), 2), "max": int(st.max()),
                                 "mean_of_the_frames_that_fail_at_eps_hi": round(float(st[st > 1].mean()), 2) if (st > 1).any() else None},
            "ms_per_batch": {v: ms(t) for v, t in times.items()},
            "host_over_device": round(med["host"] / med["device"], 3),
            "device_faster_in_every_repetition": faster,
            "device_launches_ms": {"sample_philox": ms(t_sample), "channel_keys": ms(t_keys), "frame_threshold": ms(t_dec),
                                   "full_bp_eps_one_point_at_eps_hi": ms(t_stage0)},
            "frame_threshold_over_stage_0": round(float(np.median(t_dec) / np.median(t_stage0)), 3),
            "workspace_bytes": E.frame_threshold_workspace_bytes(p, B, a16),
            "stage_0_agrees_with_full_bp_eps": stage0_agrees,
            "outputs_equal": equal}
        del d_adj, d_ch, d_keys, d_rows, d_cnt, d_fix, d_pad
        torch.cuda.empty_cache()
    result = {"what": "the exact threshold of every frame of a batch of 2048: sample_philox + channel_keys + frame_threshold against a "
                      "bisection driven from the host (a torch-formed channel and one fixpoint decode of the batch per halving)",
              "config": {"eps_lo": EPS_LO, "eps_hi": EPS_HI, "t_lo": t_lo, "t_hi": t_hi, "batch": B, "reps": opts.reps, "is_term": True,
                         "compared": ["thresh", "status"]},
              "shapes": shapes, "outputs_equal": bool(all(s["outputs_equal"] and s["stage_0_agrees_with_full_bp_eps"]
                                                          for s in shapes.values())),
              "shapes_where_the_device_path_is_not_faster_in_every_repetition":
                  [n for n, s in shapes.items() if not s["device_faster_in_every_repetition"]],
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
