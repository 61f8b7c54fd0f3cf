"""What the exact erasure thresholds of every VN and position cost per batch of frames (engine.vn_threshold,
csrc/vn_threshold.hip: the decode at t_hi, then one walk down the keys of its residual), with and without d_tau and a 64-point
grid of counts, beside what a user had before on the same frames:

  (a) engine.frame_threshold: T* of every frame only, by bisection with a rebuild of the CN words per stage — is the walk the
      cheaper way to T*?
  (b) engine.full_bp_eps with 64 points over the window: the only curve of BER and block error rate there was, exact at its
      points and silent between them;
  (c) a STAND-IN for exact per-position thresholds, which nothing computed before: engine.full_bp_eps repeated over
      ceil(log2(t_hi - t_lo) / 6) nested 64-point grids, each a sixty-fourth of the one before.  That is what refining ONE
      position's bracket of ONE frame down to an integer costs for the whole batch; it does not give the thresholds of the
      other positions or frames, whose brackets lie elsewhere, so it is a lower bound of such a search and not an equivalent.

Every variant decodes the same codes and keys (sampled outside the timed region); the levels of (b) and (c) are made outside
it too.  Compared in every repetition: thresh, status and the critical size with (a); the counts with (b)'s num_erasures and
the positions below each point with its num_blocks_err, point for point; the two vn_threshold variants with each other.
engine.full_bp_eps with the one point eps_hi stands for stage 0.  Shapes: those of profiles/thresholds_speed.json, window
[0.44, 0.48]; at N = 5000 no frame fails there (that file), so its window is [0.47, 0.49].  Device events around whole variants,
two warm-ups of every variant, --reps alternating repetitions, all values kept.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {                                                                # name: (dv, dc, L, N, eps_lo, eps_hi)
    "4-8-N1000": (4, 8, 50, 1000, 0.44, 0.48),
    "3-6-N1000": (3, 6, 50, 1000, 0.44, 0.48),
    "5-10-N1000": (5, 10, 50, 1000, 0.44, 0.48),
    "4-8-N5000": (4, 8, 50, 5000, 0.47, 0.49),
}
K = 64


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
    from fl_scaling_sc_ldpc_amd.peeling_decoding import curve_stages
    assert torch.cuda.is_available(), "vn_thresholds_speed measures on the GPU"
    B = opts.batch

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
        dv, dc, L, N, eps_lo, eps_hi = SHAPES[name]
        p = E.make_params(dv, dc, L, N)
        a16 = p.cns_pos <= 65536
        t_lo, t_hi = E.erasure_threshold(eps_lo), E.erasure_threshold(eps_hi)
        es = [float(e) for e in np.linspace(eps_hi, eps_lo, K)]          # descending, for the levels
        grid = [E.erasure_threshold(e) for e in es][::-1]
        assert len(set(grid)) == K and grid[0] == t_lo and grid[-1] == t_hi
        nests = int(np.ceil(np.log2(t_hi - t_lo) / 6.0))
        nested, lo, hi = [], eps_lo, eps_hi
        for _ in range(nests):                                           # the middle sixty-fourth of the bracket, again and again
            nested.append(curve_stages(np.linspace(hi, lo, K))[0])      # (descending, one ε per distinct threshold)
            mid, w = (lo + hi) / 2, (hi - lo) / 64
            lo, hi = mid - w / 2, mid + w / 2
        d_adj = torch.empty((B, p.n, p.dv), dtype=torch.int16 if a16 else torch.int32, device="cuda:0")
        d_ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda:0")
        d_keys = torch.empty((B, p.n), dtype=torch.int32, device="cuda:0")
        d_cnt = torch.empty((K, B, 8), dtype=torch.int32, device="cuda:0")
        d_lev = torch.empty((B, p.n), dtype=torch.uint8, device="cuda:0")
        d_nest = [torch.empty((B, p.n), dtype=torch.uint8, device="cuda:0") for _ in nested]

        def sample(k):
            key = BP.trial_key(0, 0, k * B)
            E.sample_philox(p, 11, key, B, eps_hi, (), out=(d_adj, d_ch))
            E.channel_keys(p, 11, key, B, (), out=d_keys)
            E.channel_levels(p, 11, key, B, es, out=d_lev)
            for lev, pts in zip(d_nest, nested):
                E.channel_levels(p, 11, key, B, pts, out=lev)

        variants = {
            "vn_threshold": lambda: E.vn_threshold(p, d_adj, d_keys, t_lo, t_hi, grid=grid),
            "vn_threshold_tau": lambda: E.vn_threshold(p, d_adj, d_keys, t_lo, t_hi, grid=grid, want_tau=True),
            "frame_threshold": lambda: E.frame_threshold(p, d_adj, d_keys, t_lo, t_hi),
            "full_bp_eps_64": lambda: E.full_bp_eps(p, d_adj, d_lev, K, counters=d_cnt),
            "full_bp_eps_nested": lambda: [E.full_bp_eps(p, d_adj, lev, len(pts)) for lev, pts in zip(d_nest, nested)][-1],
            "full_bp_eps_stage_0": lambda: E.full_bp_eps(p, d_adj, d_lev, 1),
        }
        for k in range(2):                                               # warm-up of every variant, in the order of the timed loop
            sample(k)
            for fn in variants.values():
                fn()
        times = {v: [] for v in variants}
        equal, steps = True, []
        for k in range(opts.reps):                                       # alternating: one repetition of every variant in turn
            sample(k)
            torch.cuda.synchronize()
            outs = {}
            for v, fn in variants.items():
                dt, out = event_timed(fn)
                times[v].append(dt)
                outs[v] = {a: (b.cpu().numpy().copy() if b is not None else None) for a, b in out.items()}
            vn, vt, ft, ge = outs["vn_threshold"], outs["vn_threshold_tau"], outs["frame_threshold"], outs["full_bp_eps_64"]
            pos = vn["pos_thresh"].view(np.uint32).astype(np.int64)
            equal = equal and bool((vn["rows"][:, :2] == ft["rows"][:, :2]).all() and (vn["rows"][:, 3] == ft["rows"][:, 2]).all())
            equal = equal and bool((vn["counts"][:, ::-1].T == ge["counters"][:, :, 0]).all())
            equal = equal and all(bool(((pos <= g).sum(axis=1) == ge["counters"][K - 1 - i, :, 1]).all()) for i, g in enumerate(grid))
            equal = equal and bool((vn["rows"][:, [0, 1, 2, 3, 4, 7]] == vt["rows"][:, [0, 1, 2, 3, 4, 7]]).all())
            equal = equal and bool((vn["pos_thresh"] == vt["pos_thresh"]).all() and (vn["counts"] == vt["counts"]).all())
            tau = vt["tau"].view(np.uint32)
            equal = equal and bool(((tau <= np.uint32(t_hi)).sum(axis=1) == vn["rows"][:, 2]).all())
            steps.append(vn["rows"][:, 4])
        rows = outs["vn_threshold"]["rows"]
        status = rows[:, 1]
        med = {v: float(np.median(t)) for v, t in times.items()}
        st = np.concatenate(steps)
        shapes[name] = {
            "shape": {"dv": dv, "dc": dc, "L": L, "N": N, "n": p.n, "ncn": p.nk},
            "window": {"eps_lo": eps_lo, "eps_hi": eps_hi, "t_lo": t_lo, "t_hi": t_hi},
            "status_0_1_2_of_last_batch": [int((status == s).sum()) for s in (0, 1, 2)],
            "steps_per_frame": {"mean": round(float(st.mean()), 1), "max": int(st.max()),
                                "mean_of_the_frames_that_fail_at_eps_hi": round(float(st[st > 0].mean()), 1) if (st > 0).any() else None},
            "scans_per_frame_mean": round(float(rows[:, 5].mean()), 2), "rescans_of_last_batch": int(rows[:, 6].sum()),
            "nested_refinements": nests,
            "ms_per_batch": {v: ms(t) for v, t in times.items()},
            "vn_threshold_over_frame_threshold": round(med["vn_threshold"] / med["frame_threshold"], 3),
            "vn_threshold_over_full_bp_eps_64": round(med["vn_threshold"] / med["full_bp_eps_64"], 3),
            "vn_threshold_over_nested_stand_in": round(med["vn_threshold"] / med["full_bp_eps_nested"], 3),
            "tau_over_no_tau": round(med["vn_threshold_tau"] / med["vn_threshold"], 3),
            "share_of_stage_0": round(med["full_bp_eps_stage_0"] / med["vn_threshold"], 3),
            "faster_than_frame_threshold_in_every_repetition":
                all(a < b for a, b in zip(times["vn_threshold"], times["frame_threshold"])),
            "faster_than_full_bp_eps_64_in_every_repetition":
                all(a < b for a, b in zip(times["vn_threshold"], times["full_bp_eps_64"])),
            "workspace_bytes": E.vn_threshold_workspace_bytes(p, B, a16),
            "outputs_equal": equal}
        print("[vn_thresholds_speed] %s: %s" % (name, json.dumps(shapes[name]["ms_per_batch"])), file=sys.stderr, flush=True)
        del d_adj, d_ch, d_keys, d_cnt, d_lev, d_nest
        torch.cuda.empty_cache()
    result = {"what": "tau of every VN and position of a batch of frames by engine.vn_threshold (with a 64-point grid of counts, with and "
                      "without d_tau) against frame_threshold (T* only), full_bp_eps at 64 points, and nested 64-point refinements of "
                      "full_bp_eps as a stand-in for a per-position search; kernels only, on the same codes and keys",
              "config": {"batch": B, "reps": opts.reps, "grid_points": K, "is_term": True},
              "shapes": shapes, "outputs_equal": bool(all(s["outputs_equal"] for s in shapes.values())),
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
