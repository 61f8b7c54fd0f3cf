"""What the wide 4-bit level decoder saves bp_traj at its shipped size: (4,8), L = 50, N = 5000 (132 500 CNs per trial),
batches of 2048 frames with trajectory rows, in the two configurations users run — ε = 0.46 truncated with MAX_IT = 500 (the
published L50_M2500 files) and ε = 0.46 terminated, unlimited (the CLI default).

  old path: sample_philox(adj16) + full_bp(rows_cap)                         (first generation, 16-bit CN words)
  new path: sample_philox(adj16) + cn_sockets + full_bp_wide(rows_cap)       (4-bit counts, 32-bit queue entries)

Host clock around work that ends in a device synchronise; every shape warmed up first; the two paths ALTERNATE over --reps
repetitions, the median is kept and all values are printed.  The three stages of the new path and the old decoder are also
timed alone, so that the record shows where the time goes.  Counters and rows of the two paths are compared on the way
(outputs_equal).  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = (("eps0.46_truncated_500it", 0.46, False, 500, 500),
           ("eps0.46_terminated_unlimited", 0.46, True, 0, 4096))      # name, ε, is_term, max_it, rows_cap (the CLI's 4096)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--N", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=32768, help="frames per timed pass (the slower path should run >= 0.5 s)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "traj_wide_speedup measures on the GPU"
    p = E.make_params(4, 8, opts.L, opts.N)
    assert E.full_bp_wide_supported(p), "the wide form does not take this ensemble"
    B, F = opts.batch, opts.frames
    a = torch.empty((B, p.n, 4), dtype=torch.int16, device="cuda")
    cs = torch.empty((B, p.nk, 8), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, E.NCOUNTERS), dtype=torch.int32, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def stats(ts, frames):
        med = float(np.median(ts))
        return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                "spread_s": round(max(ts) - min(ts), 4), "all_s": [round(x, 4) for x in ts],
                "trials_per_s": round(frames / med, 1)}

    out = {}
    for name, eps, is_term, max_it, rows_cap in CONFIGS:
        def old_path():
            for b0 in range(0, F, B):
                E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
                E.full_bp(p, a, ch, max_it=max_it, is_term=is_term, rows_cap=rows_cap, counters=cnt)

        def new_path():
            for b0 in range(0, F, B):
                E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
                E.cn_sockets(p, a, out=cs)
                E.full_bp_wide(p, a, cs, ch, max_it=max_it, is_term=is_term, rows_cap=rows_cap, counters=cnt)

        # warm-up of every shape and the outputs of the two paths compared (one batch)
        E.sample_philox(p, 11, 0, B, eps, out=(a, ch))
        E.cn_sockets(p, a, out=cs)
        ro = E.full_bp(p, a, ch, max_it=max_it, is_term=is_term, rows_cap=rows_cap)
        rn = E.full_bp_wide(p, a, cs, ch, max_it=max_it, is_term=is_term, rows_cap=rows_cap)
        torch.cuda.synchronize()
        live = (torch.arange(rows_cap, device="cuda")[None, :] < ro["counters"][:, 5:6])[:, :, None]
        equal = bool(torch.equal(ro["counters"], rn["counters"]) and torch.equal(ro["rows"] * live, rn["rows"] * live))
        iters = float(ro["counters"][:, 5].double().mean().item())
        del ro, rn, live
        t_old, t_new = [], []
        for _ in range(opts.reps):
            t_old.append(timed(old_path))
            t_new.append(timed(new_path))
        # the stages alone, on one sampled batch (alternating)
        nrep = max(2, F // B // 2)
        stage = {"sampler": [], "cn_sockets": [], "full_bp_wide": [], "full_bp": []}
        for _ in range(opts.reps):
            stage["sampler"].append(timed(lambda: [E.sample_philox(p, 11, 0, B, eps, out=(a, ch)) for _ in range(nrep)]) / nrep)
            stage["cn_sockets"].append(timed(lambda: [E.cn_sockets(p, a, out=cs) for _ in range(nrep)]) / nrep)
            stage["full_bp_wide"].append(timed(lambda: [E.full_bp_wide(p, a, cs, ch, max_it=max_it, is_term=is_term, rows_cap=rows_cap,
                                                                       counters=cnt) for _ in range(nrep)]) / nrep)
            stage["full_bp"].append(timed(lambda: [E.full_bp(p, a, ch, max_it=max_it, is_term=is_term, rows_cap=rows_cap,
                                                             counters=cnt) for _ in range(nrep)]) / nrep)
        so, sn = stats(t_old, F), stats(t_new, F)
        gain = so["median_s"] - sn["median_s"]
        out[name] = {"eps": eps, "is_term": is_term, "max_it": max_it, "rows_cap": rows_cap, "mean_iterations": round(iters, 1),
                     "old_path": so, "new_path": sn, "speedup_end_to_end": round(so["median_s"] / sn["median_s"], 3),
                     "stages_ms_per_batch": {k: {"median": round(1e3 * float(np.median(v)), 3),
                                                 "all": [round(1e3 * x, 3) for x in v]} for k, v in stage.items()},
                     "speedup_decoder_only": round(float(np.median(stage["full_bp"]) / np.median(stage["full_bp_wide"])), 3),
                     "new_beats_old_by_more_than_either_spread": bool(gain > max(so["spread_s"], sn["spread_s"])),
                     "outputs_equal": equal}
    res = {"what": "bp_traj at N = 5000: first-generation path vs cn_sockets + wide 4-bit level decoder (sample + decode, rows)",
           "config": {"dv": 4, "dc": 8, "L": opts.L, "N": opts.N, "batch": B, "frames_per_pass": F, "reps": opts.reps,
                      "device": torch.cuda.get_device_name(0)},
           "configurations": out,
           "wide_becomes_default": bool(all(c["new_beats_old_by_more_than_either_spread"] and c["outputs_equal"]
                                            for c in out.values()))}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
