"""What the exact Gram pass of simulate_pd_covariance (engine.r1_gram, csrc/r1_gram.hip) costs per batch at BASELINE config 3's
size — (4,8), L = 50, M = 10000, ε = 0.48, non-terminated, the simulator's default batch — for K = 256, 1024 and 4096 evenly
strided steps, beside

  * the sample + decode time of the same batch (sample_philox(adj16) + peel_pick with rows): what the pass is added to, and
  * the only device stand-in that exists without the kernel: gather r1[:, steps], three float64 torch.matmuls, back to int64.
    It is exact at this size, because max(r1)² · batch < 2⁵³ (checked), and at no larger one.

One batch is sampled and decoded (timed --reps times, host clock around work that ends in a device synchronise); its rows stay
on the device.  Per K: both passes are warmed up (three alternations), then timed with device events over --reps repetitions,
ALTERNATING, all values kept, and the two outputs are compared for equality in every repetition.  r1_moments, which runs beside
the Gram pass, is timed the same way.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = (4, 8, 50, 10000, 0.48, False)                                    # BASELINE config 3
KS = (256, 1024, 4096)


def default_batch(PD, l, L, M, num_pd_steps, device):
    """simulate_pd_covariance's own rule (rows wanted)."""
    per_trial = 3 * L * M * l * 4 + 4 * (num_pd_steps + 1)
    return max(64, min(8192, int(min(16e9 + 24e9, 0.6 * PD._free_bytes(device)) // per_trial)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="trials per batch (default: the simulator's rule on this device)")
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD
    assert torch.cuda.is_available(), "cov_speed measures on the GPU"
    l, r, L, M, eps, term = SHAPE
    cpp = int(l / r * M)
    npos = L + l - 1 if term else L
    total_size, nsteps = cpp * npos, int(M * npos * (eps + 0.1))
    p = E.CodeParams(l, r, L, cpp, M)
    B = opts.batch or default_batch(PD, l, L, M, nsteps, "cuda:0")

    def host_timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, res

    def sample_and_decode(k):
        d_adj, d_ch = E.sample_philox(p, 11, k * B, B, eps, [], adj16=True)
        return E.peel_pick(p, d_adj, d_ch, total_size, nsteps, seed=11, trial0=k * B)

    sample_and_decode(0)                                                 # warm-up
    t_sd = []
    for k in range(opts.reps):
        dt, res = host_timed(lambda: sample_and_decode(k))
        t_sd.append(dt)
    d_r1 = res["r1"]
    del res
    ncols = d_r1.shape[1]
    vmax = int(d_r1.max().item())
    assert vmax * vmax * B < 1 << 53, "the float64 stand-in is not exact at this size"

    def ms(ts):
        return {"median": round(1e3 * float(np.median(ts)), 3), "all": [round(1e3 * x, 3) for x in ts]}

    E.r1_moments(d_r1)
    t_mom = [event_timed(lambda: E.r1_moments(d_r1))[0] for _ in range(opts.reps)]

    def stand_in(d_steps):
        x = d_r1[:, d_steps.long()].to(torch.float64)
        m = (x != 0).to(torch.float64)
        return torch.stack([m.T @ m, x.T @ m, x.T @ x]).to(torch.int64)

    per_k = {}
    for K in opts.ks:
        stride = ncols // K
        steps = np.arange(K, dtype=np.int64) * stride
        d_steps = torch.from_numpy(steps.astype(np.int32)).cuda()
        for _ in range(3):                                               # warm-up of both, alternating as the timed loop does
            E.r1_gram(d_r1, d_steps), stand_in(d_steps)
        t_new, t_old, equal = [], [], True
        for _ in range(opts.reps):
            dt, g_new = event_timed(lambda: E.r1_gram(d_r1, d_steps))
            t_new.append(dt)
            dt, g_old = event_timed(lambda: stand_in(d_steps))
            t_old.append(dt)
            equal = equal and bool(torch.equal(g_new, g_old))
            del g_new, g_old
        per_k[str(K)] = {
            "k": K, "stride": int(stride), "trial_splits": E.r1_gram_trial_splits(B, K),
            "workspace_bytes": int(E.lib().scldpc_r1_gram_workspace_bytes(B, K)),
            "ms_per_batch": {"r1_gram": ms(t_new), "fp64_matmul_stand_in": ms(t_old)},
            "r1_gram_over_stand_in": round(float(np.median(t_new) / np.median(t_old)), 3),
            "r1_gram_over_sample_and_decode": round(float(np.median(t_new) / np.median(t_sd)), 5),
            "every_r1_gram_rep_beats_every_stand_in_rep": bool(max(t_new) < min(t_old)),
            "outputs_equal": equal}
    not_faster = sorted((k for k, s in per_k.items() if not s["every_r1_gram_rep_beats_every_stand_in_rep"]), key=int)
    out = {"what": "engine.r1_gram (exact int64 Gram matrices of r1 at K steps) per batch at BASELINE config 3's size, beside sample + "
                   "decode of the same batch and beside gather + three float64 matmuls (exact only while max(r1)^2 * batch < 2^53)",
           "config": {"l": l, "r": r, "L": L, "M": M, "eps": eps, "terminated": term, "steps": nsteps, "ncols": int(ncols), "batch": B,
                      "reps": opts.reps, "max_r1": vmax},
           "ms_per_batch": {"sample_and_decode": ms(t_sd), "r1_moments": ms(t_mom)},
           "k": per_k, "r1_gram_not_faster_on": not_faster,
           "outputs_equal": bool(all(s["outputs_equal"] for s in per_k.values())),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["outputs_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
