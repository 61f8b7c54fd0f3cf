"""What `bp_lim_iter --caps` saves at the published configuration: the BP_Full_{175,200,250,300,350}it family on
(4,8, L = 50, N = 1000), a few ε points of the published grid, a fixed number of frames per point and no stop rule.

  (a) five single-cap passes: per cap, sample every batch (sampler_v3, CN -> VN table) and decode it with full_bp_cn16
  (b) one fused pass: sample every batch once and decode it once with full_bp_caps_cn16 (a checkpoint at every cap)
  (c) the CAPS form's own cost: full_bp_caps_cn16 with ONE cap against full_bp_cn16 at that cap, decode only, same batch

Host clock around work that ends in a device synchronise; every shape warmed up first; (a) and (b) alternate over
--reps repetitions and the median is kept (the spread is printed with it).  Prints one JSON line; --out writes it too.
The outputs of (a) and (b) are compared on the way (the run counters of every cap must agree)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--eps", default="0.46,0.47,0.475")
    ap.add_argument("--caps", default="175,200,250,300,350")
    ap.add_argument("--frames", type=int, default=65536, help="frames per ε point")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "caps_speedup measures on the GPU"
    eps_list = [float(x) for x in opts.eps.split(",")]
    caps = tuple(int(x) for x in opts.caps.split(","))
    p = E.make_params(4, 8, 50, 1000)
    B, F = opts.batch, opts.frames
    a = torch.empty((B, p.n, 4), dtype=torch.int16, device="cuda")
    cn = torch.empty((B, p.nk, 8), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, E.NCOUNTERS), dtype=torch.int32, device="cuda")
    cnt_k = torch.empty((len(caps), B, E.NCOUNTERS), dtype=torch.int32, device="cuda")
    one = torch.empty((1, B, E.NCOUNTERS), dtype=torch.int32, device="cuda")

    def single_cap_passes():
        runs = {}
        for cap in caps:
            for i, eps in enumerate(eps_list):
                run = E.new_run("cuda")
                for b0 in range(0, F, B):
                    E.sample_philox_cn16(p, 11, (i << 24) + b0, B, eps, out=(a, cn, ch))
                    E.full_bp_cn16(p, a, cn, ch, max_it=cap, counters=cnt)
                    E.accumulate_run(cnt, run)
                runs[(cap, eps)] = run
        torch.cuda.synchronize()
        return runs

    def fused_pass():
        runs = {}
        for i, eps in enumerate(eps_list):
            rk = [E.new_run("cuda") for _ in caps]
            for b0 in range(0, F, B):
                E.sample_philox_cn16(p, 11, (i << 24) + b0, B, eps, out=(a, cn, ch))
                E.full_bp_caps_cn16(p, a, cn, ch, caps, counters=cnt_k)
                for k in range(len(caps)):
                    E.accumulate_run(cnt_k[k], rk[k])
            for k, cap in enumerate(caps):
                runs[(cap, eps)] = rk[k]
        torch.cuda.synchronize()
        return runs

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    # warm-up of every shape, and the outputs of both ways compared
    ra, rb = single_cap_passes(), fused_pass()
    for key in ra:
        assert (ra[key].cpu().numpy() == rb[key].cpu().numpy()).all(), key
    ta, tb = [], []
    for _ in range(opts.reps):
        ta.append(timed(single_cap_passes)[0])
        tb.append(timed(fused_pass)[0])
    # (c) decode only, one cap, on one sampled batch at the middle ε: alternate the two forms
    E.sample_philox_cn16(p, 12, 0, B, eps_list[len(eps_list) // 2], out=(a, cn, ch))
    overhead = {}
    for cap in (caps[0], caps[-1]):
        E.full_bp_cn16(p, a, cn, ch, max_it=cap, counters=cnt)
        E.full_bp_caps_cn16(p, a, cn, ch, (cap,), counters=one)
        torch.cuda.synchronize()
        assert (one[0] == cnt).all()
        t_single, t_caps = [], []
        for _ in range(max(5, opts.reps)):
            for which, acc in ((0, t_single), (1, t_caps)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(4):
                    if which == 0:
                        E.full_bp_cn16(p, a, cn, ch, max_it=cap, counters=cnt)
                    else:
                        E.full_bp_caps_cn16(p, a, cn, ch, (cap,), counters=one)
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) / 4)
        overhead[str(cap)] = {"full_bp_cn16_ms": round(1e3 * float(np.median(t_single)), 3),
                              "caps_one_cap_ms": round(1e3 * float(np.median(t_caps)), 3),
                              "ratio": round(float(np.median(t_caps) / np.median(t_single)), 4)}
    res = {"what": "bp_lim_iter --caps: five single-cap passes vs one fused pass (sample + decode)",
           "config": {"dv": 4, "dc": 8, "L": 50, "N": 1000, "caps": list(caps), "eps": eps_list, "frames_per_eps": F,
                      "batch": B, "reps": opts.reps, "device": torch.cuda.get_device_name(0)},
           "single_cap_passes_s": round(float(np.median(ta)), 4), "single_cap_passes_s_all": [round(x, 4) for x in ta],
           "fused_pass_s": round(float(np.median(tb)), 4), "fused_pass_s_all": [round(x, 4) for x in tb],
           "speedup": round(float(np.median(ta) / np.median(tb)), 3),
           "one_cap_overhead": overhead, "outputs_equal": True}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
