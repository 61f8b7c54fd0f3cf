#!/usr/bin/env python3
"""On the GPU box: the first-generation flooding decoders of this tree against a library built from another commit
(csrc/flood_common.h against its parent).  Fresh child processes alternate between the two libraries (SCLDPC_LIB_PATH), REPS a
side; each child times every kernel with device synchronisation around a fixed number of calls and hashes what it returned.

    python tools/ab_flood_common.py --parent-lib /path/to/parent/libscldpc_hip.so [--reps 5] [--bench] > profiles/flood_common_ab.txt

--set eps times the eps-grid decoders instead (csrc/eps_stages.h against its parent): engine.peel_sweep_eps on the nine-point grid
of tools/eps_fused_speed.py and engine.full_bp_eps on the 26-point grid of tools/bp_eps_fused_speed.py, the decoder launch alone on
one sampled code and its levels, written to profiles/eps_walk_ab.txt.

A kernel passes when this tree's median lies inside the range the parent's own repetitions span, or below it."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCHES = (("bench.py --config C2 --flooding --gen1", ["--config", "C2", "--flooding", "--gen1"]),
           ("bench.py --config C2 --gen1", ["--config", "C2", "--gen1"]))


def child(kset):
    import torch
    sys.path.insert(0, ROOT)
    from fl_scaling_sc_ldpc_amd import engine as E
    from fl_scaling_sc_ldpc_amd import peeling_decoding as PD

    def timed(name, calls, fn, outs):
        r = fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls): r = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / calls * 1e3
        h = hashlib.sha1()
        for k in outs(r): h.update(k.cpu().numpy().tobytes())
        print(json.dumps({"kernel": name, "ms": ms, "sha": h.hexdigest()[:12]}), flush=True)

    if kset == "eps":
        grids = (("peel_sweep_eps", [round(0.48 - 0.005 * k, 3) for k in range(9)]),
                 ("full_bp_eps", [0.48 - k * 0.00125 for k in range(26)]))
        for dv, dc, N, T, calls, what in ((4, 8, 1000, 2048, 20, "packed words, dv = 4"), (3, 6, 1000, 2048, 20, "generic dv"),
                                          (4, 8, 5000, 512, 5, "CN words in the workspace")):
            g = PD._Geometry(dv, dc, 50, N, True, True, [])
            p = g.params
            a, _ = E.sample_philox(p, 3, 0, T, 0.48, adj16=True)
            for name, es in grids:
                lev = E.channel_levels(p, 3, 0, T, es)
                if name == "peel_sweep_eps":
                    fn, outs = (lambda: E.peel_sweep_eps(p, a, lev, len(es), g.total_size, g.lost_lo, g.lost_hi)), lambda r: [r["out"]]
                else:
                    fn, outs = (lambda: E.full_bp_eps(p, a, lev, len(es))), lambda r: [r["counters"]]
                timed("%s (%d,%d) L=50 N=%d, %d points from 0.48, %d trials, 2-byte table (%s)" % (name, dv, dc, N, len(es), T, what),
                      calls, fn, outs)
            del a, lev
            torch.cuda.empty_cache()
        return
    T = 2048
    p = E.make_params(4, 8, 50, 1000)
    a, ch = E.sample_philox(p, 3, 0, T, 0.48, adj16=True)
    timed("full_bp (4,8) L=50 N=1000 eps=0.48, 2048 trials, 2-byte table", 20, lambda: E.full_bp(p, a, ch), lambda r: [r["counters"]])
    timed("full_bp_fixpoint (4,8) L=50 N=1000 eps=0.48, 2048 trials, 2-byte table", 20, lambda: E.full_bp_fixpoint(p, a, ch),
          lambda r: [r["counters"][:, [0, 1, 2, 3, 4, 6, 7]]])
    p = E.make_params(4, 8, 50, 5000)
    a, ch = E.sample_philox(p, 3, 0, 512, 0.48, adj16=True)
    timed("full_bp rows_cap=512 (4,8) L=50 N=5000 eps=0.48, 512 trials, 2-byte table", 5, lambda: E.full_bp(p, a, ch, rows_cap=512),
          lambda r: [r["counters"], r["rows"] * (torch.arange(512, device=r["rows"].device)[None, :, None] < r["counters"][:, 5, None, None])])
    p = E.make_params(4, 8, 100, 2000)
    a, ch = E.sample_philox(p, 3, 0, T, 0.47, adj16=True)
    for cl in (False, True):
        timed("sw_bp %s window, whole-chain kernel, L=100 N=2000 W=10 20 iterations, 2048 trials" % ("classical" if cl else "square"), 5,
              lambda: E.sw_bp(p, a, ch, 10, 20, 0, classical=cl, ring=False), lambda r: [r["counters"]])
    del a, ch
    torch.cuda.empty_cache()
    g = PD._Geometry(4, 8, 50, 10000, True, True, [])
    a, ch = E.sample_philox(g.params, 3, 0, T, 0.48, adj16=True)
    timed("peel_sweep L=50 M=10000 eps=0.48, 2048 trials", 3,
          lambda: E.peel_sweep(g.params, a, ch, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi), lambda r: [r["out"][:, [0, 1, 2, 7]]])


def verdict(par, new, lower_is_better=True):
    med = statistics.median(new)
    lo, hi = min(par), max(par)
    ok = med <= hi if lower_is_better else med >= lo
    inside = lo <= med <= hi
    pm = statistics.median(par)
    return "this tree's median %.4g %s the parent's range [%.4g, %.4g] (parent median %.4g, %+.2f %%)" % (
        med, "inside" if inside else ("outside, on the good side of" if ok else "OUTSIDE"), lo, hi, pm, (med / pm - 1) * 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench", action="store_true", help="also bench.py --config C2 [--flooding] --gen1 on both sides")
    ap.add_argument("--set", choices=("flood", "eps"), default="flood", help="which kernels the children time")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.set)
    sides = (("parent", a.parent_lib), ("this", os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "libscldpc_hip.so")))
    runs, order = {}, []
    for rep in range(a.reps):
        for side, lib in sides:
            env = dict(os.environ, SCLDPC_LIB_PATH=lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--set", a.set], env=env, check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            print("repetition %d, %s: done" % (rep + 1, side), file=sys.stderr, flush=True)
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    if r["kernel"] not in runs: order.append(r["kernel"])
                    runs.setdefault(r["kernel"], {"parent": [], "this": [], "sha": set()})
                    runs[r["kernel"]][side].append(r["ms"]); runs[r["kernel"]]["sha"].add(r["sha"])
    print("## ms per call, %d fresh processes a side, alternating parent / this tree" % a.reps)
    for k in order:
        r = runs[k]
        print("%s\n    parent %s | this %s | outputs_equal %s\n    %s" % (
            k, " ".join("%.3f" % x for x in r["parent"]), " ".join("%.3f" % x for x in r["this"]), len(r["sha"]) == 1,
            verdict(r["parent"], r["this"])), flush=True)
    if a.bench:
        for title, args in BENCHES:
            vals = {"parent": [], "this": []}
            print("## python %s --gpus 1 --steps 50 --warmup 5, alternating (trials/s)" % title)
            for rep in range(a.reps):
                for side, lib in sides:
                    env = dict(os.environ, SCLDPC_LIB_PATH=lib)
                    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5"] + args,
                                         env=env, check=True, capture_output=True, text=True, timeout=600, cwd=ROOT).stdout
                    j = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
                    vals[side].append(float(j["value"]))
                    print("%s_%d  %.0f  results %s" % (side, rep + 1, j["value"], json.dumps(j.get("results", ""))), flush=True)
            print(verdict(vals["parent"], vals["this"], lower_is_better=False), flush=True)


if __name__ == "__main__":
    main()
