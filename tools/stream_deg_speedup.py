"""Streaming throughput of the VN degrees 3 and 5 next to (4,8), and what adding them cost (4,8): positions/s of the (3,6),
(4,8) and (5,10) ensembles at the shape of the bench's C5 — N = 5000, L = 50, W = 20, 6144 streams as two halves on two HIP
streams, 16 positions per stream and launch, doping that decouples the chain (dv - 1 consecutive known positions per period),
ε near each pair's waterfall (written into the record).  There is no older streaming path for dv = 3 or 5, so these figures
carry no verdict.

The one comparison with a verdict: `bench.py --config C5` on this build and — with --parent-root, a checkout of the parent
commit with its library built — on the parent, alternating, --reps times each (at least three).  The branch's runs may
not fall below the parent's lowest by more than the parent's own spread (max - min of its repetitions).

Host clock around work that ends in a device synchronise, every ensemble warmed up first, all repetitions kept.  Every
measurement is a child process of its own under a time limit; the first child that fails or runs out of time ends the run
with its exit status (nothing more is started).  Prints one JSON line; --out writes it too."""
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

L_BUF, N_POS, W, NS, CHUNK = 50, 5000, 20, 6144, 16
# name: dv, dc, ε, doped positions
ENSEMBLES = {"3_6": (3, 6, 0.46, (10, 11)), "4_8": (4, 8, 0.485, (10, 11, 12)), "5_10": (5, 10, 0.48, (10, 11, 12, 13))}


def measure(name, reps, steps):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "stream_deg_speedup measures on the GPU"
    dv, dc, eps, doped = ENSEMBLES[name]
    p = E.make_params(dv, dc, L_BUF, N_POS)
    assert E.stream_supported(p, W), "the streaming kernels do not take this configuration"
    dev = torch.device("cuda:0")
    sizes = [NS - NS // 2, NS // 2]
    hip = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]
    sts = [E.Streams(p, sizes[h], seed=11, eps=eps, W=W, doped=doped, stream0=h * sizes[0], device=dev) for h in range(2)]

    def run_all():
        main = torch.cuda.current_stream(dev)
        hip[1].wait_stream(main)
        for h in range(2):
            with torch.cuda.stream(hip[h]):
                sts[h].run(CHUNK)
        main.wait_stream(hip[1])

    for _ in range(4):                                      # warm-up: past the first L/2 positions of a new stream
        run_all()
    torch.cuda.synchronize()
    c0 = [st.counters.clone() for st in sts]
    rates = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            run_all()
        torch.cuda.synchronize()
        rates.append(steps * CHUNK * NS / (time.perf_counter() - t0))
    tot = sum((st.counters - c)[:, :8].sum(dim=0) for st, c in zip(sts, c0)).cpu().numpy()
    unusable = int(sum((st.counters[:, 9] < 0).sum().item() for st in sts))
    return {"dv": dv, "dc": dc, "L": L_BUF, "N": N_POS, "W": W, "eps": eps, "doped": list(doped), "streams": NS,
            "positions_per_launch": CHUNK, "steps_per_rep": steps, "state_bytes_per_stream": int(sts[0].state.shape[1]),
            "positions_per_s": {"median": round(float(np.median(rates)), 1), "min": round(min(rates), 1),
                                "max": round(max(rates), 1), "all": [round(x, 1) for x in rates]},
            "bler_exp": float(tot[3] / max(1, tot[7])), "blocks_exp": int(tot[7]), "unusable_streams": unusable,
            "device": torch.cuda.get_device_name(0)}


def child(cmd, limit, cwd=ROOT):
    """stdout of a child process that has `limit` seconds, or its exit status (124: out of time) as an int."""
    env = dict(os.environ)
    env.pop("SCLDPC_LIB_PATH", None)                        # each tree loads its own library
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit, env=env, cwd=cwd)
    except subprocess.TimeoutExpired:
        return 124
    return r.stdout.decode() if r.returncode == 0 else (r.returncode or 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launch pairs per timed repetition")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit, library built: runs the C5 comparison")
    ap.add_argument("--one", choices=sorted(ENSEMBLES), default=None, help="measure this ensemble in this process (the children's mode)")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 3:
        ap.error("--reps must be at least 3")
    if opts.one:
        print(json.dumps(measure(opts.one, opts.reps, opts.steps)), flush=True)
        return 0
    res = {"what": "streaming (stream_gen_kernel + stream_dec_kernel) at C5's shape for the pairs (3,6), (4,8), (5,10); "
                   "bench C5 on a checkout of the parent commit and on this build",
           "config": {"L": L_BUF, "N": N_POS, "W": W, "streams": NS, "reps": opts.reps}, "ensembles": {}}
    for name in ENSEMBLES:
        out = child([sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(opts.reps), "--steps",
                     str(opts.steps)], opts.limit)
        if isinstance(out, int):
            print("stream_deg_speedup: %s ended with status %d; nothing more is started" % (name, out), file=sys.stderr)
            return out
        res["ensembles"][name] = json.loads(out.strip().split("\n")[-1])
    if opts.parent_root:
        runs = {"parent": [], "branch": []}
        for _ in range(opts.reps):
            for who in ("parent", "branch"):
                root = os.path.abspath(opts.parent_root) if who == "parent" else ROOT
                out = child([sys.executable, os.path.join(root, "bench.py"), "--config", "C5", "--gpus", "1"], opts.limit, root)
                if isinstance(out, int):
                    print("stream_deg_speedup: bench C5 (%s) ended with status %d; nothing more is started" % (who, out),
                          file=sys.stderr)
                    return out
                runs[who].append(float(json.loads(out.strip().split("\n")[-1])["value"]))
        spread = max(runs["parent"]) - min(runs["parent"])
        res["bench_C5"] = {"unit": "positions/s", "order": "parent, branch, parent, branch, …", "parent": runs["parent"],
                           "branch": runs["branch"], "parent_spread": spread,
                           "rule": "min(branch) >= min(parent) - (max(parent) - min(parent))",
                           "branch_not_slower": bool(min(runs["branch"]) >= min(runs["parent"]) - spread)}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0 if res.get("bench_C5", {}).get("branch_not_slower", True) else 1


if __name__ == "__main__":
    sys.exit(main())
