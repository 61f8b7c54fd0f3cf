"""What the CN -> socket table costs when the first-generation sampler writes it in its own launch instead of a pass after it:
the shapes the drivers run on that path, in batches of 2048 frames.

  old path: sample_philox(adj16) + cn_sockets [+ decoder]      (the (4,8) square ring: the pass runs inside sw_bp)
  new path: sample_philox_sock [+ decoder]                     (engine.sample_philox_sock, the table from the sampler's launch)

Both are timed alone (sampling, table included) and end to end with the decoder that consumes the table.  Host clock around work
that ends in a device synchronise; every shape warmed up first; the two paths ALTERNATE over --reps repetitions and all values
are kept.  The rows, the channel words and (as a set per CN) the table of the two paths are compared on the way, and so are the
decoder's counters (outputs_equal).

Each shape is measured by a child process of its own under a time limit; the first child that fails or runs out of time ends
the run with its exit status (nothing more is started).  Prints one JSON line; --out writes it too.  sampled_table_becomes_default
is the rule of bp_decoding.SAMPLED_TABLE_BY_DEFAULT: on every shape every repetition of the new path is faster end to end than
every repetition of the old one, with equal outputs."""
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

# name: dv, dc, L, N, decoder, its arguments, ε, frames per timed pass
SHAPES = {
    "4_8_L50_N5000_bp_traj_truncated_500it_rows": (4, 8, 50, 5000, "wide", dict(max_it=500, is_term=False, rows_cap=500), 0.47, 8192),
    "4_8_L100_N2500_sw_W10_20it": (4, 8, 100, 2500, "sw_ring", dict(W=10, max_it=20), 0.47, 8192),
    "3_6_L50_N1000_bp_lim_iter_500it": (3, 6, 50, 1000, "deg", dict(max_it=500), 0.46, 65536),
    "5_10_L50_N1000_bp_lim_iter_500it": (5, 10, 50, 1000, "deg", dict(max_it=500), 0.47, 65536),
    "3_6_L50_N5000_bp_traj_truncated_500it_rows": (3, 6, 50, 5000, "degwide", dict(max_it=500, is_term=False, rows_cap=500), 0.47, 8192),
    "5_10_L50_N5000_bp_traj_truncated_500it_rows": (5, 10, 50, 5000, "degwide", dict(max_it=500, is_term=False, rows_cap=500), 0.48, 8192),
    "3_6_L100_N2000_sw_W10_20it": (3, 6, 100, 2000, "sw_ring_deg", dict(W=10, max_it=20), 0.46, 8192),
}
BATCH = 2048


def measure(name, reps):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "sampled_table_speedup measures on the GPU"
    dv, dc, L, N, decoder, kw, eps, F = SHAPES[name]
    p = E.make_params(dv, dc, L, N)
    assert E.sample_philox_sock_supported(p), "the sampler does not write the table of this ensemble"
    B = BATCH
    a = torch.empty((B, p.n, dv), dtype=torch.int16, device="cuda")
    cs = torch.empty((B, p.nk, dc), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, E.NCOUNTERS), dtype=torch.int32, device="cuda")

    def decode(table):
        """The driver's decoder call; table None: the (4,8) square ring as it runs today (sw_bp builds the table)."""
        if decoder == "wide":
            return E.full_bp_wide(p, a, table, ch, counters=cnt, **kw)
        if decoder in ("deg", "degwide"):
            return E.full_bp_deg(p, a, table, ch, counters=cnt, wide=decoder == "degwide", **kw)
        deg = decoder == "sw_ring_deg"
        return E.sw_bp(p, a, ch, kw["W"], kw["max_it"], counters=cnt, ring=True, deg=deg, d_cn_sock=table)

    in_sw_bp = decoder == "sw_ring"                          # today the pass runs inside sw_bp on every call

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def stats(ts, frames):
        med = float(np.median(ts))
        return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                "all_s": [round(x, 4) for x in ts], "trials_per_s": round(frames / med, 1)}

    def old_sample(b0):
        E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
        E.cn_sockets(p, a, out=cs)

    def new_sample(b0):
        E.sample_philox_sock(p, 11, b0, B, eps, out=(a, cs, ch))

    def old_path():
        for b0 in range(0, F, B):
            if in_sw_bp:
                E.sample_philox(p, 11, b0, B, eps, out=(a, ch))
                decode(None)
            else:
                old_sample(b0)
                decode(cs)

    def new_path():
        for b0 in range(0, F, B):
            new_sample(b0)
            decode(cs)

    # warm-up of every kernel, and the outputs of the two paths compared (one batch)
    old_sample(0)
    ro = decode(None if in_sw_bp else cs)
    torch.cuda.synchronize()
    def table_sets():
        """The tables of the first 64 trials with every CN's entries in ascending order (uint16 values)."""
        u8 = cs[:64].view(torch.uint8).view(64, p.nk, dc, 2)
        return torch.sort(u8[..., 1].int() * 256 + u8[..., 0].int(), dim=-1)[0]

    ref = [x.clone() for x in (a, ch, ro["counters"])] + [table_sets()]
    rows_ref = ro["rows"].clone() if ro.get("rows") is not None else None
    new_sample(0)
    rn = decode(cs)
    torch.cuda.synchronize()
    tab = table_sets()
    equal = bool(torch.equal(a, ref[0]) and torch.equal(ch, ref[1]) and torch.equal(rn["counters"], ref[2])
                 and torch.equal(tab, ref[3]))
    if rows_ref is not None:
        live = (torch.arange(rows_ref.shape[1], device="cuda")[None, :] < ref[2][:, 5:6])[:, :, None]
        equal = equal and bool(torch.equal(rows_ref * live, rn["rows"] * live))
        del live
    del tab
    iters = float(ref[2][:, 5].double().mean().item())
    del ref, rows_ref, ro, rn
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(timed(old_path))
        t_new.append(timed(new_path))
    nrep = max(2, F // B)
    stage = {"sample_philox": [], "cn_sockets": [], "sample_philox+cn_sockets": [], "sample_philox_sock": [], "decoder": []}
    for _ in range(reps):
        stage["sample_philox+cn_sockets"].append(timed(lambda: [old_sample(0) for _ in range(nrep)]) / nrep)
        stage["sample_philox_sock"].append(timed(lambda: [new_sample(0) for _ in range(nrep)]) / nrep)
        stage["sample_philox"].append(timed(lambda: [E.sample_philox(p, 11, 0, B, eps, out=(a, ch)) for _ in range(nrep)]) / nrep)
        stage["cn_sockets"].append(timed(lambda: [E.cn_sockets(p, a, out=cs) for _ in range(nrep)]) / nrep)
        stage["decoder"].append(timed(lambda: [decode(cs) for _ in range(nrep)]) / nrep)
    so, sn = stats(t_old, F), stats(t_new, F)
    med = {k: float(np.median(v)) for k, v in stage.items()}
    return {"dv": dv, "dc": dc, "L": L, "N": N, "sockets_per_position": p.cns_pos * dc, "eps": eps, "decoder": decoder,
            "decoder_args": kw, "table_pass_today": "inside sw_bp" if in_sw_bp else "after the sampler", "batch": B,
            "frames_per_pass": F, "mean_iterations": round(iters, 1), "old_path": so, "new_path": sn,
            "speedup_end_to_end": round(so["median_s"] / sn["median_s"], 3),
            "stages_ms_per_batch": {k: {"median": round(1e3 * med[k], 3), "all": [round(1e3 * x, 3) for x in v]}
                                    for k, v in stage.items()},
            "speedup_sampling_with_table": round(med["sample_philox+cn_sockets"] / med["sample_philox_sock"], 3),
            "table_cost_ms_per_batch": {"pass": round(1e3 * med["cn_sockets"], 3),
                                        "in_the_sampler": round(1e3 * (med["sample_philox_sock"] - med["sample_philox"]), 3)},
            "every_new_rep_beats_every_old_rep": bool(max(t_new) < min(t_old)), "outputs_equal": equal,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150, help="seconds a shape's child process may take")
    ap.add_argument("--one", choices=sorted(SHAPES), default=None, help="measure this shape in this process (the children's mode)")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    if opts.one:
        print(json.dumps(measure(opts.one, opts.reps)), flush=True)
        return 0
    shapes = {}
    for name in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(opts.reps)],
                               stdout=subprocess.PIPE, timeout=opts.limit)
        except subprocess.TimeoutExpired:
            print("sampled_table_speedup: %s ran out of its %d s; nothing more is started" % (name, opts.limit), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("sampled_table_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
        print("sampled_table_speedup: %s done" % name, file=sys.stderr, flush=True)
    res = {"what": "CN -> socket table from the first-generation sampler's own launch vs the cn_sockets pass (sampling alone, and "
                   "sample + decode)",
           "config": {"batch": BATCH, "reps": opts.reps},
           "shapes": shapes,
           "sampled_table_becomes_default": bool(all(s["every_new_rep_beats_every_old_rep"] and s["outputs_equal"]
                                                     for s in shapes.values()))}
    line = json.dumps(res)
    print(line, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
