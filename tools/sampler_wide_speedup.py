"""What the second-generation sampler beyond 8192 sockets per CN position gains — or loses — over the first-generation sampler
on the paths that read a CN -> socket table, in batches of 2048 frames.

  old path:        sample_philox(adj16) + cn_sockets [+ decoder]
  old table path:  sample_philox_sock [+ decoder]                  (--sampled-table on: the table from the first generation's launch)
  new path:        sample_philox_wide_sock16 [+ decoder]           (--sampler2-wide on: sampler_v2_wide.hip)

All three are timed alone (sampling, table included) and end to end with the decoder that consumes the table.  Host clock around
work that ends in a device synchronise; every shape warmed up first; the paths ALTERNATE over --reps repetitions and all values
are kept.  The rows, the channel words and (as a set per CN) the table of the paths are compared on the way, and so are the
decoder's counters (outputs_equal).

Each shape is measured by a child process of its own under a time limit; the first child that fails or runs out of time ends
the run with its exit status (nothing more is started).  Prints one JSON line; --out writes it too.  sampler2_wide_becomes_default
is the rule bp_decoding.SAMPLER2_DEG_BY_DEFAULT documents: on every shape every repetition of the new path is faster end to end
than every repetition of both old forms, with equal outputs.  No speed-up is fixed in advance: the first-generation kernel of
these sizes already ranks only the straddlers."""
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

# name: dv, dc, L, N, decoder, its arguments, ε, frames per timed pass (the shapes of tools/sampled_table_speedup.py beyond 8192
# sockets per position that the sampler takes, and bp_lim_iter at bp_traj's shipped size)
SHAPES = {
    "4_8_L50_N5000_bp_traj_truncated_500it_rows": (4, 8, 50, 5000, "wide", dict(max_it=500, is_term=False, rows_cap=500), 0.47, 8192),
    "4_8_L100_N2500_sw_W10_20it": (4, 8, 100, 2500, "sw_ring", dict(W=10, max_it=20), 0.47, 8192),
    "3_6_L50_N5000_bp_traj_truncated_500it_rows": (3, 6, 50, 5000, "degwide", dict(max_it=500, is_term=False, rows_cap=500), 0.47, 8192),
    "4_8_L50_N5000_bp_lim_iter_500it": (4, 8, 50, 5000, "wide", dict(max_it=500, is_term=True), 0.47, 8192),
}
BATCH = 2048
PATHS = ("old", "old_table", "new")


def measure(name, reps):
    import torch
    from fl_scaling_sc_ldpc_amd import engine as E
    assert torch.cuda.is_available(), "sampler_wide_speedup measures on the GPU"
    dv, dc, L, N, decoder, kw, eps, F = SHAPES[name]
    p = E.make_params(dv, dc, L, N)
    assert E.wide_sock16_supported(p) and E.sample_philox_sock_supported(p)
    B = BATCH
    a = torch.empty((B, p.n, dv), dtype=torch.int16, device="cuda")
    cs = torch.empty((B, p.nk, dc), dtype=torch.int16, device="cuda")
    ch = torch.empty((B, p.nw), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, E.NCOUNTERS), dtype=torch.int32, device="cuda")

    def decode():
        if decoder == "wide":
            return E.full_bp_wide(p, a, cs, ch, counters=cnt, **kw)
        if decoder == "degwide":
            return E.full_bp_deg(p, a, cs, ch, counters=cnt, wide=True, **kw)
        return E.sw_bp(p, a, ch, kw["W"], kw["max_it"], counters=cnt, ring=True, d_cn_sock=cs)

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

    def old_table_sample(b0):
        E.sample_philox_sock(p, 11, b0, B, eps, out=(a, cs, ch))

    def new_sample(b0):
        E.sample_philox_wide_sock16(p, 11, b0, B, eps, out=(a, cs, ch))

    sample = {"old": old_sample, "old_table": old_table_sample, "new": new_sample}

    def path(which):
        def run():
            for b0 in range(0, F, B):
                sample[which](b0)
                decode()
        return run

    def table_sets():
        """The tables of the first 64 trials with every CN's entries in ascending order (uint16 values)."""
        u8 = cs[:64].view(torch.uint8).view(64, p.nk, dc, 2)
        return torch.sort(u8[..., 1].int() * 256 + u8[..., 0].int(), dim=-1)[0]

    # warm-up of every kernel, and the outputs of the three paths compared (one batch)
    outs = {}
    for which in PATHS:
        a.fill_(-1), cs.fill_(-1), ch.fill_(-1)
        sample[which](0)
        r = decode()
        torch.cuda.synchronize()
        rows = r.get("rows")
        if rows is not None:                                                # the rows of the iterations that ran
            its = r["counters"][:, 5].long()
            rows = rows * (torch.arange(rows.shape[1], device=its.device)[None, :] < its[:, None])[:, :, None]
        outs[which] = (a.clone(), ch.clone(), r["counters"].clone(), table_sets()) + ((rows.clone(),) if rows is not None else ())
    equal = all(bool(torch.equal(x, y)) for which in PATHS[1:] for x, y in zip(outs["old"], outs[which]))
    iters = float(outs["old"][2][:, 5].double().mean().item())
    del outs
    t = {which: [] for which in PATHS}
    for _ in range(reps):
        for which in PATHS:
            t[which].append(timed(path(which)))
    nrep = max(2, F // B)
    stage = {"sample_philox+cn_sockets": [], "sample_philox_sock": [], "sample_philox_wide_sock16": [], "sample_philox": [],
             "cn_sockets": [], "decoder": []}
    for _ in range(reps):
        stage["sample_philox+cn_sockets"].append(timed(lambda: [old_sample(0) for _ in range(nrep)]) / nrep)
        stage["sample_philox_sock"].append(timed(lambda: [old_table_sample(0) for _ in range(nrep)]) / nrep)
        stage["sample_philox_wide_sock16"].append(timed(lambda: [new_sample(0) for _ in range(nrep)]) / nrep)
        stage["sample_philox"].append(timed(lambda: [E.sample_philox(p, 11, 0, B, eps, out=(a, ch)) for _ in range(nrep)]) / nrep)
        stage["cn_sockets"].append(timed(lambda: [E.cn_sockets(p, a, out=cs) for _ in range(nrep)]) / nrep)
        stage["decoder"].append(timed(lambda: [decode() for _ in range(nrep)]) / nrep)
    st = {which: stats(t[which], F) for which in PATHS}
    med = {k: float(np.median(v)) for k, v in stage.items()}
    return {"dv": dv, "dc": dc, "L": L, "N": N, "sockets_per_position": p.cns_pos * dc, "eps": eps, "decoder": decoder,
            "decoder_args": kw, "batch": B, "frames_per_pass": F, "mean_iterations": round(iters, 1),
            "old_path": st["old"], "old_table_path": st["old_table"], "new_path": st["new"],
            "speedup_end_to_end": {"over_old": round(st["old"]["median_s"] / st["new"]["median_s"], 3),
                                   "over_old_table": round(st["old_table"]["median_s"] / st["new"]["median_s"], 3)},
            "ratio_new_over_old": {
                "end_to_end": {"old": round(st["new"]["median_s"] / st["old"]["median_s"], 3),
                               "old_table": round(st["new"]["median_s"] / st["old_table"]["median_s"], 3)},
                "alone": {"old": round(med["sample_philox_wide_sock16"] / med["sample_philox+cn_sockets"], 3),
                          "old_table": round(med["sample_philox_wide_sock16"] / med["sample_philox_sock"], 3)}},
            "stages_ms_per_batch": {k: {"median": round(1e3 * med[k], 3), "all": [round(1e3 * x, 3) for x in v]}
                                    for k, v in stage.items()},
            "speedup_sampling_with_table": {
                "over_old": round(med["sample_philox+cn_sockets"] / med["sample_philox_wide_sock16"], 3),
                "over_old_table": round(med["sample_philox_sock"] / med["sample_philox_wide_sock16"], 3)},
            "every_new_rep_beats_every_old_rep": bool(max(t["new"]) < min(t["old"]) and max(t["new"]) < min(t["old_table"])),
            "outputs_equal": equal, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
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
            print("sampler_wide_speedup: %s ran out of its %d s; nothing more is started" % (name, opts.limit), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("sampler_wide_speedup: %s ended with status %d; nothing more is started" % (name, r.returncode), file=sys.stderr)
            return r.returncode
        shapes[name] = json.loads(r.stdout.decode().strip().split("\n")[-1])
        print("sampler_wide_speedup: %s done" % name, file=sys.stderr, flush=True)
    res = {"what": "second-generation sampler beyond 8192 sockets per position vs the first-generation sampler with the cn_sockets "
                   "pass and with the table from its own launch (sampling alone, and sample + decode)",
           "config": {"batch": BATCH, "reps": opts.reps},
           "shapes": shapes,
           "sampler2_wide_becomes_default": bool(all(s["every_new_rep_beats_every_old_rep"] and s["outputs_equal"]
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
