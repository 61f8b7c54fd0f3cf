"""What the error-propagation statistics (engine.chain_runs, engine.StreamRuns; csrc/err_runs.hip) cost where the command lines
run them, beside what they are added to and beside the only stand-in there was.

Chain, at BASELINE config 2's shape ((4,8), L = 50, N = 1000, eps = 0.48, full BP) and config 4's ((4,8), L = 100, N = 2000,
W = 10, 20 iterations per window, the ring window decoder), at the command lines' batch of 2048:
  * sample + decode through the Simulator with and without want_erased (Simulator(runs=True) against the default);
  * the chain_runs launch alone, with the bytes it reads over its time, and the same launch over 65 536 trials (the batch's bits
    repeated), where the time is the read and not the launch;
  * the stand-in: the bits copied to the host and tests/test_runs_host.np_chain_runs over them (its sums are compared with the
    device's).
Stream, at config 5's shape ((4,8), N = 5000, L = 50, W = 20, doped (24,), 512 streams, --chunk 64), at eps = 0.47 (hardly a
failing position) and 0.49 (bursts):
  * positions per second of the `sw` chunk loop (run + the nine sums the stop rule reads) as it is without --runs — the loop of
    the commit before this feature — and with trace + StreamRuns.update, on two sets of the same streams;
  * the stand-in: the chunk's trace copied to the host.
Device events, warm-up, --reps alternating repetitions, all values kept, outputs compared in every one.  Prints one JSON line;
--out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

HBM_READ_TBS = 6.29             # the achievable HBM rate of an MI355X (a float4 copy; 8.0 TB/s is the data sheet's peak)
CHAIN = {"config2_full_bp": dict(L=50, N=1000, eps=0.48, decoder="full", W=0, max_it=1000000, init_it=0),
         "config4_sw_ring": dict(L=100, N=2000, eps=0.47, decoder="sw", W=10, max_it=20, init_it=20)}
STREAM = dict(L=50, N=5000, W=20, doped=(24,), streams=512, chunk=64)
STREAM_EPS = (0.47, 0.49)        # hardly a failing position; bursts
BIG = 65536


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--chunks", type=int, default=4, help="stream: chunks per repetition")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if opts.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    from fl_scaling_sc_ldpc_amd import engine as E
    from test_runs_host import np_chain_runs, np_stream_runs
    assert torch.cuda.is_available(), "runs_speed measures on the GPU"

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, res

    def ms(ts):
        return {"median": round(1e3 * float(np.median(ts)), 4), "all": [round(1e3 * x, 4) for x in ts]}

    names = ("pos", "run_hist", "fail_hist")
    chain = {}
    for key, c in CHAIN.items():
        p, B = E.make_params(4, 8, c["L"], c["N"]), opts.batch
        kw = dict(decoder=c["decoder"], W=c["W"], max_it=c["max_it"], init_it=c["init_it"], batch=B, rng="philox", seed=1)
        plain, traced = BP.Simulator(p, **kw), BP.Simulator(p, runs=True, **kw)

        def step(sim):
            sim.fill_batch(0, c["eps"], 0, B)
            return sim.decode_batch(B)

        for _ in range(2):                                               # warm-up of all three, in the order of the timed loop
            step(plain)
            E.chain_runs(p, step(traced)["erased"])
        t_plain, t_erased, t_pass, equal, want = [], [], [], True, None
        for k in range(opts.reps):
            dt, res0 = event_timed(lambda: step(plain))
            t_plain.append(dt)
            cnt0 = res0["counters"].clone()
            dt, res = event_timed(lambda: step(traced))
            t_erased.append(dt)
            dt, acc = event_timed(lambda: E.chain_runs(p, res["erased"]))
            t_pass.append(dt)
            if want is None:                                             # the stand-in, once: the same frames every repetition
                t0 = time.perf_counter()
                words = res["erased"].cpu().numpy()
                t_copy = time.perf_counter() - t0
                t0 = time.perf_counter()
                want = np_chain_runs(E.unpack_bits(words, p.n), p.L, p.vns_pos)[0]
                t_host = time.perf_counter() - t0
            equal = equal and bool(torch.equal(cnt0, res["counters"])) and all((acc[n].cpu().numpy() == want[n]).all() for n in names)
        reps = -(-BIG // B)
        big = res["erased"].repeat(reps, 1)[:BIG].contiguous()
        E.chain_runs(p, big)
        t_big = []
        for k in range(opts.reps):
            dt, acc_big = event_timed(lambda: E.chain_runs(p, big))
            t_big.append(dt)
        if BIG % B == 0:
            equal = equal and all((acc_big[n].cpu().numpy() == reps * want[n]).all() for n in names)
        nbytes, big_bytes = B * p.nw * 4, BIG * p.nw * 4
        chain[key] = {
            "shape": dict(c, dv=4, dc=8, batch=B), "kernels": traced.kernel_choice(),
            "failed_positions_of_the_batch": int(want["pos"][:, 0].sum()), "runs_of_the_batch": int(want["run_hist"][1:, 0].sum()),
            "ms_per_batch": {"sample_decode": ms(t_plain), "sample_decode_want_erased": ms(t_erased), "chain_runs": ms(t_pass)},
            "want_erased_over_plain": round(float(np.median(t_erased) / np.median(t_plain)), 4),
            "runs_run_over_plain_run": round(float((np.median(t_erased) + np.median(t_pass)) / np.median(t_plain)), 4),
            "chain_runs_bytes_read": nbytes, "chain_runs_TBs": round(nbytes / float(np.median(t_pass)) * 1e-12, 4),
            "chain_runs_65536_trials": {"ms": ms(t_big), "bytes_read": big_bytes,
                                        "TBs": round(big_bytes / float(np.median(t_big)) * 1e-12, 4),
                                        "share_of_achievable_hbm_read": round(big_bytes / float(np.median(t_big)) * 1e-12 / HBM_READ_TBS, 4)},
            "host_stand_in": {"copy_of_the_bits_ms": round(1e3 * t_copy, 3), "np_chain_runs_ms": round(1e3 * t_host, 3)},
            "stand_in_over_chain_runs": round(float((t_copy + t_host) / np.median(t_pass)), 1),
            "outputs_equal": equal}
        del plain, traced, big
        torch.cuda.empty_cache()

    def stream_at(eps):
        s = dict(STREAM, eps=eps)
        p = E.make_params(4, 8, s["L"], s["N"])
        S, chunk = s["streams"], s["chunk"]
        st_a = E.Streams(p, S, 1, s["eps"], s["W"], s["doped"], stream0=0)
        st_b = E.Streams(p, S, 1, s["eps"], s["W"], s["doped"], stream0=0)
        sr = E.StreamRuns(p, S, s["doped"], 256)
        ref = np_stream_runs(S, 4, s["doped"], 256)

        def sums_of(cnt):                                                    # what the `sw` loop reads after every chunk
            return torch.cat([cnt[:, :8].sum(dim=0), (cnt[:, 9] < 0).sum().reshape(1)]).cpu().numpy()

        def loop_plain():
            for _ in range(opts.chunks):
                tot = sums_of(st_a.run(chunk)[0])
            return tot

        traces = []

        def loop_runs():
            for _ in range(opts.chunks):
                cnt, tr = st_b.run(chunk, trace=True)
                sr.update(tr, cnt)
                tot = sums_of(cnt)
                traces.append(tr)
            return tot

        loop_plain()
        loop_runs()
        t_a, t_b, t_copy, equal = [], [], [], True
        for k in range(opts.reps):
            dt, tot_a = event_timed(loop_plain)
            t_a.append(dt)
            dt, tot_b = event_timed(loop_runs)
            t_b.append(dt)
            t0 = time.perf_counter()
            host = traces[-1].cpu().numpy()
            t_copy.append(time.perf_counter() - t0)
            for tr in traces:
                ref.feed(tr.cpu().numpy())
            del traces[:]
            equal = equal and (tot_a == tot_b).all() and (sr.hist.cpu().numpy() == ref.hist).all() \
                and (sr.sums.cpu().numpy() == ref.sums).all() and (sr.phase.cpu().numpy() == ref.phase).all() \
                and (sr.carry.cpu().numpy() == ref.carry).all()
        positions = S * chunk * opts.chunks
        t0 = time.perf_counter()
        np_stream_runs(S, 4, s["doped"], 256).feed(host)
        t_np = time.perf_counter() - t0
        stream = {
            "shape": dict(s, dv=4, dc=8, nbins=256, chunks_per_repetition=opts.chunks),
            "ms_per_repetition": {"chunk_loop": ms(t_a), "chunk_loop_trace_stream_runs": ms(t_b)},
            "positions_per_s": {"chunk_loop": round(positions / float(np.median(t_a)), 1),
                                "chunk_loop_trace_stream_runs": round(positions / float(np.median(t_b)), 1)},
            "runs_loop_over_plain_loop": round(float(np.median(t_b) / np.median(t_a)), 4),
            "failed_positions": int(ref.sums[1]), "runs": int(ref.sums[3]), "events": int(ref.sums[5]),
            "host_stand_in": {"copy_of_one_chunk_trace_ms": ms(t_copy), "trace_bytes_per_chunk": S * chunk * 40,
                              "np_stream_runs_one_chunk_ms": round(1e3 * t_np, 3)},
            "outputs_equal": bool(equal)}
        return stream

    streams = {str(eps): stream_at(eps) for eps in STREAM_EPS}
    result = {"what": "engine.chain_runs per batch beside sample + decode with and without the erased bits, and engine.StreamRuns in "
                      "the sw chunk loop, each beside its host stand-in",
              "achievable_hbm_read_TBs": HBM_READ_TBS, "reps": opts.reps, "chain": chain, "stream": streams,
              "outputs_equal": bool(all(v["outputs_equal"] for v in chain.values()) and all(v["outputs_equal"] for v in streams.values())),
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
