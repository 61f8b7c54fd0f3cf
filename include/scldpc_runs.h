/* libscldpc_hip — extension header: error-propagation statistics of the window decoders (runs of failed positions), on the
 * device.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, which this header includes; they are
 * declared HERE, not there, for the reason scldpc_cov.h gives: tests/test_abi.py ties scldpc.h to _lib.EXPORTS.  The device
 * entries of this header have a buffer-contract file of their own, tests/test_gpu_buffer_contracts_runs.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's.
 *
 * Common to both entries: enqueue only — one kernel launch on `stream`, no allocation, no synchronisation, no workspace;
 * capturable.  The inputs are only read.  Every output that is ACCUMULATED is an integer sum, so it does not depend on the
 * batch split, the launch geometry, streams or ranks.  The checks need no device. */
#ifndef SCLDPC_RUNS_H
#define SCLDPC_RUNS_H

#include "scldpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDPC_RUNS_MAX_L      1024     /* chain: L <= this */
#define SCLDPC_RUNS_MAX_BINS   4096     /* stream: 2 <= nbins <= this */
#define SCLDPC_RUNS_MAX_PERIOD 4096     /* stream: the doping period, where d_phase is given */
#define SCLDPC_RUNS_CARRY      8        /* stream: int64 per stream carried from call to call */
#define SCLDPC_RUNS_MAX_DOPED  32       /* stream: doped positions per period (the streaming kernels' limit) */
#define SCLDPC_RUNS_MAX_NPOS   (1 << 28) /* stream: trace rows per stream and call (32-bit bins in LDS: 4 streams share them) */

/* Runs of failed positions of a terminated chain.  Trial t has the bits d_bits uint32 [ntrials][nw] (the layout of the chain
 * decoders' d_erased_bits and of the sweep decoders' d_lost_bits; bits at or beyond n = L * vns_pos are ignored whatever they
 * hold).  With V = vns_pos: e[u] = set bits in [uV, (u+1)V), f[u] = e[u] > 0, a RUN is a maximal interval [s, s + len) of
 * positions with f = 1.  ACCUMULATED, all int64:
 *   d_pos       [L][4]    [u][0] += f[u]; [u][1] += e[u]; [u][2] += 1 if u is the trial's first failing position;
 *                         [u][3] += 1 per run that starts at u;
 *   d_run_hist  [L+1][2]  [0][0] += 1 per trial without a failing position; [len][0] += 1 per run; [len][1] += 1 per run
 *                         with s + len == L (the burst reached the end of the chain);
 *   d_fail_hist [L+1]     [k] += 1 per trial with exactly k failing positions.
 * OVERWRITTEN per trial, each may be NULL:
 *   d_trial     int32 [ntrials][4] = (failing positions, first failing position or L, runs, longest run);
 *   d_fail_bits uint32 [ntrials][(L + 31) / 32] = the flags f, bit u & 31 of word u >> 5; padding bits are 0.
 *
 * Persistent 256-thread workgroups stride over the trials.  A wave takes a position: its lanes load the words that cover it,
 * mask the first and the last, popcount and wave-reduce into e[u] in LDS (no atomics).  The flags come from __ballot, the
 * runs from the 64-bit masks.  Sums go to LDS bins — 64-bit for the e sums, 32-bit for the counts, which a workgroup flushes
 * before any can overflow (every 2^22 trials: at most L/2 + 1 <= 513 runs per trial) — and the non-zero bins go out with one
 * 64-bit integer atomic each when the workgroup ends.
 *
 * Checks, in this order: the parameters (scldpc.h's check, SCLDPC_ERR_BAD_ARG / _TOO_LARGE); L <= SCLDPC_RUNS_MAX_L
 * (SCLDPC_ERR_TOO_LARGE); ntrials >= 0 (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK and touches nothing; then null d_bits,
 * d_pos, d_run_hist, d_fail_hist (SCLDPC_ERR_BAD_ARG). */
int scldpc_chain_runs_device(const scldpc_code_params *p, int32_t ntrials, const uint32_t *d_bits,
                             int64_t *d_pos, int64_t *d_run_hist, int64_t *d_fail_hist,
                             int32_t *d_trial, uint32_t *d_fail_bits, void *stream);

/* Runs and events of failed positions of the streaming decoder.  d_trace int32 [nstreams][npos][10] holds the rows the
 * streaming kernels write (scldpc_stream_run_device), in order, one call's rows after the other's in any split; only row[0]
 * (pos) and row[1] (nep, the value of decodeBP_SW_circular) are read.  With ms = dv - 1, a row with pos < ms decides nothing
 * and is skipped; otherwise d = pos - ms is the decided position and x = nep > 0.  doped(d) is position_is_doped
 * (BPF:1589-1612) for the ndoped ascending HOST values doped_positions; period = doped_positions[ndoped - 1] + 1, or 1 where
 * nothing is doped.  A RUN is a maximal sequence of consecutive decided positions with x = 1.  An EVENT merges runs that are
 * separated only by doped positions: a non-failing doped position neither ends nor lengthens it, a non-failing position that
 * is not doped ends it, and its length counts the failing positions in it.
 *
 * d_carry int64 [nstreams][SCLDPC_RUNS_CARRY], zero before a stream's first call, read and written back: [0] positions
 * decided so far, [1] length of the open run, [2] length of the open event (0 = none), [3] decided positions since the last
 * failing one, [4] failing positions so far, [5..7] zero.  Per decided position, in this order:
 *   1. carry[0] += 1, sums[0] += 1, phase[d % period] += (1, x, nep);
 *   2. if x: sums[1] += 1, sums[2] += nep; if no event is open: hist[3][min(d, nbins - 1)] += 1 if the stream has not failed
 *      before (time to first failure), else hist[2][min(since, nbins - 1)] += 1 and sums[7] += since (gap between events);
 *      then run += 1, event += 1, failed += 1, since = 0;
 *   3. else: if a run is open, hist[0][min(run, nbins - 1)] += 1, sums[3] += 1, sums[4] += run, run = 0; if an event is open
 *      and the position is not doped, hist[1][min(event, nbins - 1)] += 1, sums[5] += 1, sums[6] += event, event = 0;
 *      since += 1.
 * Runs and events still open after the last row stay in the carry (censored).  ACCUMULATED: d_hist int64 [4][nbins], d_sums
 * int64 [8], d_phase int64 [period][3] (may be NULL).
 *
 * d_counters int64 [nstreams][10] (the streaming kernels' counters), or NULL: a stream with d_counters[s][9] < 0 was marked
 * unusable, its trace rows are unwritten, and it is skipped entirely — nothing read from its rows, its carry untouched.
 * No value read from the trace is used as an index without a clamp.
 *
 * One wave per stream, four to a workgroup; 64 rows per step, ballots for x and doped, the state machine over the masks;
 * 32-bit LDS bins (64-bit for the nep sums), flushed once per workgroup with 64-bit integer atomics.
 *
 * Checks, in this order: the parameters; nstreams >= 0 and npos >= 0 (SCLDPC_ERR_BAD_ARG); npos <= SCLDPC_RUNS_MAX_NPOS
 * (SCLDPC_ERR_TOO_LARGE); 0 <= ndoped <= SCLDPC_RUNS_MAX_DOPED, doped_positions given where ndoped > 0, non-negative and
 * ascending (SCLDPC_ERR_BAD_ARG); 2 <= nbins <= SCLDPC_RUNS_MAX_BINS (SCLDPC_ERR_BAD_ARG); d_phase given and period >
 * SCLDPC_RUNS_MAX_PERIOD (SCLDPC_ERR_TOO_LARGE); nstreams == 0 or npos == 0 is SCLDPC_OK and touches nothing; then null
 * d_trace, d_carry, d_hist, d_sums (SCLDPC_ERR_BAD_ARG). */
int scldpc_stream_runs_device(const scldpc_code_params *p, int32_t nstreams, int32_t npos, const int32_t *d_trace,
                              const int64_t *d_counters, int32_t ndoped, const int32_t *doped_positions,
                              int32_t nbins, int64_t *d_carry, int64_t *d_hist, int64_t *d_sums,
                              int64_t *d_phase, void *stream);

#ifdef __cplusplus
}
#endif

#endif
