/* libscldpc_hip — extension header: exact integer Gram matrices of degree-1 trajectories between chosen peeling steps.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, which this header includes; they are
 * declared HERE, not there, for the reason scldpc_ensembles.h gives: tests/test_abi.py ties scldpc.h to _lib.EXPORTS.  The
 * device entry of this header has a buffer-contract file of its own, tests/test_gpu_buffer_contracts_cov.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_COV_H
#define SCLDPC_COV_H

#include "scldpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDPC_COV_MAX_STEPS 4096       /* 1 <= k <= this */
#define SCLDPC_COV_STEP_CLAMPED 1       /* status word: an element of d_steps lay outside [0, ncols) and was clamped into it */

/* The second moments of the trajectories between steps (the finite-length-scaling analysis reads the Ornstein-Uhlenbeck
 * parameter off how the covariance of r1 between two steps decays with their distance).  d_r1 is int32 [ntrials][ncols]
 * exactly as scldpc_peel_pick_device and scldpc_peel_pick_device_adj16_deg write it (counts: values >= 0; the kernels read them
 * as unsigned 32-bit); d_steps holds k column indices.  With
 * x[t][i] = d_r1[t][d_steps[i]] and m[t][i] = (x[t][i] != 0 ? 1 : 0), d_gram int64 [3][k][k] is ACCUMULATED in place, like
 * scldpc_r1_moments_device's output:
 *     d_gram[0][i][j] += sum_t m[t][i] * m[t][j]     pairs of steps at which the trial was still decoding
 *     d_gram[1][i][j] += sum_t x[t][i] * m[t][j]     (not symmetric)
 *     d_gram[2][i][j] += sum_t x[t][i] * x[t][j]
 * On the diagonal these are scldpc_r1_moments_device's three rows at column d_steps[i].  Every product and sum is formed in
 * 64-bit integers, no floating point anywhere: the result is exact while the sums fit 63 bits, and it does not depend on
 * how a run is cut into calls.  The covariance on the pair mask is g2/g0 - (g1[i][j]/g0) * (g1[j][i]/g0).
 *
 * Workspace: scldpc_r1_gram_workspace_bytes(ntrials, k) bytes at a 16-byte aligned address, caller-owned, content on entry
 * irrelevant (needs no device; -1 and a text in scldpc_last_error for ntrials < 0 or k outside 1 .. SCLDPC_COV_MAX_STEPS).  Its
 * first int32 is the STATUS WORD of the call: the call writes 0 there and the kernels OR in SCLDPC_COV_STEP_CLAMPED where an
 * element of d_steps lay outside [0, ncols): the kernels never read outside d_r1, such a step is read at column 0 or
 * ncols - 1, and the caller reads the word after the stream has finished — d_gram then holds sums of the clamped columns.
 * The rest is the gathered panel.  scldpc_r1_gram_trial_splits says over how many workgroups per output tile the launch of
 * these sizes splits the trials (needs no device; the same -1).
 *
 * Two kernel launches and a 4-byte memset on `stream`; no allocation, no synchronisation; capturable.  d_r1 and d_steps are
 * only read.  Checks, in this order: ntrials >= 0; 1 <= k <= SCLDPC_COV_MAX_STEPS; ncols >= 0 (SCLDPC_ERR_BAD_ARG);
 * ntrials == 0 is SCLDPC_OK and touches nothing; then ncols >= 1, null buffers, the alignment and the size of the workspace
 * (SCLDPC_ERR_BAD_ARG). */
int64_t scldpc_r1_gram_workspace_bytes(int32_t ntrials, int32_t k);
int32_t scldpc_r1_gram_trial_splits(int32_t ntrials, int32_t k);
int scldpc_r1_gram_device(int32_t ntrials, int32_t ncols, const int32_t *d_r1, int32_t k, const int32_t *d_steps,
                          int64_t *d_gram, void *d_ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
