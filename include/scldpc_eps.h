/* libscldpc_hip — extension header: a whole eps grid from one sampled code.  The channel of a trial as LEVELS (at how many
 * points of a descending eps grid each VN is erased) and the sweep decoder that walks the grid downwards, peeling on from the
 * residual of the point before.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, which this header includes; they are
 * declared HERE, not there, for the reason scldpc_cov.h gives: tests/test_abi.py ties scldpc.h to _lib.EXPORTS.  The device
 * entries of this header have a buffer-contract file of their own, tests/test_gpu_buffer_contracts_eps.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_EPS_H
#define SCLDPC_EPS_H

#include "scldpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDPC_EPS_MAX_POINTS 64        /* 1 <= npoints <= this */

/* The channel of trials trial0 .. trial0 + ntrials - 1 at npoints erasure probabilities at once.  eps[k] (host memory, each in
 * [0, 1]) maps to the threshold thresh_k = ceil(eps[k] * RAND_MAX) of every Philox sampler, and the THRESHOLDS must be strictly
 * decreasing (two eps that round to one threshold are one point: merge them before the call).
 *   d_levels uint8 [ntrials][n]: lev[j] = the number of points at which VN j is erased = #{k : (draw_j >> 1) < thresh_k}, so VN j
 *   is erased at point k iff lev[j] > k.  The draw is the samplers': VN j = 32 w + 4 c + u reads word u of
 *   philox4x32_10(w * 8 + c, 0x80000000, trial_lo, trial_hi, seed_lo, seed_hi).  VNs of the ndoped positions doped_positions[]
 *   (host memory, each in [0, L), at most 32) get level 0.  Every byte [0, n) of a trial's row is written, no byte beyond.
 * Contract: for every k, the bits (lev > k), packed 32 to a word, are the d_chan_bits row scldpc_sample_philox_device and
 * scldpc_sample_philox_ensemble_device (every ensemble) write for eps[k] on the same (seed, trial, doped positions).
 *
 * One launch on `stream`, no workspace, no allocation, no synchronisation; capturable.  Checks, in this order: the parameters;
 * a negative ntrials or a null d_levels (with trials to write); 0 <= ndoped <= 32; 1 <= npoints <= SCLDPC_EPS_MAX_POINTS and a
 * non-null eps; every eps in [0, 1]; strictly decreasing thresholds (all SCLDPC_ERR_BAD_ARG, before any device work);
 * ntrials == 0 is SCLDPC_OK and touches nothing; the doped positions. */
int scldpc_channel_levels_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials, int32_t npoints,
                                 const double *eps, int32_t ndoped, const int32_t *doped_positions, uint8_t *d_levels,
                                 void *stream);

/* Sweep peeling (scldpc_peel_sweep_device with sweep_start = 0) of one code at every point of the grid, in one launch.
 * With the sweep starting at CN 0 the residual of sweep peeling is the maximal stopping set inside the erased set; the erased
 * sets E_0 ⊇ E_1 ⊇ … of a descending grid are nested, so the residual R_k of point k is residual(R_{k-1} ∩ E_k): the kernel
 * peels point 0, then reveals the VNs known at the next point and peels on.  There is no sweep_start argument: with
 * sweep_start > 0 a CN below it fires only on a transition and the identity is false.
 *   d_levels    uint8 [ntrials][n] as scldpc_channel_levels_device writes them (any bytes are valid: VN j is erased at point k
 *               iff lev[j] > k), only read;
 *   d_out       int32 [npoints][ntrials][8], point-major: d_out[k] is the [ntrials][8] block scldpc_peel_sweep_device writes
 *               for the channel of point k and the same total_size, lost_lo, lost_hi with sweep_start = 0 — [0] #lost,
 *               [1] #lost in components of more than 2 VNs, [2] #positions over those components, [7] #erased VNs at point k,
 *               equal value for value; [5] the peeling rounds of THIS point's stage (not that entry's count), [6] its scans after
 *               the first (0 unless a queue overflowed, as scldpc_peel_sweep_device_sock16 counts them); [3] and [4] are 0.
 *               scldpc_accumulate_peel_device reads d_out[k] as it is;
 *   d_lost_bits uint32 [npoints][ntrials][nw], or NULL: the lost set of every point, as that entry's.
 * One 1024-thread workgroup per trial, the CN words in 16-bit or 32-bit form in LDS or, beyond it, 32-bit words in the
 * caller's workspace: scldpc_peel_sweep_eps_workspace_query(p, ntrials, adj16) bytes (0 where the words stay in LDS; < 0: the
 * error code), content on entry irrelevant.  The environment variable SCLDPC_DEBUG_EPS_QCAP (tests only, read per call) caps
 * the length of the two frontier queues, which forces the overflow re-scan at small shapes; only [6] depends on it (a re-scan
 * finds exactly the CNs the overflowed queue would have held, so not even the number of rounds changes).
 *
 * One launch on `stream`, no allocation, no synchronisation; capturable.  Checks, in this order: the parameters; a negative
 * ntrials or a null d_vn_adj / d_levels / d_out (with trials to decode); 1 <= npoints <= SCLDPC_EPS_MAX_POINTS; total_size in
 * [0, ncn], lost_lo >= 0, lost_hi <= ncn (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; dc <= 15, dv <= 8, dc * n < 2^24 and
 * a shape whose VN bits, second VN bitmap and scan bits leave two queues of 256 entries in 160 KiB of LDS
 * (SCLDPC_ERR_TOO_LARGE); the workspace. */
int scldpc_peel_sweep_eps_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj, const uint8_t *d_levels,
                                 int32_t npoints, int32_t total_size, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                 uint32_t *d_lost_bits, void *d_workspace, uint64_t workspace_bytes, void *stream);
int scldpc_peel_sweep_eps_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                       const uint8_t *d_levels, int32_t npoints, int32_t total_size, int32_t lost_lo,
                                       int32_t lost_hi, int32_t *d_out, uint32_t *d_lost_bits, void *d_workspace,
                                       uint64_t workspace_bytes, void *stream);
int64_t scldpc_peel_sweep_eps_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16);

#ifdef __cplusplus
}
#endif

#endif
