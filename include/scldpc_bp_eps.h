/* libscldpc_hip — extension header: unlimited full BP at every point of a descending eps grid from one sampled code.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h and scldpc_eps.h, which this header
 * includes; they are declared HERE, not there, for the reason scldpc_cov.h gives: tests/test_abi.py ties scldpc.h to
 * _lib.EXPORTS and tests/test_eps_host.py ties scldpc_eps.h to _lib.EXPORTS_EPS.  The device entries of this header have a
 * buffer-contract file of their own, tests/test_gpu_buffer_contracts_bp_eps.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_BP_EPS_H
#define SCLDPC_BP_EPS_H

#include "scldpc_eps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fixpoint of unlimited flooding BP (scldpc_full_bp_fixpoint_device) of one code at every point of the grid, in one launch.
 * On the BEC the set flooding converges to is the maximal stopping set inside the erased set (over the CNs below cn_lim, the
 * only ones that fire) and does not depend on the schedule; the erased sets E_0 ⊇ E_1 ⊇ … of a descending grid are nested, so
 * the residual R_k of point k is fixpoint(R_{k-1} ∩ E_k): the kernel peels point 0, then reveals the VNs known at the next
 * point and peels on.  There is no iteration cap: a capped result depends on the schedule and the identity is false for it.
 *   d_levels      uint8 [ntrials][n] as scldpc_channel_levels_device writes them (any bytes are valid: VN j is erased at point
 *                 k iff lev[j] > k), only read;
 *   is_term       cn_lim = is_term ? nk : L * cns_pos, as scldpc_full_bp_fixpoint_device sets it: CNs at or beyond cn_lim never
 *                 fire and stay counted;
 *   d_counters    int32 [npoints][ntrials][SCLDPC_NCOUNTERS], point-major: d_counters[k] is the block
 *                 scldpc_full_bp_fixpoint_device writes for the channel of point k with the same is_term, equal value for value
 *                 in SCLDPC_C_NUM_ERASURES, _NUM_BLOCKS_ERR, _NUM_ERASURES_EXP, _NUM_BLOCKS_ERR_EXP, _NUM_ERASURES_P1 (0),
 *                 _STATUS (0) and _CHANNEL_ERASURES.  SCLDPC_C_ITERATIONS holds the peeling rounds of THIS point's stage (not
 *                 flooding iterations, and not that entry's barrier rounds); 0 at the points after the one that emptied the
 *                 residual.  scldpc_accumulate_run_device reads d_counters[k] as it is;
 *   d_erased_bits uint32 [npoints][ntrials][nw], or NULL: the erased set at the end of every point, as that entry's.
 * One 1024-thread workgroup per trial, the CN words in 16-bit or 32-bit form in LDS or, beyond it, 32-bit words in the
 * caller's workspace: scldpc_full_bp_eps_workspace_query(p, ntrials, adj16) bytes (0 where the words stay in LDS; < 0: the
 * error code), content on entry irrelevant.  The environment variable SCLDPC_DEBUG_EPS_QCAP (tests only, read per call) caps
 * the length of the two frontier queues, which forces the overflow re-scan at small shapes; only SCLDPC_C_ITERATIONS may
 * depend on it.
 *
 * One launch on `stream`, no allocation, no synchronisation; capturable.  Checks, in this order: the parameters; a negative
 * ntrials or a null d_vn_adj / d_levels / d_counters (with trials to decode); 1 <= npoints <= SCLDPC_EPS_MAX_POINTS
 * (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; dc <= 15, dv <= 8, dc * n < 2^24 and a shape whose VN bits, second VN bitmap
 * and scan bits leave two queues of 256 entries in 160 KiB of LDS (SCLDPC_ERR_TOO_LARGE); the workspace. */
int scldpc_full_bp_eps_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj, const uint8_t *d_levels,
                              int32_t npoints, int32_t is_term, int32_t *d_counters, uint32_t *d_erased_bits, void *d_workspace,
                              uint64_t workspace_bytes, void *stream);
int scldpc_full_bp_eps_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                    const uint8_t *d_levels, int32_t npoints, int32_t is_term, int32_t *d_counters,
                                    uint32_t *d_erased_bits, void *d_workspace, uint64_t workspace_bytes, void *stream);
int64_t scldpc_full_bp_eps_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16);

#ifdef __cplusplus
}
#endif

#endif
