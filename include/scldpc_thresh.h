/* libscldpc_hip — extension header: the exact erasure threshold of every frame under unlimited full BP, bisected on the device.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, scldpc_eps.h and scldpc_bp_eps.h, the last
 * of which this header includes; they are declared HERE, not there, for the reason scldpc_cov.h gives: every extension header is
 * tied to a tuple of its own in _lib.py by a test of its own (this one to _lib.EXPORTS_THRESH by tests/test_thresh_host.py).  The
 * device entries of this header have a buffer-contract file of their own, tests/test_gpu_buffer_contracts_thresh.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_THRESH_H
#define SCLDPC_THRESH_H

#include "scldpc_bp_eps.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDPC_THRESH_NCOLS 8
#define SCLDPC_THRESH_MAX 2147483647u   /* RAND_MAX: erasure_threshold(1.0), the largest threshold there is */

/* The 31-bit channel keys of trials trial0 .. trial0 + ntrials - 1, one per VN.
 *   d_keys   uint32 [ntrials][n]: entry j holds draw >> 1 of exactly the Philox call the samplers and
 *            scldpc_channel_levels_device make for VN j (VN j = 4 call + u reads word u of philox4x32_10(call, 0x80000000, trial,
 *            seed)); the VNs of a doped position hold 0xFFFFFFFF, which no threshold exceeds: they are never erased.
 * For every eps, pack(d_keys[t][j] < erasure_threshold(eps)) is the channel scldpc_sample_philox_device writes at eps for the same
 * (seed, trial, doped): VN j is erased iff its key is below the threshold, so the erased sets of all eps are nested.
 * Each thread makes one Philox call and one 16-byte store where every row is 16-byte aligned and n % 4 == 0, else scalar stores;
 * no word at or past n is written.  No LDS, no workspace; launches on `stream` (trials ride on blockIdx.y in slabs of 65535).
 * Checks, in this order: the parameters; a negative ntrials or a null d_keys (with trials to write); 0 <= ndoped <= 32 and a
 * non-null doped_positions where ndoped > 0 (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; every doped position in [0, L). */
int scldpc_channel_keys_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials, int32_t ndoped,
                               const int32_t *doped_positions, uint32_t *d_keys, void *stream);

/* The critical threshold of every frame.  With E(t) = {j : key[j] < t} and S(t) the maximal stopping set inside E(t) over the CNs
 * below cn_lim — what unlimited flooding BP (scldpc_full_bp_device with no cap, scldpc_full_bp_fixpoint_device) leaves of the
 * channel E(t) — S is monotone in t, and the frame has one integer
 *     T* = min { t : S(t) is non-empty }:
 * it fails at eps iff T* <= erasure_threshold(eps).  The kernel decodes E(t_hi), then bisects on the integer threshold inside the
 * residual: S(t) = S(S(t') ∩ E(t)) for t <= t', so every stage peels only what the stage before left.
 *   d_keys      uint32 [ntrials][n], only read.  ANY keys are valid input (scldpc_channel_keys_device writes the samplers');
 *   t_lo, t_hi  the window, 0 <= t_lo < t_hi <= SCLDPC_THRESH_MAX;
 *   is_term     cn_lim = is_term ? nk : L * cns_pos, as scldpc_full_bp_eps_device sets it;
 *   d_rows      int32 [ntrials][SCLDPC_THRESH_NCOLS]:
 *                 [0] thresh   T* where status == 0; t_lo where status == 2; -1 where status == 1
 *                 [1] status   0: t_lo < T* <= t_hi.  1: the frame decodes at t_hi (T* > t_hi).  2: S(t_lo) is non-empty
 *                              (T* <= t_lo)
 *                 [2] size     #VNs of the critical residual: S(T*) (status 0) or S(t_lo) (status 2); 0 for status 1
 *                 [3], [4]     the lowest and the highest VN position with a bit in that residual; -1 for status 1
 *                 [5] stages   peel stages run, the first decode included (diagnostic: depends on how the search is cut)
 *                 [6] rescans  re-scans after a queue overflow, summed over the stages (diagnostic)
 *                 [7] erased   #VNs with key < t_hi: the channel erasures at the top of the window
 *   d_bits      uint32 [ntrials][nw], or NULL: the critical residual as a bitmap in the layout of d_erased_bits (all zero for
 *               status 1; the padding bits of the last word are 0).
 * After a non-empty stage the upper end drops to max(key over the residual) + 1: S(t) is that residual for every t above its
 * largest key, so T* - 1 is the largest key of S(T*).  At most 33 stages without that cut.
 * One 1024-thread workgroup per frame, the CN words in 16-bit or 32-bit form in LDS or, beyond it, 32-bit words in the caller's
 * workspace: scldpc_frame_threshold_workspace_query(p, ntrials, adj16) bytes (0 where the words stay in LDS; < 0: the error
 * code), content on entry irrelevant.  SCLDPC_DEBUG_EPS_QCAP (tests only, read per call) caps the two frontier queues as it does
 * for scldpc_full_bp_eps_device; only columns 5 and 6 may depend on it.
 *
 * One launch on `stream`, no allocation, no synchronisation; capturable.  Checks, in this order: the parameters; a negative
 * ntrials or a null d_vn_adj / d_keys / d_rows (with trials to decode); 0 <= t_lo < t_hi <= SCLDPC_THRESH_MAX
 * (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; dc <= 15, dv <= 8, dc * n < 2^24 and a shape whose VN bits, second VN bitmap
 * and scan bits leave two queues of 256 entries in 160 KiB of LDS (SCLDPC_ERR_TOO_LARGE); the workspace. */
int scldpc_frame_threshold_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj, const uint32_t *d_keys,
                                  uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t *d_rows, uint32_t *d_bits,
                                  void *d_workspace, uint64_t workspace_bytes, void *stream);
int scldpc_frame_threshold_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                        const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t *d_rows,
                                        uint32_t *d_bits, void *d_workspace, uint64_t workspace_bytes, void *stream);
int64_t scldpc_frame_threshold_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16);

#ifdef __cplusplus
}
#endif

#endif
