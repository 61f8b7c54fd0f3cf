/* libscldpc_hip — extension header: the exact erasure threshold of every VN and of every position under unlimited full BP, walked
 * on the device.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h and scldpc_thresh.h, which this header
 * includes; they are declared HERE, not there, for the reason scldpc_cov.h gives: every extension header is tied to a tuple of
 * its own in _lib.py by a test of its own (this one to _lib.EXPORTS_VN_THRESH by tests/test_vn_thresh_host.py).  The device
 * entries of this header have a buffer-contract file of their own, tests/test_gpu_buffer_contracts_vn_thresh.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_VN_THRESH_H
#define SCLDPC_VN_THRESH_H

#include "scldpc_thresh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDPC_VNT_NCOLS 8
#define SCLDPC_VNT_MAX_POINTS 256
#define SCLDPC_VNT_NONE 0xFFFFFFFFu     /* a threshold no erasure probability reaches: the VN (position) is never lost */

/* The threshold of every VN.  With E(t) = {j : key[j] < t} and S(t) the maximal stopping set inside E(t) over the CNs below
 * cn_lim, as scldpc_thresh.h defines them, S is monotone in t and VN j has one integer
 *     tau(j) = min { t : j in S(t) }:
 * j is lost at eps iff tau(j) <= erasure_threshold(eps).  Inside the window t_lo < t_hi the kernel decodes E(t_hi), which leaves
 * R = S(t_hi), and walks down: with m the largest key of R, S(t) = R for every t above m; the VNs of R with key m leave E at
 * t = m, the peeling they start runs to its end, and everything it removes has tau = m + 1; R is then S(m).  The walk ends when
 * R is empty or every key of R is below t_lo; what is left then is S(t_lo) and gets tau = t_lo, meaning "tau <= t_lo".  A VN
 * outside S(t_hi) gets SCLDPC_VNT_NONE.  The least tau of a frame is scldpc_frame_threshold_device's T*.
 *   d_keys, t_lo, t_hi, is_term   as scldpc_frame_threshold_device;
 *   npoints, grid   0 <= npoints <= SCLDPC_VNT_MAX_POINTS thresholds in HOST memory, strictly ascending, t_lo <= grid[0] and
 *                   grid[npoints - 1] <= t_hi; copied into the kernel's arguments;
 *   d_rows          int32 [ntrials][SCLDPC_VNT_NCOLS]:
 *                     [0] thresh, [1] status   exactly scldpc_frame_threshold_device's columns 0 and 1
 *                     [2] top      #VNs of S(t_hi)
 *                     [3] size     #VNs of the critical residual, scldpc_frame_threshold_device's column 2
 *                     [4] steps    the number of distinct values of tau in (t_lo, t_hi] (defined by the keys, no diagnostic)
 *                     [5] scans    candidate scans of the walk (diagnostic: depends on the capacities)
 *                     [6] rescans  scans repeated after the candidate list or a frontier queue overflowed (diagnostic)
 *                     [7] erased   #VNs with key < t_hi
 *   d_pos_thresh    uint32 [ntrials][L]: the least tau over the VNs of the position, SCLDPC_VNT_NONE where none is lost;
 *   d_counts        int32 [ntrials][npoints], or NULL where npoints == 0: counts[k] = #{j : tau(j) <= grid[k]} = #VNs of S(grid[k]);
 *   d_tau           uint32 [ntrials][n], or NULL: tau of every VN.  Every word of a row is written once, no word at or past n.
 * One 1024-thread workgroup per frame with scldpc_frame_threshold_device's CN-word forms; the workspace is
 * scldpc_vn_threshold_workspace_query(p, ntrials, adj16) bytes (0 where the words stay in LDS; < 0: the error code), content on
 * entry irrelevant.  SCLDPC_DEBUG_VNT_CCAP (tests only, read per call) caps the candidate list and SCLDPC_DEBUG_EPS_QCAP the two
 * frontier queues; only columns 5 and 6 may depend on them.
 *
 * One launch on `stream`, no allocation, no synchronisation; capturable.  Checks, in this order: the parameters; a negative
 * ntrials or a null d_vn_adj / d_keys / d_rows / d_pos_thresh (with trials to decode); 0 <= t_lo < t_hi <= SCLDPC_THRESH_MAX;
 * 0 <= npoints <= SCLDPC_VNT_MAX_POINTS, a non-null grid and d_counts where npoints > 0, the grid ascending inside the window
 * (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; dc <= 15, dv <= 8, dc * n < 2^24 and a shape whose VN bits, scan bits,
 * position words, grid and candidate list (1536 words; from n = 47 000 on the regions of scldpc_frame_threshold_device, which
 * are larger, so that a shape takes the same CN-word form in both) leave two queues of 256 entries in 160 KiB of LDS
 * (SCLDPC_ERR_TOO_LARGE); the workspace.
 * The diagnostics: the first candidate scan of a frame looks at the keys in [t_hi - w, t_hi), w = t_hi * max(1, cap / 2) /
 * |S(t_hi)| clamped to [1, t_hi - t_lo] with cap the list's capacity (512, or SCLDPC_DEBUG_VNT_CCAP below it); more candidates
 * than cap halve w and count in column 6; w == 1 needs no list. */
int scldpc_vn_threshold_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj, const uint32_t *d_keys,
                               uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t npoints, const uint32_t *grid,
                               int32_t *d_rows, uint32_t *d_pos_thresh, int32_t *d_counts, uint32_t *d_tau, void *d_workspace,
                               uint64_t workspace_bytes, void *stream);
int scldpc_vn_threshold_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                     const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t npoints,
                                     const uint32_t *grid, int32_t *d_rows, uint32_t *d_pos_thresh, int32_t *d_counts,
                                     uint32_t *d_tau, void *d_workspace, uint64_t workspace_bytes, void *stream);
int64_t scldpc_vn_threshold_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16);

#ifdef __cplusplus
}
#endif

#endif
