/* libscldpc_hip — extension header: the size spectrum of the connected components (stopping sets) of a set of VNs, per trial,
 * on the device.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, which this header includes; they are
 * declared HERE, not there, for the reason scldpc_cov.h gives: tests/test_abi.py ties scldpc.h to _lib.EXPORTS.  The device
 * entry of this header has a buffer-contract file of its own, tests/test_gpu_buffer_contracts_ss.py.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_SS_H
#define SCLDPC_SS_H

#include "scldpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDPC_SS_MAX_BINS 4096         /* 2 <= nbins <= this */
#define SCLDPC_SS_POS_SIZES 8           /* columns of d_pos_hist */
#define SCLDPC_SS_BAD_CN 1              /* status word: a CN id outside [0, ncn) was met and that edge skipped */

/* extract_stopping_sets (PD:1077-1095) for a batch: the members of trial t are the VNs j whose bit j is set in
 * d_member_bits uint32 [ntrials][nw] (the layout of a sweep decoder's d_lost_bits and of full BP's d_erased_bits; bits at or
 * beyond n in the last word are ignored; ANY subset is valid, it need not be a stopping set).  Two members are joined if they
 * share a CN, a component is a class of the transitive closure and its size s the number of its VNs.
 *   adj_kind 0: d_vn_adj int32 [ntrials][n][dv], global CN ids (any ensemble);
 *   adj_kind 1: d_vn_adj uint16 [ntrials][n][dv], ids local to CN position pos + i (the Olmos and protograph chains' 2-byte rows).
 * ncn = (L + dv - 1) * cns_pos.  Outputs, all ACCUMULATED in place (integer sums: they do not depend on order, batch split,
 * streams or ranks):
 *   d_hist     int64 [nbins]: hist[0] += trials of the call with no member; hist[min(s, nbins - 1)] += 1 per component;
 *   d_pos_hist int64 [L][SCLDPC_SS_POS_SIZES], or NULL: [q][min(s, 8) - 1] += 1 per component, q = j / vns_pos of the
 *              component's lowest-index member j;
 *   d_trial    int32 [ntrials][4], or NULL, OVERWRITTEN per trial: [0] components, [1] largest size, [2] members,
 *              [3] members in components of more than 2 VNs.  Behind a sweep decoder's lost bits [2] and [3] are that
 *              decoder's out[0] and out[1].
 *
 * One 1024-thread workgroup per trial, a lock-free union-find over two int32 arrays, parent[n] and cn_rep[ncn]:
 * scldpc_ss_spectrum_form says where they live, 1 = in LDS beside the member words and the bins, 2 = in the trial's slice of
 * the workspace (the environment variable SCLDPC_DEBUG_SS_FORCE_WORKSPACE=1, read per call, sends every shape there), or the
 * error code (< 0) of an ensemble the entry refuses: dv > 8, or member words, bins and position table beyond one CU's LDS.
 *
 * Workspace: scldpc_ss_spectrum_workspace_bytes(p, ntrials) bytes at a 16-byte aligned address, caller-owned, content on entry
 * irrelevant (needs no device; -1 and a text in scldpc_last_error on bad input).  Its first int32 is the STATUS WORD of the
 * call: the call writes 0 there and the kernel ORs in SCLDPC_SS_BAD_CN where a CN id lay outside [0, ncn): such an edge is
 * skipped, never used as an index, and the caller reads the word after the stream has finished.
 *
 * One kernel launch and a 4-byte memset on `stream`; no allocation, no synchronisation; capturable.  The inputs are only
 * read.  Checks, in this order: the parameters (and the limits above); ntrials >= 0; 2 <= nbins <= SCLDPC_SS_MAX_BINS;
 * adj_kind 0 or 1, adj_kind 1 with vns_pos * dv <= 65535 and an exact multiply-high division (SCLDPC_ERR_BAD_ARG /
 * SCLDPC_ERR_TOO_LARGE); ntrials == 0 is SCLDPC_OK and touches nothing; then null buffers, the alignment and the size of the
 * workspace (SCLDPC_ERR_BAD_ARG). */
int scldpc_ss_spectrum_form(const scldpc_code_params *p);
int64_t scldpc_ss_spectrum_workspace_bytes(const scldpc_code_params *p, int32_t ntrials);
int scldpc_ss_spectrum_device(const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, int32_t adj_kind,
                              const uint32_t *d_member_bits, int32_t nbins, int64_t *d_hist, int64_t *d_pos_hist,
                              int32_t *d_trial, void *d_ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
