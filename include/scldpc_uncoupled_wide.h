/* libscldpc_hip — extension header: the rejection sampler of the uncoupled (dv, dc) ensemble up to 32 768 sockets.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h and scldpc_uncoupled.h, which this header
 * includes; they are declared HERE for the reason scldpc_uncoupled.h gives: tests/test_uncoupled_host.py ties that header to
 * its two symbols and its size refusal.  The device entry of this header has a buffer-contract file of its own,
 * tests/test_gpu_buffer_contracts_unc_wide.py (poisoned outputs, red zones, offset views; it checks that it covers every device
 * entry declared here).
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_UNCOUPLED_WIDE_H
#define SCLDPC_UNCOUPLED_WIDE_H

#include "scldpc_uncoupled.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The law, the keys, the parameters, the three buffers and the status conventions of scldpc_sample_philox_uncoupled_device
 * (scldpc_uncoupled.h), for p = (dv, dc, 1, cns_pos, vns_pos) with up to 32 768 sockets: candidate a of trial t is what the
 * tail-biting sampler draws at L = 1 under trial' = t + (a << 40), sockets ranked by (key, socket), CN = rank / dc, the first
 * candidate in which no row holds a CN twice is the graph, its channel words those of the same trial', d_attempts[t] = a + 1.
 * On every shape both entries take, the three outputs of the two are bit-identical; results do not depend on how a run is cut
 * into calls.
 * A trial without an accepted candidate within max_attempts gets d_attempts[t] = 0.  Beyond 16 384 sockets the keys are ranked in
 * four parts by their two top bits, and a part of more than 12 288 keys (never, on Philox keys: the mean is at most 8192 and the
 * tail below exp(-819)) gives d_attempts[t] = -1; the rows and channel words of both are zeros.  The call itself returns
 * SCLDPC_OK either way: the caller reads d_attempts.
 *
 * d_vn_adj int32 [ntrials][vns_pos][dv], ids < cns_pos; d_chan_bits uint32 [ntrials][nw]; d_attempts int32 [ntrials].  Every
 * element of the three buffers is written.  No workspace, no allocation, no synchronisation; capturable.
 * Checks, in this order and the first four even for ntrials == 0: valid parameters; L == 1 (SCLDPC_ERR_BAD_ARG); dv <= 8 and
 * cns_pos * dc <= 32768 (SCLDPC_ERR_TOO_LARGE); dv <= cns_pos, else no simple graph exists (SCLDPC_ERR_BAD_ARG) — this is the
 * shape rule, and scldpc_sample_philox_uncoupled_wide_supported returns 1 where it passes and 0 with the limit named in
 * scldpc_last_error() where it does not (needs no device).  Then eps in [0, 1], 1 <= max_attempts <= 2^24,
 * trial0 + ntrials <= 2^40 and ntrials >= 0 (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; then null buffers
 * (SCLDPC_ERR_BAD_ARG). */
int scldpc_sample_philox_uncoupled_wide_supported(const scldpc_code_params *p);
int scldpc_sample_philox_uncoupled_wide_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
                                               double eps, int32_t max_attempts, int32_t *d_vn_adj, uint32_t *d_chan_bits,
                                               int32_t *d_attempts, void *stream);

#ifdef __cplusplus
}
#endif

#endif
