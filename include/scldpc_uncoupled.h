/* libscldpc_hip — extension header: the rejection sampler of the uncoupled (dv, dc) ensemble.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, which this header includes; they are
 * declared HERE, not there, for the reason scldpc_ensembles.h gives: tests/test_buffer_contracts_host.py and
 * tests/test_sweep_ens_host.py tie every device entry of the two other headers to their contract tables.  The device entry
 * of this header has a buffer-contract file of its own, tests/test_gpu_buffer_contracts_unc.py (poisoned outputs, red zones,
 * offset views; it checks that it covers every device entry declared here).
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_UNCOUPLED_H
#define SCLDPC_UNCOUPLED_H

#include "scldpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The uncoupled (dv, dc) ensemble of ldpc.gen_slots (ldpc.py:45-84, PD:134-135) in throughput mode: one uniformly random
 * permutation of the dv * vns_pos sockets, socket dv * t + i wired to edge i of VN t, CN = rank / dc, REDRAWN until no VN
 * meets a CN twice — and the channel of the accepted draw.  p = (dv, dc, 1, cns_pos, vns_pos): one position, L = 1.
 *
 * The law and the keys.  Trial t = trial0 + (index in the batch) tries attempts a = 0, 1, 2, ...  Candidate a is what
 * scldpc_sample_philox_ensemble_device would draw for SCLDPC_ENS_TAIL_BITING at L = 1 under trial' = t + (a << 40) (that
 * entry itself refuses L < dv): Philox4x32-10 keys with counter (s >> 2, 0, trial', trial' >> 32), word s & 3 the key of
 * socket s; rank by (key, socket); CN = rank / dc; row t = the CNs of sockets dv * t .. dv * t + dv - 1.  The trial's graph is
 * the FIRST candidate in which no row holds a CN twice, its channel words those of the same trial' (stream 2^31 and the
 * threshold of every sampler; the channel keys are independent of the graph keys, so acceptance does not bias them), and
 * d_attempts[t] = a + 1.  Results do not depend on how a run is cut into calls.
 * A trial without an accepted candidate within max_attempts gets d_attempts[t] = 0, and one in which sixteen keys met in one
 * counting bucket (never, on Philox keys) gets -1; the rows and channel words of both are zeros.  The call itself returns
 * SCLDPC_OK either way: the caller reads d_attempts.
 *
 * d_vn_adj int32 [ntrials][vns_pos][dv], ids < cns_pos; d_chan_bits uint32 [ntrials][nw]; d_attempts int32 [ntrials].  Every
 * element of the three buffers is written.  No workspace, no allocation, no synchronisation; capturable.
 * Checks, in this order and the first four even for ntrials == 0: valid parameters; L == 1 (SCLDPC_ERR_BAD_ARG); dv <= 8 and
 * cns_pos * dc <= 8192 (SCLDPC_ERR_TOO_LARGE); dv <= cns_pos, else no simple graph exists (SCLDPC_ERR_BAD_ARG) — this is the
 * shape rule, and scldpc_sample_philox_uncoupled_supported returns 1 where it passes and 0 with the limit named in
 * scldpc_last_error() where it does not (needs no device).  Then eps in [0, 1], 1 <= max_attempts <= 2^24,
 * trial0 + ntrials <= 2^40 and ntrials >= 0 (SCLDPC_ERR_BAD_ARG); ntrials == 0 is SCLDPC_OK; then null buffers
 * (SCLDPC_ERR_BAD_ARG). */
int scldpc_sample_philox_uncoupled_supported(const scldpc_code_params *p);
int scldpc_sample_philox_uncoupled_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
                                          double eps, int32_t max_attempts, int32_t *d_vn_adj, uint32_t *d_chan_bits,
                                          int32_t *d_attempts, void *stream);

#ifdef __cplusplus
}
#endif

#endif
