/* libscldpc_hip — extension header: the 4-bit sweep decoder for the tail-biting and protograph ensembles.
 *
 * The entries below are exported by the same libscldpc_hip.so as those of scldpc.h, which this header includes; they are
 * declared HERE, not there, because tests/test_buffer_contracts_host.py ties every device entry of scldpc.h to the case table
 * of tests/test_gpu_buffer_contracts.py.  The device entries of this header have a buffer-contract file of their own,
 * tests/test_gpu_buffer_contracts_ens.py (poisoned outputs, red zones, offset views; tests/test_sweep_ens_host.py checks that
 * it covers every one of them), so the rule "every device entry is poison-tested" holds for both headers.
 *
 * Plain C, as scldpc.h.  Error codes, scldpc_last_error and the buffer conventions are that header's. */
#ifndef SCLDPC_ENSEMBLES_H
#define SCLDPC_ENSEMBLES_H

#include "scldpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scldpc_sample_philox_ensemble_device with position-local 2-byte rows and the CN -> socket table of the code, for
 * SCLDPC_ENS_TAIL_BITING and SCLDPC_ENS_PROTOGRAPH (SCLDPC_ENS_OLMOS: SCLDPC_ERR_BAD_ARG, that chain's entry is
 * scldpc_sample_philox_device_adj16_sock).  Same Philox keys; d_chan_bits bit for bit that entry's; for VN j = (q, t) and
 * edge i, d_vn_adj16[j][i] + cpos(q, i) * cns_pos is that entry's d_vn_adj[j][i], with cpos = (q + i) mod L for tail-biting
 * and q + i for protograph.
 * d_cn_sock16 uint16 [ntrials][nk][dc], nk = (L + dv - 1) * cns_pos: the entries of CN (pc, l) other than 0xFFFF are, as a
 * set, { dv * t + i : edge i of VN (pc - i [mod L], t) is CN (pc, l) }; order within a row unspecified.  Tail-biting: every
 * row of positions 0 .. L - 1 is full and every entry of positions L .. L + dv - 2 is 0xFFFF.  Protograph: as a set per CN what
 * scldpc_cn_sockets_device builds from the rows.  Every element of the three buffers is written; no workspace.
 * Limits: those of scldpc_sample_philox_ensemble_device (at most 8192 sockets per position; tail-biting L >= dv; protograph
 * dv | dc), vns_pos * dv <= 65535 and cns_pos <= 65536; SCLDPC_ERR_TOO_LARGE / SCLDPC_ERR_BAD_ARG with the limit named, judged
 * even for ntrials == 0.  scldpc_sample_philox_ensemble_adj16_sock_supported: 1 if (p, ensemble) is taken.  Needs no device. */
int scldpc_sample_philox_ensemble_adj16_sock_supported(const scldpc_code_params *p, int32_t ensemble);
int scldpc_sample_philox_ensemble_device_adj16_sock(const scldpc_code_params *p, int32_t ensemble, uint64_t seed,
                                                    uint64_t trial0, int32_t ntrials, double eps, int32_t ndoped,
                                                    const int32_t *doped_positions, uint16_t *d_vn_adj16,
                                                    uint16_t *d_cn_sock16, uint32_t *d_chan_bits, void *stream);

/* scldpc_peel_sweep_device_sock16 / _sock16_wide on the tables of a TAIL-BITING code (the entry above): edge i of VN position
 * q lies in CN position (q + i) mod L, and socket dv * t + i of a CN of position pc belongs to VN position (pc - i) mod L.
 * Parameters, order of the checks and outputs as those entries; the shape rules are theirs plus L >= dv
 * (scldpc_peel_sweep_tb_supported / _tb_wide_supported, judged at sweep_start = 0; a launch answers L < dv with
 * SCLDPC_ERR_BAD_ARG, as the sampler does, behind the chain's shape rule and before the buffers); error texts start with the
 * entry's name.
 * total_size in [0, nk]: the CNs of positions L .. L + dv - 2 count zero.  d_out columns 0, 1, 2, 7 and d_lost_bits equal
 * scldpc_peel_sweep_device on the int32 rows of the same code bit for bit; [5] rounds, [6] scans after the first, [3] = [4] = 0.
 * (A protograph code is a chain: it runs scldpc_peel_sweep_device_sock16 / _sock16_wide unchanged.) */
int scldpc_peel_sweep_tb_supported(const scldpc_code_params *p);
int scldpc_peel_sweep_tb_wide_supported(const scldpc_code_params *p);
int scldpc_peel_sweep_device_sock16_tb(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                       const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size,
                                       int32_t sweep_start, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                       uint32_t *d_lost_bits, void *stream);
int scldpc_peel_sweep_device_sock16_tb_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                            const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size,
                                            int32_t sweep_start, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                            uint32_t *d_lost_bits, void *stream);

#ifdef __cplusplus
}
#endif

#endif
