// The channel of a trial at every eps at once (include/scldpc_thresh.h): one 31-bit key per VN, the draw the samplers compare with
// the erasure threshold.  The draw is theirs (sampler.hip's channel loop, channel_levels.hip: VN j = 32 w + 4 c + u reads word u of
// philox4x32_10(w * 8 + c, 0x80000000, trial, seed), erased iff (draw >> 1) < thresh), so the bits (key < thresh) are the channel
// words of that threshold.  A VN of a doped position gets 0xFFFFFFFF, above every threshold.  Each thread makes one Philox call
// and writes its four keys with one 16-byte store; there is no LDS and no workspace.
#include "sampler_common.h"
#include "philox.h"
#include "../../include/scldpc_thresh.h"

namespace {

using namespace scldpc_dev;

constexpr int kBlock = 256;

struct KArgs {
    int n, vns_pos, ndoped, ncalls, wide;               // wide: every row is 16-byte aligned and n % 4 == 0
    uint32_t seed_lo, seed_hi;
    unsigned long long trial0;
    uint32_t *keys;
    int doped[scldpc::kMaxDoped];
};

__global__ __launch_bounds__(kBlock) void channel_keys_kernel(const KArgs a)
{
    const int call = blockIdx.x * kBlock + threadIdx.x;             // = w * 8 + c: VNs 4 call .. 4 call + 3
    if (call >= a.ncalls) return;
    const unsigned long long trial = a.trial0 + blockIdx.y;
    uint32_t r[4];
    philox4x32_10((uint32_t)call, 0x80000000u, (uint32_t)trial, (uint32_t)(trial >> 32), a.seed_lo, a.seed_hi, r);
    uint32_t key[4];
#pragma unroll
    for (int u = 0; u < 4; u++) key[u] = r[u] >> 1;
    const int j0 = 4 * call;
    for (int d = 0; d < a.ndoped; d++) {                            // doped positions are never erased (channel_undope's rule)
        const int lo = a.doped[d] * a.vns_pos - j0, hi = lo + a.vns_pos;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (u >= lo && u < hi) key[u] = 0xFFFFFFFFu;
    }
    uint32_t *row = a.keys + (size_t)blockIdx.y * a.n;
    if (a.wide) {
        *reinterpret_cast<uint4 *>(row + j0) = make_uint4(key[0], key[1], key[2], key[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (j0 + u < a.n) row[j0 + u] = key[u];                 // no word at or past n
    }
}

}  // namespace

extern "C" int scldpc_channel_keys_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
                                          int32_t ndoped, const int32_t *doped_positions, uint32_t *d_keys, void *stream)
{
    using namespace scldpc;
    static const char *who = "scldpc_channel_keys_device";
    if (int rc = check_params(p)) return rc;
    if (ntrials < 0 || (ntrials > 0 && !d_keys))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer or negative ntrials", who);
    if (ndoped < 0 || ndoped > kMaxDoped || (ndoped > 0 && !doped_positions))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 0 <= ndoped <= %d", who, kMaxDoped);
    if (ntrials == 0) return SCLDPC_OK;
    KArgs a{};
    for (int d = 0; d < ndoped; d++) {
        if (doped_positions[d] < 0 || doped_positions[d] >= p->L)
            return set_error(SCLDPC_ERR_BAD_ARG, "doped position %d outside [0,%d)", doped_positions[d], p->L);
        a.doped[d] = doped_positions[d];
    }
    a.n = n_of(p); a.vns_pos = p->vns_pos; a.ndoped = ndoped;
    a.ncalls = (a.n + 3) / 4;
    a.wide = (a.n & 3) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.keys = d_keys;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kMaxGridY = 65535;                                // trials ride on blockIdx.y
    for (int32_t t0 = 0; t0 < ntrials; t0 += kMaxGridY) {
        const int nt = ntrials - t0 < kMaxGridY ? ntrials - t0 : kMaxGridY;
        KArgs b = a;
        b.trial0 = trial0 + (uint64_t)t0;
        b.keys = d_keys + (size_t)t0 * a.n;
        hipLaunchKernelGGL(channel_keys_kernel, dim3((a.ncalls + kBlock - 1) / kBlock, nt), dim3(kBlock), 0, st, b);
        SCLDPC_HIP_CHECK(hipGetLastError());
    }
    return SCLDPC_OK;
}
