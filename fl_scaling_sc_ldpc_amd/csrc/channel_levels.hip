// The channel of a trial at every point of a descending eps grid (include/scldpc_eps.h): one byte per VN, the number of
// points at which the VN is erased.  The draw is the samplers' (sampler.hip's channel loop: VN j = 32 w + 4 c + u reads word u of
// philox4x32_10(w * 8 + c, 0x80000000, trial, seed), erased iff (draw >> 1) < thresh), so the bits (lev > k) are the channel
// words of point k.  Each thread makes one Philox call and writes its four level bytes with one 4-byte store; the thresholds
// travel in the kernel argument (uniform loads), there is no LDS and no workspace.
#include "sampler_common.h"
#include "philox.h"
#include "../../include/scldpc_eps.h"

namespace {

using namespace scldpc_dev;

constexpr int kBlock = 256;

struct LArgs {
    int n, vns_pos, npoints, ndoped, ncalls, wide;      // wide: every row is 4-byte aligned and n % 4 == 0
    uint32_t seed_lo, seed_hi;
    unsigned long long trial0;
    uint8_t *levels;
    uint32_t thresh[SCLDPC_EPS_MAX_POINTS];
    int doped[scldpc::kMaxDoped];
};

__global__ __launch_bounds__(kBlock) void channel_levels_kernel(const LArgs a)
{
    const int call = blockIdx.x * kBlock + threadIdx.x;             // = w * 8 + c: VNs 4 call .. 4 call + 3
    if (call >= a.ncalls) return;
    const unsigned long long trial = a.trial0 + blockIdx.y;
    uint32_t r[4];
    philox4x32_10((uint32_t)call, 0x80000000u, (uint32_t)trial, (uint32_t)(trial >> 32), a.seed_lo, a.seed_hi, r);
    uint32_t lev[4] = {0, 0, 0, 0};
    for (int k = 0; k < a.npoints; k++) {
        const uint32_t th = a.thresh[k];
#pragma unroll
        for (int u = 0; u < 4; u++) lev[u] += channel_erased(r[u], th);
    }
    const int j0 = 4 * call;
    for (int d = 0; d < a.ndoped; d++) {                            // doped positions are never erased (channel_undope's rule)
        const int lo = a.doped[d] * a.vns_pos - j0, hi = lo + a.vns_pos;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (u >= lo && u < hi) lev[u] = 0;
    }
    uint8_t *row = a.levels + (size_t)blockIdx.y * a.n;
    if (a.wide) {
        *reinterpret_cast<uint32_t *>(row + j0) = lev[0] | (lev[1] << 8) | (lev[2] << 16) | (lev[3] << 24);
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (j0 + u < a.n) row[j0 + u] = (uint8_t)lev[u];       // no byte at or past n
    }
}

}  // namespace

extern "C" int scldpc_channel_levels_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
                                            int32_t npoints, const double *eps, int32_t ndoped, const int32_t *doped_positions,
                                            uint8_t *d_levels, void *stream)
{
    using namespace scldpc;
    static const char *who = "scldpc_channel_levels_device";
    if (int rc = check_params(p)) return rc;
    if (ntrials < 0 || (ntrials > 0 && !d_levels))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer or negative ntrials", who);
    if (ndoped < 0 || ndoped > kMaxDoped || (ndoped > 0 && !doped_positions))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 0 <= ndoped <= %d", who, kMaxDoped);
    if (npoints < 1 || npoints > SCLDPC_EPS_MAX_POINTS || !eps)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 1 <= npoints <= %d and a non-null eps (got npoints = %d)", who,
                         SCLDPC_EPS_MAX_POINTS, npoints);
    LArgs a{};
    for (int k = 0; k < npoints; k++) {
        if (!(eps[k] >= 0.0 && eps[k] <= 1.0))
            return set_error(SCLDPC_ERR_BAD_ARG, "%s: eps[%d]=%g outside [0,1]", who, k, eps[k]);
        a.thresh[k] = erasure_threshold(eps[k]);
        if (k > 0 && a.thresh[k] >= a.thresh[k - 1])
            return set_error(SCLDPC_ERR_BAD_ARG, "%s: the thresholds must be strictly decreasing (eps[%d]=%.17g after eps[%d]=%.17g)",
                             who, k, eps[k], k - 1, eps[k - 1]);
    }
    if (ntrials == 0) return SCLDPC_OK;
    for (int d = 0; d < ndoped; d++) {
        if (doped_positions[d] < 0 || doped_positions[d] >= p->L)
            return set_error(SCLDPC_ERR_BAD_ARG, "doped position %d outside [0,%d)", doped_positions[d], p->L);
        a.doped[d] = doped_positions[d];
    }
    a.n = n_of(p); a.vns_pos = p->vns_pos; a.npoints = npoints; a.ndoped = ndoped;
    a.ncalls = (a.n + 3) / 4;
    a.wide = (a.n & 3) == 0 && (reinterpret_cast<uintptr_t>(d_levels) & 3) == 0;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.levels = d_levels;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kMaxGridY = 65535;                                // trials ride on blockIdx.y
    for (int32_t t0 = 0; t0 < ntrials; t0 += kMaxGridY) {
        const int nt = ntrials - t0 < kMaxGridY ? ntrials - t0 : kMaxGridY;
        LArgs b = a;
        b.trial0 = trial0 + (uint64_t)t0;
        b.levels = d_levels + (size_t)t0 * a.n;
        hipLaunchKernelGGL(channel_levels_kernel, dim3((a.ncalls + kBlock - 1) / kBlock, nt), dim3(kBlock), 0, st, b);
        SCLDPC_HIP_CHECK(hipGetLastError());
    }
    return SCLDPC_OK;
}
