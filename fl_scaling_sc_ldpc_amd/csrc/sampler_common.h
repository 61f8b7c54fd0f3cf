// What the Philox samplers share (sampler.hip, sampler_v2.hip, sampler_v2_deg.hip, sampler_v2_wide.hip): on the device the steps of a channel word,
// the histogram words of a thread, the exclusive scan of the bucket counts, the two-calls-per-thread look-up and the worklist's
// resolve loop; on the host the erasure threshold, the validation of a sampling call and the second generation's LDS layout.
// Every device function is inlined into its kernel, and cut so that the kernels' code stays what it was when each carried its
// own copy (profiles/sampler_common_static.txt has the comparison).
#pragma once
#include "common.h"
#include "kernel_util.h"
#include <algorithm>
#include <cstdlib>

namespace scldpc {

constexpr int kSamplerThreads = 1024;           // one workgroup samples one trial
constexpr int kSamplerWaves = kSamplerThreads / 64;
constexpr int kMaxDoped = 32;
constexpr int kWorkCap = 1024;                  // second generation: keys of buckets that span two CNs, per position

}  // namespace scldpc

namespace scldpc_dev {

// ---- channel: word w holds the erasure bits of VNs j0 = 32 w .. 32 w + 31, four to a Philox draw.  Here are the three rules of
//      a word, on plain values and without a loop — NOT the whole channel: the loop over the eight draws of a word and the
//      placing of their bits (<< (c * 4 + u)) stand in each of the five kernels, as does the loop over a.doped[], and a change to
//      how a draw is obtained or packed touches all five.  (A helper that holds the eight draws, or the four compares of one, is
//      unrolled before it is inlined and the kernel's reassociation pass regroups the ORs: 50 -> 69 VGPRs in
//      sample_philox_kernel; one that takes the kernel's argument struct by reference costs 4 to 15 VGPRs there as well:
//      profiles/sampler_common_static.txt, sampler_common_ab.txt.)
// the VN of this draw is erased
__device__ __forceinline__ uint32_t channel_erased(uint32_t draw, uint32_t thresh) { return (uint32_t)((draw >> 1) < thresh); }
// no bit at or past n
__device__ __forceinline__ uint32_t channel_tail(uint32_t word, int j0, int n)
{
    if (j0 + 32 > n) word &= (1u << (n - j0)) - 1u;
    return word;
}
// doped positions are never erased (BPF:1566-1573)
__device__ __forceinline__ uint32_t channel_undope(uint32_t word, int j0, int pos, int vns_pos)
{
    const int lo = max(pos * vns_pos, j0) - j0, hi = min((pos + 1) * vns_pos, j0 + 32) - j0;
    if (lo < hi) word &= ~(((hi - lo) == 32 ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u)) << lo);
    return word;
}

// ---- the histogram words of a thread: thread t owns words t*ROWS .. t*ROWS+ROWS-1 of four nibble-wide bucket counters each
//      (wide LDS accesses)
__device__ __forceinline__ uint32_t nib_sum(uint32_t x)                 // sum of the four nibbles of the low half
{
    const uint32_t v = (x & 0x0F0Fu) + ((x >> 4) & 0x0F0Fu);
    return (v + (v >> 8)) & 0xFFu;
}

template <int ROWS>
__device__ __forceinline__ void load_hist_words(const uint32_t *hist, int tid, uint32_t (&x)[ROWS])
{
    if constexpr (ROWS % 4 == 0) {
#pragma unroll
        for (int r = 0; r < ROWS / 4; r++) {
            const uint4 q = reinterpret_cast<const uint4 *>(hist)[tid * (ROWS / 4) + r];
            x[4 * r] = q.x; x[4 * r + 1] = q.y; x[4 * r + 2] = q.z; x[4 * r + 3] = q.w;
        }
    } else if constexpr (ROWS == 2) { const uint2 q = reinterpret_cast<const uint2 *>(hist)[tid]; x[0] = q.x; x[1] = q.y; }
    else { static_assert(ROWS == 1, "ROWS is 1, 2 or a multiple of 4"); x[0] = hist[tid]; }
}

template <int ROWS>
__device__ __forceinline__ void store_hist_words(uint32_t *hist, int tid, const uint32_t (&x)[ROWS])
{
    if constexpr (ROWS % 4 == 0) {
#pragma unroll
        for (int r = 0; r < ROWS / 4; r++)
            reinterpret_cast<uint4 *>(hist)[tid * (ROWS / 4) + r] = make_uint4(x[4 * r], x[4 * r + 1], x[4 * r + 2], x[4 * r + 3]);
    } else if constexpr (ROWS == 2) reinterpret_cast<uint2 *>(hist)[tid] = make_uint2(x[0], x[1]);
    else hist[tid] = x[0];
}

template <int ROWS>
__device__ __forceinline__ void clear_hist_words(uint32_t *hist, int tid)
{
    uint32_t z[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) z[r] = 0;
    store_hist_words<ROWS>(hist, tid, z);
}

// ---- exclusive scan of the bucket counts (second generation): every thread scans its ROWS words, the wave scans the thread
//      totals (DPP), the 16 wave totals meet in wsum; the global prefix goes into the words' high halves.
// hist word while counting = [0:16 | n3:4 | n2:4 | n1:4 | n0:4]: four nibble-wide bucket counters (the atomic's return value
// is the key's arrival slot).  After the scan:
//   INCL:  [exclusive prefix:12 | i3:4 | i2:4 | i1:4 | i0:4 | 0:4] with ik = n0 + .. + nk, so bucket k's ranks are
//          [prefix + (word >> 4k & 15), prefix + (word >> 4k+4 & 15)) — valid while the word holds at most 15 keys;
//   else:  [exclusive prefix:16 | n3 n2 n1 n0], the lower buckets' counts summed at look-up time.
// Two barriers: between the wave totals' write and their read, and behind the write-back.  Returns whether the histogram's
// ranks hold (else the caller's exact fallback ranks the position).  INCL: a word of more than 15 keys, which includes a
// wrapped nibble, makes that word's scanned total smaller than its true count, so the grand total falls short of S: one
// uniform compare for the whole position.  Else: the flag wsum[kWaves + 1], raised by a thread that saw a full nibble.
template <int ROWS, bool INCL>
__device__ __forceinline__ bool scan_hist(uint32_t *hist, uint32_t *wsum, int tid, int lane, int wave, int S)
{
    constexpr int kWaves = scldpc::kSamplerWaves;
    bool ranked = true;
    if constexpr (INCL) {
        // one multiply per word: nibble k+1 of x * 0x111110 is n0 + .. + nk, nibble 5 the word's total again (no carries
        // while the word holds at most 15 keys; else nibble 5 is below the true count and the grand total shows it)
        uint32_t x[ROWS], t20[ROWS], tot20 = 0;
        load_hist_words<ROWS>(hist, tid, x);
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            x[r] *= 0x111110u;
            t20[r] = x[r] & 0xF00000u;                                  // the word's total << 20
            tot20 += t20[r];
        }
        const uint32_t tot = tot20 >> 20, inc = wave_inclusive_scan(tot);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t winc = lane < kWaves ? wsum[lane] : 0u;              // the 16 wave totals: a scan within DPP row 0
        const uint32_t wt = winc;
        winc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)winc, 0x111, 0xF, 0xF, false);
        winc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)winc, 0x112, 0xF, 0xF, false);
        winc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)winc, 0x114, 0xF, 0xF, false);
        winc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)winc, 0x118, 0xF, 0xF, false);
        ranked = __builtin_amdgcn_readlane((int)winc, kWaves - 1) == S;
        uint32_t pre20 = (inc - tot + (uint32_t)__builtin_amdgcn_readlane((int)(winc - wt), wave)) << 20;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            x[r] = (x[r] & 0xFFFF0u) | pre20;
            pre20 += t20[r];
        }
        store_hist_words<ROWS>(hist, tid, x);
    } else {
        uint32_t x[ROWS], v[ROWS], tot = 0;
        load_hist_words<ROWS>(hist, tid, x);
#pragma unroll
        for (int r = 0; r < ROWS; r++) v[r] = 0;
        if constexpr (ROWS % 2 == 0) {                                  // two words' counters (16 bits each) per 32-bit lane
#pragma unroll
            for (int r = 0; r < ROWS; r += 2) {
                const uint32_t y = x[r] | (x[r + 1] << 16);
                const uint32_t sb = (y & 0x0F0F0F0Fu) + ((y >> 4) & 0x0F0F0F0Fu);      // four byte sums <= 30
                v[r] = (sb & 0xFFu) + ((sb >> 8) & 0xFFu);
                v[r + 1] = ((sb >> 16) & 0xFFu) + (sb >> 24);
                tot += v[r] + v[r + 1];
            }
        } else {
            static_assert(ROWS == 1 || ROWS % 2 == 0, "ROWS is 1, 2, 4 or 8");
            v[0] = nib_sum(x[0]);
            tot = v[0];
        }
        const uint32_t inc = wave_inclusive_scan(tot);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        const uint32_t wt = lane < kWaves ? wsum[lane] : 0u;
        const uint32_t winc = wave_inclusive_scan(wt);
        uint32_t pre = inc - tot + (uint32_t)__builtin_amdgcn_readlane((int)(winc - wt), wave);
#pragma unroll
        for (int r = 0; r < ROWS; r++) { x[r] |= pre << 16; pre += v[r]; }
        store_hist_words<ROWS>(hist, tid, x);
    }
    __syncthreads();
    if constexpr (!INCL) ranked = wsum[kWaves + 1] == 0u;
    return ranked;
}

// ---- two calls per thread (the exclusive form of the scanned word): first rank g0 and end rank g1 of every key's bucket.
//      live(e): key e stands for a socket (the others read word 0 and are masked by the caller).
template <int KSHIFT, int E, class Live>
__device__ __forceinline__ void bucket_ranges_excl(const uint32_t *hist, const uint32_t (&key)[E], Live &&live,
                                                   uint32_t (&g0a)[E], uint32_t (&g1a)[E])
{
    uint32_t h[E];
#pragma unroll
    for (int e = 0; e < E; e++) h[e] = hist[live(e) ? (key[e] >> KSHIFT) >> 2 : 0u];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t k4 = ((key[e] >> KSHIFT) & 3u) * 4u, x = h[e];
        const uint32_t below = x & ((1u << k4) - 1u);                    // the counters of the word's lower buckets
        g0a[e] = (x >> 16) + (below & 0xFu) + ((below >> 4) & 0xFu) + ((below >> 8) & 0xFu);
        g1a[e] = g0a[e] + ((x >> k4) & 0xFu);
    }
}

// ---- the worklist: a straddler's true rank is its bucket's first rank + the mates below it.  entry(socket) is what the
//      rank-ordered stage holds for a socket (STAGE: a table goes out), cn_of(rank) the CN of a rank.
template <int LG, bool STAGE, class Entry, class CnOf>
__device__ __forceinline__ void resolve_worklist(int nwork, int tid, const uint32_t *wl, const uint32_t *gpk, uint16_t *stage,
                                                 uint16_t *fix, Entry &&entry, CnOf &&cn_of)
{
    for (int w = tid; w < nwork; w += scldpc::kSamplerThreads) {
        const uint32_t ea = wl[2 * w], pk = wl[2 * w + 1];
        uint32_t r = ea & 0xFFFFu;
#pragma unroll 1
        for (uint32_t m = ea & 0xFFFFu; m < (ea >> 16); m++) r += gpk[m] < pk;     // (itself included: not below)
        const uint32_t sck = pk & ((1u << LG) - 1u);
        if constexpr (STAGE) stage[r] = entry(sck);
        fix[sck] = (uint16_t)cn_of(r);
    }
}

}  // namespace scldpc_dev

namespace scldpc {

// erased iff r/RAND_MAX < eps with r = 31-bit draw  ⇔  r < ceil(eps * RAND_MAX)   (BPF:370,1554-1562)
inline uint32_t erasure_threshold(double eps)
{
    const double x = eps * 2147483647.0;
    double c = (double)(uint64_t)x;
    if (c < x) c += 1.0;
    return (uint32_t)c;
}

// The arguments every sampling launch takes.  bad_buffers: ntrials is negative or a buffer the launch writes is null.
// With trials to sample, the doped positions are checked against [0, L) and copied to a_doped.  0 or SCLDPC_ERR_BAD_ARG.
inline int check_sample_call(const char *who, const scldpc_code_params *p, bool bad_buffers, int32_t ntrials, double eps,
                             int32_t ndoped, const int32_t *doped_positions, int *a_ndoped, int (&a_doped)[kMaxDoped])
{
    if (bad_buffers)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer or negative ntrials", who);
    if (ndoped < 0 || ndoped > kMaxDoped || (ndoped > 0 && !doped_positions))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 0 <= ndoped <= %d", who, kMaxDoped);
    if (!(eps >= 0.0 && eps <= 1.0))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: eps=%g outside [0,1]", who, eps);
    if (ntrials <= 0) return SCLDPC_OK;
    *a_ndoped = ndoped;
    for (int d = 0; d < ndoped; d++) {
        if (doped_positions[d] < 0 || doped_positions[d] >= p->L)
            return set_error(SCLDPC_ERR_BAD_ARG, "doped position %d outside [0,%d)", doped_positions[d], p->L);
        a_doped[d] = doped_positions[d];
    }
    return SCLDPC_OK;
}

// LDS of a second-generation workgroup, in 32-bit words: hist_bufs histograms of nb words (nb = 1 << *lg = power of two >=
// max(S, kSamplerThreads): the histogram of sampler.hip), then the packed keys, the CN ids, the stage (with a table) and the wave
// totals with the worklist behind them.  Sets a->nb, the four offsets and a->force_exact (SCLDPC_DEBUG_SAMPLER_EXACT_POS:
// diagnostics / tests only, else -1), *lg and *bytes.  hist_bufs: 2 for the third generation's double buffer.  by_nb: the
// regions behind the histogram are sized for nb sockets rather than S (sampler_v2.hip's one-call instances address them by
// V2Layout's immediates).
template <class Args>
inline int v2_lds_layout(const char *who, int S, int hist_bufs, bool by_nb, bool stage, Args *a, int *lg, size_t *bytes)
{
    *lg = 10;
    while ((1 << *lg) < S) ++*lg;
    a->nb = 1 << *lg;
    const int s_lay = by_nb ? a->nb : S;
    int off = (hist_bufs * a->nb + 3) & ~3;
    a->off_gpk = off;   off += (s_lay + 3) & ~3;
    a->off_fix = off;   off += (s_lay / 2 + 3) & ~3;        // S uint16 (S % 4 == 2: and the two dead ids of the last call)
    a->off_stage = off; off += stage ? (s_lay / 2 + 3) & ~3 : 0;
    a->off_wsum = off;  off += 32 + 2 * kWorkCap;
    *bytes = 4u * (size_t)off;
    *bytes = std::min(*bytes + debug_lds_pad("SAMPLER"), std::max(*bytes, (size_t)kMaxLdsBytes));
    if (*bytes > (size_t)kMaxLdsBytes)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: %zu bytes of LDS per trial", who, *bytes);
    a->force_exact = -1;
    if (const char *v = getenv("SCLDPC_DEBUG_SAMPLER_EXACT_POS")) a->force_exact = atoi(v);
    return SCLDPC_OK;
}

// LDS of the wide second generation (sampler_v2_wide.hip, more than 8192 sockets per position), which ranks a position in one
// part (up to kWidePartCap sockets) or in two, by the top key bit: one histogram of kWideHistWords words over the next 15 key
// bits and the packed keys of one part (kWidePartCap entries, by part-local rank) — the two lie side by side and together hold
// the S keys of the exact fallback — then the stage of one part, the S CN ids of the position and two sets of wave totals,
// worklist counter and overflow flag (parts alternate between them, 32 words each) with the worklist behind them.  Sets the
// offsets, a->force_exact as above and a->part_cap (SCLDPC_DEBUG_SAMPLER_PART_CAP lowers it: diagnostics / tests only).
constexpr int kWideHistWords = 8192;
constexpr int kWidePartCap = 12288;
constexpr int kWideMaxSockets = kWideHistWords + kWidePartCap;  // the exact fallback's keys: histogram + packed keys

template <class Args>
inline int v2_wide_lds_layout(const char *who, int S, Args *a, size_t *bytes)
{
    int off = kWideHistWords;                                   // the histogram at word 0
    a->off_gpk = off;   off += kWidePartCap;
    a->off_stage = off; off += kWidePartCap / 2;
    a->off_fix = off;   off += (S / 2 + 3) & ~3;
    a->off_wsum = off;  off += 64 + 2 * kWorkCap;
    *bytes = 4u * (size_t)off;
    *bytes = std::min(*bytes + debug_lds_pad("SAMPLER"), std::max(*bytes, (size_t)kMaxLdsBytes));
    if (S > kWideMaxSockets || *bytes > (size_t)kMaxLdsBytes)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: %zu bytes of LDS per trial", who, *bytes);
    a->force_exact = -1;
    if (const char *v = getenv("SCLDPC_DEBUG_SAMPLER_EXACT_POS")) a->force_exact = atoi(v);
    a->part_cap = kWidePartCap;
    if (const char *v = getenv("SCLDPC_DEBUG_SAMPLER_PART_CAP")) a->part_cap = std::min(kWidePartCap, std::max(0, atoi(v)));
    return SCLDPC_OK;
}

}  // namespace scldpc
