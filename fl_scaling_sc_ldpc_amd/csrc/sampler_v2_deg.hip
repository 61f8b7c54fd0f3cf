// Second-generation sampler for the degree pairs (3,6) and (5,10) (gfx950): sampler_v2.hip's ranking — a key histogram whose
// buckets give the CN of every key they hold unless they straddle a multiple of dc, a worklist for the few keys that do, the
// CN -> socket table as the inverse of the ranking — with the two things that file ties to dv = 4, dc = 8 set free:
//
//  * rank / dc is a multiply and a shift by compile-time constants (ranks are below 8192: checked below over all of them),
//    and a bucket [g0, g1) straddles when g0 / dc != (g1 - 1) / dc.
//  * Socket s = dv*t + i of CN position q + i is edge i of VN (q, t) (BPF:1712), but a Philox call still draws the keys of four
//    consecutive sockets: the thread that classifies a socket is no longer the thread that holds its VN.  Behind the barrier
//    that ends the worklist the VN-owner thread t (and t + 1024, ...) reads this position's CN ids fix[dv*t + i], i < dv, from
//    LDS, keeps the dv (dv - 1) / 2 ids of the dv - 1 VN positions still waiting for edges in registers and stores VN position
//    p - dv + 1 as whole rows of dv ids.  (A ring of dv fix arrays, as sampler.hip keeps, would not fit beside the histogram,
//    the packed keys and the stage at (5,10) with 8190 sockets.)
//
// S = cns_pos * dc is even but need not be a multiple of four: the last Philox call then owns two live sockets.  Its dead words
// add nothing to the histogram, are never classified or staged, and nothing is stored past S; the table's S entries per
// position go out as 32-bit words.
// Same law, same keys (word s & 3 of philox4x32_10(s >> 2, p, trial, seed)), rank by key, ties by socket: vn_adj16 and the
// channel words are bit for bit scldpc_sample_philox_device_adj16's, the table is scldpc_cn_sockets_device's as a set per CN.
//
// What is sampler_v2.hip's line for line lives in sampler_common.h: the histogram words of a thread, the scan, the
// two-calls-per-thread look-up, the worklist's resolve loop, the steps of a channel word, and on the host the validation, the
// threshold and the LDS layout.  Here stay rank / dc, the worklist pushes, the exact fallback, the pend queues, edge_of /
// stage_own and the table's copy-out.
#include "sampler_common.h"
#include "philox.h"

namespace {

using scldpc_dev::philox4x32_10;

constexpr int kThreads = scldpc::kSamplerThreads;
constexpr int kWaves = kThreads / 64;
using scldpc::kMaxDoped;
using scldpc::kWorkCap;                 // keys of buckets that span two CNs, per position
constexpr int kMaxSockets = 8192;       // per CN position: two Philox calls per thread

struct SDArgs {
    int L, cns_pos, vns_pos, n, S, D, nb, nw;
    int force_exact;                    // diagnostics: rank this CN position by the exact fallback (-1: none, -2: every position)
    int tabw;                           // bytes per store of the table's copy-out: 8 (S % 4 == 0), 4 or 2 (by the table's alignment)
    int ndoped;
    int doped[kMaxDoped];
    uint32_t seed_lo, seed_hi;
    unsigned long long trial0;
    uint32_t thresh;                    // erased iff (draw >> 1) < thresh
    int off_gpk, off_fix, off_stage, off_wsum;      // LDS offsets in 32-bit words
    uint16_t *vn_adj16;                 // uint16 [T][n][dv], CN index local to its position
    uint16_t *cn_sock16;                // uint16 [T][D*cns_pos][dc] sockets of every CN (0xFFFF: its VN position is off the chain), or null
    uint32_t *chan;
};

// x / D for x < 8192 (ranks and sockets) as one 24-bit multiply and a shift
template <int D> constexpr uint32_t small_magic() { return (65536u + D - 1) / D; }
template <int D> constexpr bool small_div_exact()
{
    for (uint32_t x = 0; x < (uint32_t)kMaxSockets; x++)
        if (((x * small_magic<D>()) >> 16) != x / D) return false;
    return true;
}
static_assert(small_div_exact<3>() && small_div_exact<5>() && small_div_exact<6>() && small_div_exact<10>(),
              "the multiply-and-shift division holds for every rank and socket below 8192");
template <int D> __device__ __forceinline__ uint32_t small_div(uint32_t x) { return __umul24(x, small_magic<D>()) >> 16; }

// KMAX = Philox calls (4 sockets each) per thread and position: 1 up to 4096 sockets per position, 2 up to 8192
// ROWS = histogram words per thread (nb / 1024)
// CNMODE: 0 no table, 2 the rank-ordered stage holds the sockets themselves (the table the _deg decoders and sw_ring read)
template <int DV, int DC, int KMAX, int ROWS, int CNMODE>
__global__ __launch_bounds__(kThreads, KMAX == 1 ? 8 : 4) __attribute__((amdgpu_num_sgpr(72))) void sample_philox_v2_deg_kernel(const SDArgs a)
{
    static_assert((DV == 3 && DC == 6) || (DV == 5 && DC == 10), "the pairs (3,6) and (5,10)");
    static_assert(CNMODE == 0 || CNMODE == 2, "no table or the CN -> socket table");
    constexpr int E = 4 * KMAX;
    constexpr int VMAX = (4096 * KMAX / DV + kThreads - 1) / kThreads;  // VNs per thread: vns_pos = S / DV <= 4096 KMAX / DV
    constexpr int LG = ROWS == 1 ? 10 : ROWS == 2 ? 11 : ROWS == 4 ? 12 : 13;        // log2(nb) = socket bits
    constexpr int KSHIFT = 32 - LG - 2;                                 // key >> KSHIFT = fine bucket
    // one call per thread: inclusive nibble prefixes in the scanned word and one overflow test per position (sampler_v2.hip)
    constexpr bool INCL = KMAX == 1;
    static_assert(ROWS * kThreads == (1 << LG) && (INCL ? ROWS <= 4 : ROWS == 8), "ROWS is 1, 2, 4 (KMAX 1) or 8 (KMAX 2)");
    extern __shared__ uint32_t lds[];
    uint32_t *hist = lds;                                               // nb words of four nibble-wide bucket counters
    uint32_t *gpk = lds + a.off_gpk;                                    // S words: packed keys of straddling buckets
    uint16_t *fix = reinterpret_cast<uint16_t *>(lds + a.off_fix);      // S CN-local ids of this position's sockets
    uint16_t *stage = reinterpret_cast<uint16_t *>(lds + a.off_stage);  // the S sockets in rank order
    uint32_t *wsum = lds + a.off_wsum;                                  // 16 wave totals + the worklist counter
    uint32_t *wl = wsum + 32;                                           // worklist: 2 words per key of a straddling bucket

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, nb = a.nb;
    // call k of this thread draws sockets 4*(tid + 1024 k) .. +3.  S is even: the first two are live together (own), and so are
    // the last two (full); only the last call of a position with S % 4 == 2 is own without being full.
    bool own[KMAX], full[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        own[k] = 4 * (tid + k * kThreads) < S;
        full[k] = 4 * (tid + k * kThreads) + 3 < S;
    }
    auto live = [&](int e) { return (e & 2) ? full[e >> 2] : own[e >> 2]; };
    auto sock = [&](int e) { return (uint32_t)((tid + (e >> 2) * kThreads) * 4 + (e & 3)); };
    // what the stage holds for socket sck = DV*t + i at CN position p: edge i of VN t of position p - i (BPF:1712), which is
    // off the chain only at the chain's ends (p < DV - 1 or p >= L)
    auto stage_entry = [&](int p, bool ends, uint32_t sck) -> uint16_t {
        if (ends && (unsigned)(p - (int)(sck - (uint32_t)DV * small_div<DV>(sck))) >= (unsigned)a.L) return (uint16_t)0xFFFFu;
        return (uint16_t)sck;
    };
    uint32_t edge_of = 0;                                               // this thread's sockets' edges s % DV, three bits each
    if constexpr (CNMODE != 0) {
#pragma unroll
        for (int e = 0; e < E; e++) edge_of |= (sock(e) - (uint32_t)DV * small_div<DV>(sock(e) & 8191u)) << (3 * e);
        asm volatile("" : "+v"(edge_of));                               // (kept packed: not E registers across the position loop)
    }
    // stage[rank[e]] = this thread's live socket e, or 0xFFFF.  The sockets and their edges are cut out of two registers at
    // every use (the empty asm keeps the compiler from carrying 3 E loop-invariant registers across the position loop instead)
    auto stage_own = [&](int p, bool ends, const uint32_t (&rank)[E]) {
        uint32_t s0 = 4u * (uint32_t)tid, eo = edge_of;
        asm volatile("" : "+v"(s0), "+v"(eo));
        if (!ends) {
#pragma unroll
            for (int e = 0; e < E; e++)
                if (live(e)) stage[rank[e]] = (uint16_t)(s0 + (uint32_t)((e >> 2) * 4 * kThreads + (e & 3)));
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) {
                const bool off = (unsigned)(p - (int)((eo >> (3 * e)) & 7u)) >= (unsigned)a.L;
                if (live(e)) stage[rank[e]] = off ? (uint16_t)0xFFFFu : (uint16_t)(s0 + (uint32_t)((e >> 2) * 4 * kThreads + (e & 3)));
            }
        }
    };

    // (the layout of a hist word while counting and after the scan: scan_hist, sampler_common.h)
    for (int b = tid; b < nb; b += kThreads) hist[b] = 0;
    if (tid == 0) { wsum[kWaves] = 0; wsum[kWaves + 1] = 0; }
    __syncthreads();

    const int tr = (int)blockIdx.x;
    const unsigned long long trial = a.trial0 + (unsigned long long)tr;
    const uint32_t t_lo = (uint32_t)trial, t_hi = (uint32_t)(trial >> 32);
    // Edge i drawn at step p belongs to VN position p - i, whose row goes out at step p - i + DV - 1: it waits DV - 1 - i steps.
    // pend[j] holds, for VN tid + 1024 j, one queue of DV - 1 - i ids per edge i < DV - 1 (dv (dv - 1) / 2 ids in all), two ids
    // to a register, the oldest in the low half of the queue's first word: a step is one v_alignbit per word.
    constexpr int PW = DV == 3 ? 2 : 6;                                 // words: ceil(2/2) + ceil(1/2); ceil(4/2) + 2 + 1 + 1
    auto q_words = [](int i) { return (DV - 1 - i + 1) / 2; };
    auto q_off = [&](int i) { int o = 0; for (int k = 0; k < i; k++) o += q_words(k); return o; };
    uint32_t pend[VMAX][PW];
#pragma unroll
    for (int j = 0; j < VMAX; j++)
#pragma unroll
        for (int w = 0; w < PW; w++) pend[j][w] = 0;
    // the keys of position p+1 are drawn while the worklist lanes of position p chase their bucket mates: nxt[] carries them
    uint32_t nxt[E];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        uint32_t r[4] = {0, 0, 0, 0};
        if (own[k]) philox4x32_10((uint32_t)(tid + k * kThreads), 0u, t_lo, t_hi, a.seed_lo, a.seed_hi, r);
#pragma unroll
        for (int u = 0; u < 4; u++) nxt[4 * k + u] = r[u];
    }
    for (int p = 0; p < a.D; p++) {
        const bool ends = p < DV - 1 || p >= a.L;                       // some VN position p - i is off the chain
        // ---- bucket histogram of this position's keys (dead sockets add zero)
        uint32_t key[E], slot[E], crowded = 0;
        auto word_of = [](uint32_t k) { return (k >> KSHIFT) & ~3u; };
        auto nib_of = [](uint32_t k) { return (k >> (KSHIFT - 2)) & 12u; };
#pragma unroll
        for (int e = 0; e < E; e++) {
            key[e] = nxt[e];
            const uint32_t sh = nib_of(key[e]);
            uint32_t *w = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(hist) + word_of(key[e]));
            slot[e] = (atomicAdd(w, (live(e) ? 1u : 0u) << sh) >> sh) & 0xFu;
            if constexpr (!INCL) crowded = max(crowded, slot[e]);
        }
        // a bucket count that does not fit its nibble, or straddlers that do not fit their worklist: the exact fallback below
        if (!INCL && crowded >= 15u) wsum[kWaves + 1] = 1u;
        __syncthreads();

        // ---- exclusive scan of the bucket counts; false: the histogram's ranks do not hold (exact fallback)
        const bool ranked = scldpc_dev::scan_hist<ROWS, INCL>(hist, wsum, tid, lane, wave, S);

        // ---- classify: every live key gets rank g0 + arrival slot, which gives the right CN (rank / dc) when its bucket lies
        //      inside one block of dc ranks.  CN ids go into fix, sockets into the rank-ordered stage; keys of buckets that
        //      span two CNs also go on the worklist [bucket's end rank:16 | first rank:16], pk = key << LG | socket.
        if (ranked) {
            uint32_t rk[E], g0a[E], g1a[E];
            bool st[E];
            if constexpr (INCL) {
                uint32_t h[E];
#pragma unroll
                for (int e = 0; e < E; e++) h[e] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(hist) + word_of(key[e]));
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const uint32_t t = h[e] >> nib_of(key[e]), pre = h[e] >> 20;
                    g0a[e] = pre + (t & 0xFu);
                    g1a[e] = pre + ((t >> 4) & 0xFu);
                    rk[e] = g0a[e] + slot[e];
                    st[e] = live(e) && small_div<DC>(g0a[e]) != small_div<DC>(g1a[e] - 1u);
                }
            } else {
                scldpc_dev::bucket_ranges_excl<KSHIFT>(hist, key, live, g0a, g1a);
#pragma unroll
                for (int e = 0; e < E; e++) {
                    rk[e] = g0a[e] + slot[e];
                    st[e] = live(e) && small_div<DC>(g0a[e]) != small_div<DC>(g1a[e] - 1u);
                }
            }
            if constexpr (INCL) {
                // the wave's straddlers take consecutive worklist entries: ballots and one LDS atomic per wave
                unsigned long long vote[E], anyv = 0;
                int total = 0;
#pragma unroll
                for (int e = 0; e < E; e++) { vote[e] = __builtin_amdgcn_ballot_w64(st[e]); anyv |= vote[e]; total += __builtin_popcountll(vote[e]); }
                if (anyv) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(reinterpret_cast<int *>(&wsum[kWaves]), total);
                    base = __builtin_amdgcn_readfirstlane(base);
                    // past the list's end the entries are not written: the count still grows, and the exact fallback ranks
                    // the position
                    const bool fits = base + total <= kWorkCap;
#pragma unroll
                    for (int e = 0; e < E; e++) {
                        if (st[e]) {
                            const uint32_t w = __builtin_amdgcn_mbcnt_hi((uint32_t)(vote[e] >> 32),
                                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)vote[e], (uint32_t)base));
                            const uint32_t pk = (key[e] << LG) | sock(e);
                            gpk[rk[e]] = pk;
                            if (fits) { wl[2 * w] = g0a[e] | (g1a[e] << 16); wl[2 * w + 1] = pk; }
                        }
                        base += __builtin_popcountll(vote[e]);
                    }
                }
            } else {
                uint32_t smask = 0;
#pragma unroll
                for (int e = 0; e < E; e++) smask |= (st[e] ? 1u : 0u) << e;
                while (smask) {                                         // rare (3 % of the keys): one short divergent loop
                    const uint32_t e = (uint32_t)__ffs((int)smask) - 1u;
                    smask &= smask - 1u;
                    uint32_t ky = key[0], r0 = rk[0], g0 = g0a[0], g1 = g1a[0];
#pragma unroll
                    for (int f = 1; f < E; f++)
                        if (e == (uint32_t)f) { ky = key[f]; r0 = rk[f]; g0 = g0a[f]; g1 = g1a[f]; }
                    const uint32_t pk = (ky << LG) | (uint32_t)((tid + (int)(e >> 2) * kThreads) * 4 + (int)(e & 3u));
                    gpk[r0] = pk;
                    const int w = atomicAdd(reinterpret_cast<int *>(&wsum[kWaves]), 1);
                    if (w < kWorkCap) { wl[2 * w] = g0 | (g1 << 16); wl[2 * w + 1] = pk; }
                }
            }
#pragma unroll
            for (int k = 0; k < KMAX; k++) {                            // provisional CN ids (final unless on the worklist)
                if (!own[k]) continue;
                const uint32_t lo = small_div<DC>(rk[4 * k]) | (small_div<DC>(rk[4 * k + 1]) << 16);
                if (full[k]) {
                    const uint32_t hi = small_div<DC>(rk[4 * k + 2]) | (small_div<DC>(rk[4 * k + 3]) << 16);
                    reinterpret_cast<uint2 *>(fix)[tid + k * kThreads] = make_uint2(lo, hi);
                } else {
                    reinterpret_cast<uint32_t *>(fix)[2 * (tid + k * kThreads)] = lo;
                }
            }
            if constexpr (CNMODE != 0) stage_own(p, ends, rk);
        }
        __syncthreads();

        // ---- the worklist: true rank among the bucket mates; counters cleared for the next position
        {
            scldpc_dev::clear_hist_words<ROWS>(hist, tid);
            int nwork = (int)wsum[kWaves];
            const bool exact = !ranked || nwork > kWorkCap || a.force_exact == p || a.force_exact == -2;
            if (exact) {
                // every key's true rank among all S keys, ties by socket: S comparisons per key — never taken in a real run
                nwork = 0;
#pragma unroll
                for (int e = 0; e < E; e++) if (live(e)) gpk[sock(e)] = key[e];
                __syncthreads();
                uint32_t xr[E];
#pragma unroll
                for (int e = 0; e < E; e++) xr[e] = 0;
                for (int s2 = 0; s2 < S; s2++) {
                    const uint32_t k2 = gpk[s2];
#pragma unroll
                    for (int e = 0; e < E; e++) xr[e] += (k2 < key[e]) || (k2 == key[e] && (uint32_t)s2 < sock(e));
                }
#pragma unroll
                for (int e = 0; e < E; e++)
                    if (live(e)) fix[sock(e)] = (uint16_t)small_div<DC>(xr[e]);
                if constexpr (CNMODE != 0) stage_own(p, ends, xr);
            }
            scldpc_dev::resolve_worklist<LG, CNMODE != 0>(nwork, tid, wl, gpk, stage, fix, [&](uint32_t sck) { return stage_entry(p, ends, sck); },
                                                          [](uint32_t r) { return small_div<DC>(r); });
        }
        if (p + 1 < a.D) {
            // the round keys are recomputed from the seed here rather than kept in twenty SGPRs across the whole loop
            uint32_t k_lo = a.seed_lo, k_hi = a.seed_hi;
            asm volatile("" : "+s"(k_lo), "+s"(k_hi));
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                uint32_t r[4] = {0, 0, 0, 0};
                if (own[k]) philox4x32_10((uint32_t)(tid + k * kThreads), (uint32_t)(p + 1), t_lo, t_hi, k_lo, k_hi, r);
#pragma unroll
                for (int u = 0; u < 4; u++) nxt[4 * k + u] = r[u];
            }
        }
        __syncthreads();
        if (tid == 0) { wsum[kWaves] = 0; wsum[kWaves + 1] = 0; }        // read again only after the next two barriers

        // ---- VN position q = p-dv+1 now has all its dv edges (BPF:1703-1716); CN position p its sockets.  This step drew
        //      edge i of VN position p - i: fix[dv*v + i]
        //      (tv: the thread's index behind an empty asm, so that the addresses below are computed here, at two or three
        //      operations each, and not carried in registers across the whole position loop)
        const int qpos = p - (DV - 1);
        int tv = tid;
        asm volatile("" : "+v"(tv));
#pragma unroll
        for (int j = 0; j < VMAX; j++) {
            const int v = tv + j * kThreads;
            if (v >= a.vns_pos) continue;
            uint32_t c[DV];
#pragma unroll
            for (int i = 0; i < DV; i++) c[i] = fix[DV * v + i];
            if (qpos >= 0) {
                uint16_t *row = a.vn_adj16 + ((size_t)tr * a.n + (size_t)qpos * a.vns_pos + (size_t)v) * DV;
#pragma unroll
                for (int i = 0; i < DV - 1; i++) row[i] = (uint16_t)pend[j][q_off(i)];       // the queues' oldest ids
                row[DV - 1] = (uint16_t)c[DV - 1];
            }
#pragma unroll
            for (int i = 0; i < DV - 1; i++) {                          // every queue drops its oldest id and takes c[i]
                const int o = q_off(i), nw = q_words(i);
#pragma unroll
                for (int w = 0; w + 1 < nw; w++) pend[j][o + w] = __builtin_amdgcn_alignbit(pend[j][o + w + 1], pend[j][o + w], 16);
                pend[j][o + nw - 1] = (DV - 1 - i) % 2 == 0 ? __builtin_amdgcn_alignbit(c[i], pend[j][o + nw - 1], 16) : c[i];
            }
        }
        if constexpr (CNMODE != 0) {
            uint16_t *trow = a.cn_sock16 + ((size_t)tr * a.D + p) * (size_t)S;
            if (a.tabw == 8) {
                uint2 *dst = reinterpret_cast<uint2 *>(trow);
                const uint2 *src = reinterpret_cast<const uint2 *>(stage);
                for (int w = tv; w < (S >> 2); w += kThreads) dst[w] = src[w];
            } else if (a.tabw == 4) {
                uint32_t *dst = reinterpret_cast<uint32_t *>(trow);
                const uint32_t *src = reinterpret_cast<const uint32_t *>(stage);
                for (int w = tv; w < (S >> 1); w += kThreads) dst[w] = src[w];
            } else {
                for (int w = tv; w < S; w += kThreads) trow[w] = stage[w];
            }
        }
    }

    // ---- channel: 32 VNs per output word, 8 Philox calls
    uint32_t *chan = a.chan + (size_t)tr * a.nw;
    for (int w = tid; w < a.nw; w += kThreads) {
        uint32_t word = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            uint32_t r[4];
            philox4x32_10((uint32_t)(w * 8 + c), 0x80000000u, t_lo, t_hi, a.seed_lo, a.seed_hi, r);
#pragma unroll
            for (int u = 0; u < 4; u++) word |= scldpc_dev::channel_erased(r[u], a.thresh) << (c * 4 + u);
        }
        const int j0 = w * 32;
        word = scldpc_dev::channel_tail(word, j0, a.n);
        for (int d = 0; d < a.ndoped; d++) word = scldpc_dev::channel_undope(word, j0, a.doped[d], a.vns_pos);
        chan[w] = word;
    }
}

bool deg_shape(const scldpc_code_params *p)
{
    if (scldpc::check_params(p)) return false;
    const int64_t S = (int64_t)p->cns_pos * p->dc;
    return ((p->dv == 3 && p->dc == 6) || (p->dv == 5 && p->dc == 10)) && S <= kMaxSockets && (int64_t)p->vns_pos * p->dv == S;
}

template <int DV, int DC, int CNMODE>
void (*deg_kernel(int rows))(const SDArgs)
{
    return rows == 1 ? sample_philox_v2_deg_kernel<DV, DC, 1, 1, CNMODE> : rows == 2 ? sample_philox_v2_deg_kernel<DV, DC, 1, 2, CNMODE>
         : rows == 4 ? sample_philox_v2_deg_kernel<DV, DC, 1, 4, CNMODE> : sample_philox_v2_deg_kernel<DV, DC, 2, 8, CNMODE>;
}

int launch_v2_deg(const char *who, const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials, double eps,
                  int32_t ndoped, const int32_t *doped_positions, uint16_t *d_vn_adj16, uint16_t *d_table, uint32_t *d_chan_bits,
                  void *stream)
{
    SDArgs a{};
    if (int rc = scldpc::check_sample_call(who, p, ntrials < 0 || (ntrials > 0 && (!d_vn_adj16 || !d_chan_bits)), ntrials, eps,
                                           ndoped, doped_positions, &a.ndoped, a.doped)) return rc;
    if (ntrials == 0) return SCLDPC_OK;
    const bool table = d_table != nullptr;

    a.L = p->L; a.cns_pos = p->cns_pos; a.vns_pos = p->vns_pos;
    a.n = scldpc::n_of(p); a.S = p->cns_pos * p->dc; a.D = p->L + p->dv - 1; a.nw = scldpc::nw_of(p);
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.thresh = scldpc::erasure_threshold(eps);
    int lg;                                         // one histogram, regions sized by S
    size_t lds_bytes;
    if (int rc = scldpc::v2_lds_layout(who, a.S, 1, false, table, &a, &lg, &lds_bytes)) return rc;
    a.vn_adj16 = d_vn_adj16; a.cn_sock16 = d_table; a.chan = d_chan_bits;
    const uintptr_t taddr = reinterpret_cast<uintptr_t>(d_table);
    a.tabw = ((a.S & 3) == 0 && (taddr & 7u) == 0) ? 8 : (taddr & 3u) == 0 ? 4 : 2;

    const int rows = a.nb / kThreads;                       // 1, 2, 4 (one Philox call per thread) or 8 (two)
    void (*kern)(const SDArgs) = p->dv == 3 ? (table ? deg_kernel<3, 6, 2>(rows) : deg_kernel<3, 6, 0>(rows))
                                            : (table ? deg_kernel<5, 10, 2>(rows) : deg_kernel<5, 10, 0>(rows));
    if (int rc_ = scldpc::allow_max_lds(reinterpret_cast<const void *>(kern))) return rc_;
    hipLaunchKernelGGL(kern, dim3(ntrials), dim3(kThreads), lds_bytes, static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

}  // namespace

// 1 when scldpc_sample_philox_device_deg_sock16 takes this ensemble: the pairs (3,6) and (5,10) with at most 8192 sockets per
// CN position (dv = 4, dc = 8 has scldpc_sample_philox_device_sock16)
extern "C" int scldpc_sample_philox_deg_sock16_supported(const scldpc_code_params *p)
{
    return p && deg_shape(p) ? 1 : 0;
}

extern "C" int scldpc_sample_philox_device_deg_sock16(const scldpc_code_params *p, uint64_t seed, uint64_t trial0,
                                                      int32_t ntrials, double eps, int32_t ndoped,
                                                      const int32_t *doped_positions, uint16_t *d_vn_adj16,
                                                      uint16_t *d_cn_sock16, uint32_t *d_chan_bits, void *stream)
{
    const char *who = "scldpc_sample_philox_device_deg_sock16";
    if (int rc = scldpc::check_params(p)) return rc;
    if (!scldpc_sample_philox_deg_sock16_supported(p))
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: takes dv = 3, dc = 6 or dv = 5, dc = 10 and at most %d sockets per "
                                 "position (got dv=%d dc=%d cns_pos=%d: %lld sockets)", who, kMaxSockets, p->dv, p->dc, p->cns_pos,
                                 (long long)p->cns_pos * p->dc);
    return launch_v2_deg(who, p, seed, trial0, ntrials, eps, ndoped, doped_positions, d_vn_adj16, d_cn_sock16, d_chan_bits,
                         stream);
}
