// Second-generation sampler beyond 8192 sockets per CN position (gfx950): 8192 < S = cns_pos * dc <= 20480, three to five Philox
// calls per thread, for the pairs (3,6), (4,8) and (5,10).  sampler_v2_deg.hip's ranking — a key histogram whose buckets give the
// CN of every key they hold unless they straddle a multiple of dc, a worklist for the few keys that do, the CN -> socket table
// as the inverse of the ranking — does not fit 160 KiB at these sizes with its regions sized by S, so a position of more than
// 12288 sockets is ranked in two parts, by the top bit of the key (up to 12288 sockets: in one part, all keys):
//
//  * part 1's keys all rank behind the keys of part 0: its first rank (base) is part 0's count, which the scan's wave totals
//    give.
//  * each part counts its keys in one histogram of 8192 words over the next 15 key bits (four nibble-wide buckets a word),
//    scans it (scan_hist), tests a bucket [base + g0, base + g1) for a multiple of dc inside it, pushes the keys of such buckets
//    on the worklist with their packed keys pk = key << 15 | socket at their part-local rank (the 15 key bits this drops are
//    among those that bucket mates share), and stages its sockets in part-local rank order; the stage leaves for the table's
//    entries [base, base + count) before the next part writes it.
//  * kept for the whole position: the S CN ids (fix) that the VN rows are read from, as in sampler_v2_deg.hip.
//
// (Four parts by two key bits and a capacity of 8192 fit as well, but every thread then walks its keys four times a position
// with a quarter of the lanes at work each time: measured, that sampler was slower at S = 20000 than the first generation with
// its own table.)
// One of two parts has Binomial(S, 1/2) keys (mean 10240, sigma 72 at S = 20480) against a capacity of 12288.  A part over its
// capacity (a.part_cap: a kernel argument, lowered by SCLDPC_DEBUG_SAMPLER_PART_CAP), a nibble that fills or a worklist that
// overflows sends the whole position to the exact fallback: every key's true rank by S comparisons, ties by socket; its S keys
// lie in the histogram and the packed keys, which are side by side, and its table entries go straight to global memory.
//
// Keys are drawn once per position and stay in registers (the arrival slots four bits each beside them); the next position's
// keys are drawn behind the last part's worklist.  Nothing of the ranking goes through global memory, there is no workspace, and
// the VN rows leave through the register queues of sampler_v2_deg.hip (pend[]).
// Same law, same keys (word s & 3 of philox4x32_10(s >> 2, p, trial, seed)), rank by key, ties by socket: vn_adj16 and the
// channel words are bit for bit scldpc_sample_philox_device_adj16's, the table is scldpc_cn_sockets_device's as a set per CN.
#include "sampler_common.h"
#include "philox.h"

namespace {

using scldpc_dev::philox4x32_10;

constexpr int kThreads = scldpc::kSamplerThreads;
constexpr int kWaves = kThreads / 64;
using scldpc::kMaxDoped;
using scldpc::kWorkCap;                         // keys of buckets that span two CNs, per part
constexpr int kHistWords = scldpc::kWideHistWords;
constexpr int kPartCap = scldpc::kWidePartCap;  // keys of a part: packed keys, stage entries
constexpr int kMinSockets = 8192;               // per CN position: at and below, sampler_v2.hip and sampler_v2_deg.hip
constexpr int kMaxSockets = scldpc::kWideMaxSockets;
static_assert(kMaxSockets == 20480 && kMaxSockets < (1 << 15), "five Philox calls per thread; a socket takes 15 bits of pk");
static_assert(kPartCap == 3 * 4096 && kPartCap < (1 << 16), "three calls per thread rank in one part; the worklist's 16-bit ranks");

struct SWArgs {
    int L, cns_pos, vns_pos, n, S, D, nw;
    int force_exact;                    // diagnostics: rank this CN position by the exact fallback (-1: none, -2: every position)
    int part_cap;                       // keys a part may hold (<= kPartCap); a part with more sends its position to the fallback
    int tabw;                           // bytes per store of the table's copy-out: 4 or 2 (by the table's alignment)
    int roww;                           // bytes per store of a VN row: 8 (dv = 4, aligned rows) or 2
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

// x / D for x <= 20480 (ranks and sockets) as one 24-bit multiply and a shift
template <int D> constexpr uint32_t wide_magic() { return ((1u << 18) + D - 1) / D; }
template <int D> constexpr bool wide_div_exact()
{
    for (uint32_t x = 0; x <= (uint32_t)kMaxSockets; x++)
        if (((x * wide_magic<D>()) >> 18) != x / D) return false;
    return wide_magic<D>() < (1u << 24) && (uint64_t)kMaxSockets * wide_magic<D>() < (1ull << 32);
}
static_assert(wide_div_exact<3>() && wide_div_exact<4>() && wide_div_exact<5>() && wide_div_exact<6>() && wide_div_exact<8>() &&
              wide_div_exact<10>(), "the multiply-and-shift division holds for every rank and socket up to 20480");
template <int D> __device__ __forceinline__ uint32_t wide_div(uint32_t x)
{
    if constexpr (D == 4) return x >> 2;
    else if constexpr (D == 8) return x >> 3;
    else return __umul24(x, wide_magic<D>()) >> 18;
}

// KMAX = Philox calls (4 sockets each) per thread and position: 3 up to 12288 sockets per position, 4 up to 16384, 5 up to 20480
// TABLE: the CN -> socket table goes out (the rank-ordered stage holds the sockets themselves)
template <int DV, int DC, int KMAX, bool TABLE>
__global__ __launch_bounds__(kThreads, 4) __attribute__((amdgpu_num_sgpr(72))) void sample_philox_v2_wide_kernel(const SWArgs a)
{
    static_assert((DV == 3 && DC == 6) || (DV == 4 && DC == 8) || (DV == 5 && DC == 10), "the pairs (3,6), (4,8) and (5,10)");
    static_assert(KMAX >= 3 && KMAX <= 5, "8192 < S <= 20480");
    constexpr int E = 4 * KMAX;
    constexpr int VMAX = (4096 * KMAX / DV + kThreads - 1) / kThreads;  // VNs per thread: vns_pos = S / DV <= 4096 KMAX / DV
    constexpr int NPARTS = KMAX == 3 ? 1 : 2;                           // S <= kPartCap: every key in one part
    constexpr int ROWS = kHistWords / kThreads;                         // histogram words per thread
    constexpr int LG = 15;                                              // socket bits of a packed key
    constexpr int KSHIFT = 17;                                          // (key << (NPARTS - 1)) >> KSHIFT = the part's fine bucket
    static_assert(ROWS == 8, "scan_hist's eight words per thread");
    extern __shared__ uint32_t lds[];
    uint32_t *hist = lds;                                               // 8192 words of four nibble-wide bucket counters
    uint32_t *gpk = lds + a.off_gpk;                                    // packed keys of straddling buckets, by part-local rank
    uint16_t *stage = reinterpret_cast<uint16_t *>(lds + a.off_stage);  // the part's sockets in part-local rank order
    uint16_t *fix = reinterpret_cast<uint16_t *>(lds + a.off_fix);      // S CN-local ids of this position's sockets
    uint32_t *wsum = lds + a.off_wsum;                                  // two sets of 16 wave totals, worklist counter, overflow flag
    uint32_t *wl = wsum + 64;                                           // worklist: 2 words per key of a straddling bucket

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S;
    // call k of this thread draws sockets 4*(tid + 1024 k) .. +3.  S is even, so a call has four live sockets, two (the last call
    // of a position with S % 4 == 2) or none.  Whether socket e is live is one compare at every use, not a mask kept across the
    // position loop (s4: 4 tid behind an empty asm wherever it is used, so that the compares are not hoisted)
    auto fresh4 = [&]() { uint32_t x = 4u * (uint32_t)tid; asm volatile("" : "+v"(x)); return x; };
    auto sock = [&](uint32_t s4, int e) { return s4 + (uint32_t)((e >> 2) * 4 * kThreads + (e & 3)); };
    auto live = [&](uint32_t s4, int e) { return sock(s4, e) < (uint32_t)S; };
    auto own = [&](uint32_t s4, int k) { return sock(s4, 4 * k) < (uint32_t)S; };
    // what the table holds for socket sck = DV*t + i at CN position p: edge i of VN t of position p - i (BPF:1712), which is
    // off the chain only at the chain's ends (p < DV - 1 or p >= L)
    auto stage_entry = [&](int p, bool ends, uint32_t sck) -> uint16_t {
        if (ends && (unsigned)(p - (int)(sck - (uint32_t)DV * wide_div<DV>(sck))) >= (unsigned)a.L) return (uint16_t)0xFFFFu;
        return (uint16_t)sck;
    };

    // (the layout of a hist word while counting and after the scan: scan_hist, sampler_common.h)
    scldpc_dev::clear_hist_words<ROWS>(hist, tid);
    if (tid < 64) wsum[tid] = 0;
    __syncthreads();

    const int tr = (int)blockIdx.x;
    const unsigned long long trial = a.trial0 + (unsigned long long)tr;
    const uint32_t t_lo = (uint32_t)trial, t_hi = (uint32_t)(trial >> 32);
    // Edge i drawn at step p belongs to VN position p - i, whose row goes out at step p - i + DV - 1: it waits DV - 1 - i steps.
    // pend[j] holds, for VN tid + 1024 j, one queue of DV - 1 - i ids per edge i < DV - 1 (dv (dv - 1) / 2 ids in all), two ids
    // to a register, the oldest in the low half of the queue's first word: a step is one v_alignbit per word.
    constexpr int PW = DV == 3 ? 2 : DV == 4 ? 4 : 6;                   // words: sum over i < DV - 1 of ceil((DV - 1 - i) / 2)
    auto q_words = [](int i) { return (DV - 1 - i + 1) / 2; };
    auto q_off = [&](int i) { int o = 0; for (int k = 0; k < i; k++) o += q_words(k); return o; };
    uint32_t pend[VMAX][PW];
#pragma unroll
    for (int j = 0; j < VMAX; j++)
#pragma unroll
        for (int w = 0; w < PW; w++) pend[j][w] = 0;
    // the keys of a position, drawn once: those of position p+1 behind the last worklist of position p, into the same registers
    uint32_t key[E];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        __builtin_amdgcn_sched_barrier(0);                              // (one call at a time, here and below)
        uint32_t r[4] = {0, 0, 0, 0};
        if (own(fresh4(), k)) philox4x32_10((uint32_t)(tid + k * kThreads), 0u, t_lo, t_hi, a.seed_lo, a.seed_hi, r);
#pragma unroll
        for (int u = 0; u < 4; u++) key[4 * k + u] = r[u];
    }
    for (int p = 0; p < a.D; p++) {
        const bool ends = p < DV - 1 || p >= a.L;                       // some VN position p - i is off the chain
        uint16_t *trow = TABLE ? a.cn_sock16 + ((size_t)tr * a.D + p) * (size_t)S : nullptr;
        uint32_t slots[(E + 7) / 8];                                    // arrival slots of the keys in their buckets, 4 bits each
#pragma unroll
        for (int w = 0; w < (E + 7) / 8; w++) slots[w] = 0;
        int base = 0;                                                   // first rank of the part: the keys of the parts below
        bool bad = false;                                               // some part's ranks do not hold: the exact fallback
#pragma unroll 1
        for (uint32_t q = 0; q < (uint32_t)NPARTS; q++) {
            const uint32_t pc = (uint32_t)p * NPARTS + q;               // parts alternate between the two sets:
            uint32_t *ws = wsum + 32 * (pc & 1u);                       // this part's wave totals, ws[kWaves] worklist counter,
            uint32_t *wo = wsum + 32 * (~pc & 1u);                      // ws[kWaves + 1] overflow flag; the other part's set
            auto part_of = [](uint32_t k) { return NPARTS == 1 ? 0u : k >> 31; };
            // ---- bucket histogram of the part's keys
            uint32_t crowded = 0;
            uint32_t s4 = fresh4();
            // (the keys behind an empty asm: their words, shifts and masks are worked out in every part, at two or three
            // operations each, and not carried in 3 E registers across the parts)
#pragma unroll
            for (int e = 0; e < E; e++) asm volatile("" : "+v"(key[e]));
#pragma unroll
            for (int e = 0; e < E; e++) {
                if (live(s4, e) && part_of(key[e]) == q) {
                    const uint32_t kb = key[e] << (NPARTS - 1), sh = (kb >> (KSHIFT - 2)) & 12u;
                    uint32_t *w = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(hist) + ((kb >> KSHIFT) & 0x7FFCu));
                    const uint32_t sl = (atomicAdd(w, 1u << sh) >> sh) & 0xFu;
                    slots[e >> 3] |= sl << (4 * (e & 7));
                    crowded = max(crowded, sl);
                }
                if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // (one call at a time: not E addresses and shifts at once)
            }
            // a bucket count that does not fit its nibble: the exact fallback below
            if (crowded >= 15u) ws[kWaves + 1] = 1u;
            __syncthreads();
            if (tid == 0) { wo[kWaves] = 0; wo[kWaves + 1] = 0; }      // last read in the part before, written next behind this one

            // ---- exclusive scan of the bucket counts; false: the histogram's ranks do not hold
            const bool ranked = scldpc_dev::scan_hist<ROWS, false>(hist, ws, tid, lane, wave, S);
            uint32_t cnt = 0;                                           // the part's keys: the sum of the 16 wave totals
#pragma unroll
            for (int w = 0; w < kWaves; w++) cnt += ws[w];
            const int count = __builtin_amdgcn_readfirstlane((int)cnt);
            bool ok = !bad && ranked && count <= a.part_cap && base + count <= S;

            // ---- classify: every key of the part gets part-local rank g0 + arrival slot, and base + that gives the right CN
            //      (rank / dc) when its bucket lies inside one block of dc ranks.  CN ids go into fix, sockets into the
            //      rank-ordered stage; keys of buckets that span two CNs also go on the worklist
            //      [bucket's end rank:16 | first rank:16] (part-local), pk = key << LG | socket.
            if (ok) {
                s4 = fresh4();
#pragma unroll
                for (int k = 0; k < KMAX; k++) {
                    __builtin_amdgcn_sched_barrier(0);
                    uint32_t k4[4], g0a[4], g1a[4];
                    bool in[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        k4[u] = key[4 * k + u] << (NPARTS - 1);
                        in[u] = live(s4, 4 * k + u) && part_of(key[4 * k + u]) == q;
                    }
                    if (!(in[0] || in[1] || in[2] || in[3])) continue;
                    scldpc_dev::bucket_ranges_excl<KSHIFT>(hist, k4, [&](int u) { return in[u]; }, g0a, g1a);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (!in[u]) continue;
                        const int e = 4 * k + u;
                        const uint32_t rk = g0a[u] + ((slots[e >> 3] >> (4 * (e & 7))) & 0xFu);
                        fix[sock(s4, e)] = (uint16_t)wide_div<DC>((uint32_t)base + rk);
                        if constexpr (TABLE) stage[rk] = stage_entry(p, ends, sock(s4, e));
                        if (wide_div<DC>((uint32_t)base + g0a[u]) != wide_div<DC>((uint32_t)base + g1a[u] - 1u)) {
                            const uint32_t pk = (key[e] << LG) | sock(s4, e);
                            gpk[rk] = pk;
                            // past the list's end the entries are not written: the count still grows, and the exact fallback
                            // ranks the position
                            const int w = atomicAdd(reinterpret_cast<int *>(&ws[kWaves]), 1);
                            if (w < kWorkCap) { wl[2 * w] = g0a[u] | (g1a[u] << 16); wl[2 * w + 1] = pk; }
                        }
                    }
                }
            }
            __syncthreads();

            // ---- the worklist: true rank among the bucket mates; counters cleared for the next part
            scldpc_dev::clear_hist_words<ROWS>(hist, tid);
            const int nwork = __builtin_amdgcn_readfirstlane((int)ws[kWaves]);
            ok = ok && nwork <= kWorkCap;
            if (ok)
                scldpc_dev::resolve_worklist<LG, TABLE>(nwork, tid, wl, gpk, stage, fix, [&](uint32_t sck) { return stage_entry(p, ends, sck); },
                                                        [&](uint32_t r) { return wide_div<DC>((uint32_t)base + r); });
            __syncthreads();

            // ---- the part's sockets in rank order are the table's entries base .. base + count - 1 of this position
            if constexpr (TABLE) {
                if (ok) {
                    if (a.tabw == 4) {
                        // whole words where both halves are the part's: an odd base or end leaves one entry on its own
                        const int lo = base, hi = base + count;
                        if (tid == 0 && (lo & 1) && count > 0) trow[lo] = stage[0];
                        if (tid == 64 && (hi & 1) && hi - 1 >= lo) trow[hi - 1] = stage[hi - 1 - lo];
                        uint32_t *dst = reinterpret_cast<uint32_t *>(trow);
                        for (int w = ((lo + 1) >> 1) + tid; w < (hi >> 1); w += kThreads)
                            dst[w] = (uint32_t)stage[2 * w - lo] | ((uint32_t)stage[2 * w + 1 - lo] << 16);
                    } else {
                        for (int w = tid; w < count; w += kThreads) trow[base + w] = stage[w];
                    }
                }
            }
            bad = bad || !ok;
            base += count;
        }

        // ---- the exact fallback: every key's true rank among all S keys, ties by socket: S comparisons per key — never taken
        //      in a real run.  The S keys lie in the histogram and the packed keys; the table's entries go straight out
        if (bad || a.force_exact == p || a.force_exact == -2) {
            __syncthreads();                                            // (the last part's stage has left)
            uint32_t *keys = lds;
            const uint32_t s4 = fresh4();
#pragma unroll
            for (int e = 0; e < E; e++) if (live(s4, e)) keys[sock(s4, e)] = key[e];
            __syncthreads();
            // (one call's four keys at a time: four rank counters, not E)
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                uint32_t xr[4] = {0, 0, 0, 0};
#pragma unroll 1
                for (int s2 = 0; s2 < S; s2++) {
                    const uint32_t k2 = keys[s2];
#pragma unroll
                    for (int u = 0; u < 4; u++) xr[u] += (k2 < key[4 * k + u]) || (k2 == key[4 * k + u] && (uint32_t)s2 < sock(s4, 4 * k + u));
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!live(s4, 4 * k + u)) continue;
                    fix[sock(s4, 4 * k + u)] = (uint16_t)wide_div<DC>(xr[u]);
                    if constexpr (TABLE) trow[xr[u]] = stage_entry(p, ends, sock(s4, 4 * k + u));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();                                            // (every thread has read the keys)
            scldpc_dev::clear_hist_words<ROWS>(hist, tid);
        }
        if (p + 1 < a.D) {
            // the round keys are recomputed from the seed here rather than kept in twenty SGPRs across the whole loop, and the
            // calls' counters come from s4: their first products are not kept in 2 KMAX registers either
            uint32_t k_lo = a.seed_lo, k_hi = a.seed_hi;
            asm volatile("" : "+s"(k_lo), "+s"(k_hi));
            const uint32_t s4 = fresh4();
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                __builtin_amdgcn_sched_barrier(0);
                uint32_t r[4] = {0, 0, 0, 0};
                if (own(s4, k)) philox4x32_10((s4 >> 2) + (uint32_t)(k * kThreads), (uint32_t)(p + 1), t_lo, t_hi, k_lo, k_hi, r);
#pragma unroll
                for (int u = 0; u < 4; u++) key[4 * k + u] = r[u];
            }
        }
        __syncthreads();

        // ---- VN position q = p-dv+1 now has all its dv edges (BPF:1703-1716).  This step drew edge i of VN position p - i:
        //      fix[dv*v + i]
        //      (tv: the thread's index behind an empty asm, so that the addresses below are computed here, at two or three
        //      operations each, and not carried in registers across the whole position loop)
        const int qpos = p - (DV - 1);
        int tv = tid;
        asm volatile("" : "+v"(tv));
#pragma unroll
        for (int j = 0; j < VMAX; j++) {
            __builtin_amdgcn_sched_barrier(0);                          // (one VN at a time: not VMAX rows' ids and addresses at once)
            const int v = tv + j * kThreads;
            if (v >= a.vns_pos) continue;
            uint32_t c[DV];
#pragma unroll
            for (int i = 0; i < DV; i++) c[i] = fix[DV * v + i];
            if (qpos >= 0) {
                uint16_t *row = a.vn_adj16 + ((size_t)tr * a.n + (size_t)qpos * a.vns_pos + (size_t)v) * DV;
                bool whole = false;                                     // dv = 4: a row is one aligned 8-byte store
                if constexpr (DV == 4) whole = a.roww == 8;
                if (whole) {
                    *reinterpret_cast<uint2 *>(row) = make_uint2((pend[j][q_off(0)] & 0xFFFFu) | (pend[j][q_off(1)] << 16),
                                                                 (pend[j][q_off(DV - 2)] & 0xFFFFu) | (c[DV - 1] << 16));
                } else {
#pragma unroll
                    for (int i = 0; i < DV - 1; i++) row[i] = (uint16_t)pend[j][q_off(i)];   // the queues' oldest ids
                    row[DV - 1] = (uint16_t)c[DV - 1];
                }
            }
#pragma unroll
            for (int i = 0; i < DV - 1; i++) {                          // every queue drops its oldest id and takes c[i]
                const int o = q_off(i), nw = q_words(i);
#pragma unroll
                for (int w = 0; w + 1 < nw; w++) pend[j][o + w] = __builtin_amdgcn_alignbit(pend[j][o + w + 1], pend[j][o + w], 16);
                pend[j][o + nw - 1] = (DV - 1 - i) % 2 == 0 ? __builtin_amdgcn_alignbit(c[i], pend[j][o + nw - 1], 16) : c[i];
            }
        }
        // (fix is written next behind the first barrier of position p + 1)
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

bool wide_shape(const scldpc_code_params *p)
{
    if (scldpc::check_params(p)) return false;
    const int64_t S = (int64_t)p->cns_pos * p->dc;
    return ((p->dv == 3 && p->dc == 6) || (p->dv == 4 && p->dc == 8) || (p->dv == 5 && p->dc == 10)) && S > kMinSockets &&
           S <= kMaxSockets && (int64_t)p->vns_pos * p->dv == S;
}

template <int DV, int DC, bool TABLE>
void (*wide_kernel(int calls))(const SWArgs)
{
    return calls == 3 ? sample_philox_v2_wide_kernel<DV, DC, 3, TABLE> : calls == 4 ? sample_philox_v2_wide_kernel<DV, DC, 4, TABLE>
                                                                                    : sample_philox_v2_wide_kernel<DV, DC, 5, TABLE>;
}

int launch_v2_wide(const char *who, const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials, double eps,
                   int32_t ndoped, const int32_t *doped_positions, uint16_t *d_vn_adj16, uint16_t *d_table, uint32_t *d_chan_bits,
                   void *stream)
{
    SWArgs a{};
    if (int rc = scldpc::check_sample_call(who, p, ntrials < 0 || (ntrials > 0 && (!d_vn_adj16 || !d_chan_bits)), ntrials, eps,
                                           ndoped, doped_positions, &a.ndoped, a.doped)) return rc;
    if (ntrials == 0) return SCLDPC_OK;
    const bool table = d_table != nullptr;

    a.L = p->L; a.cns_pos = p->cns_pos; a.vns_pos = p->vns_pos;
    a.n = scldpc::n_of(p); a.S = p->cns_pos * p->dc; a.D = p->L + p->dv - 1; a.nw = scldpc::nw_of(p);
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.thresh = scldpc::erasure_threshold(eps);
    size_t lds_bytes;
    if (int rc = scldpc::v2_wide_lds_layout(who, a.S, &a, &lds_bytes)) return rc;
    a.vn_adj16 = d_vn_adj16; a.cn_sock16 = d_table; a.chan = d_chan_bits;
    a.tabw = (reinterpret_cast<uintptr_t>(d_table) & 3u) == 0 ? 4 : 2;          // (S is even: every position's row keeps it)
    a.roww = (p->dv == 4 && (reinterpret_cast<uintptr_t>(d_vn_adj16) & 7u) == 0) ? 8 : 2;

    const int calls = (a.S + 4 * kThreads - 1) / (4 * kThreads);                // Philox calls per thread: 3, 4 or 5
    void (*kern)(const SWArgs) = p->dv == 3 ? (table ? wide_kernel<3, 6, true>(calls) : wide_kernel<3, 6, false>(calls))
                               : p->dv == 4 ? (table ? wide_kernel<4, 8, true>(calls) : wide_kernel<4, 8, false>(calls))
                                            : (table ? wide_kernel<5, 10, true>(calls) : wide_kernel<5, 10, false>(calls));
    if (int rc_ = scldpc::allow_max_lds(reinterpret_cast<const void *>(kern))) return rc_;
    hipLaunchKernelGGL(kern, dim3(ntrials), dim3(kThreads), lds_bytes, static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

}  // namespace

// 1 when scldpc_sample_philox_device_wide_sock16 takes this ensemble: the pairs (3,6), (4,8) and (5,10) with more than 8192 and
// at most 20480 sockets per CN position (at and below 8192: scldpc_sample_philox_device_sock16 and ..._deg_sock16)
extern "C" int scldpc_sample_philox_wide_sock16_supported(const scldpc_code_params *p)
{
    return p && wide_shape(p) ? 1 : 0;
}

extern "C" int scldpc_sample_philox_device_wide_sock16(const scldpc_code_params *p, uint64_t seed, uint64_t trial0,
                                                       int32_t ntrials, double eps, int32_t ndoped,
                                                       const int32_t *doped_positions, uint16_t *d_vn_adj16,
                                                       uint16_t *d_cn_sock16, uint32_t *d_chan_bits, void *stream)
{
    const char *who = "scldpc_sample_philox_device_wide_sock16";
    if (int rc = scldpc::check_params(p)) return rc;
    if (!scldpc_sample_philox_wide_sock16_supported(p))
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: takes dv = 3, dc = 6, dv = 4, dc = 8 or dv = 5, dc = 10 with more than "
                                 "%d and at most %d sockets per position (got dv=%d dc=%d cns_pos=%d: %lld sockets)", who,
                                 kMinSockets, kMaxSockets, p->dv, p->dc, p->cns_pos, (long long)p->cns_pos * p->dc);
    return launch_v2_wide(who, p, seed, trial0, ntrials, eps, ndoped, doped_positions, d_vn_adj16, d_cn_sock16, d_chan_bits,
                          stream);
}
