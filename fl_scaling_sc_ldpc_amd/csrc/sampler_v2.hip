// Throughput-mode sampler, second generation (gfx950) — the (dv = 4, dc = 8) Olmos chain with up to 4096 sockets per
// CN position, i.e. the BASELINE ensemble (4,8,L,N <= 1024).  Same law and same Philox keys as sampler.hip
// (generate_code / channel_doped, BPF:1656-1761, 1547-1574): its vn_adj16 and channel words are bit for bit those of
// scldpc_sample_philox_device_adj16 and of the CPU twin.  Two differences:
//
//  * Ranking only where it matters.  The CN of a socket is rank / dc, so a bucket of the key histogram whose rank range
//    [g0, g1) lies inside one block of dc ranks gives all its keys the same CN whatever their order: CN = g0 / dc, no
//    comparison, no grouping.  Only the keys of buckets that straddle a multiple of dc (3 % of the keys at 0.24 keys per
//    bucket) are written out (packed [key's low bits | socket], one word) and compared with their bucket mates.
//    sampler.hip groups and ranks every key: 61 % of its cycles (profiles/r01_stamps.txt).
//  * The CN -> VN table comes with it: cn_adj16[trial][CN][dc] = the VNs attached to every CN (global VN index, which
//    needs n < 65535), which is just the inverse of the ranking: rank r holds socket s = dv*t + i, i.e. edge i of VN t
//    of position CNpos - i; at the chain ends sockets of positions outside [0, L) stand for no VN (the reference leaves
//    such CNs with a lower degree, BPF:1703-1716) and read 0xFFFF.  Within a CN the order is unspecified (arrival order
//    of the histogram atomics for non-straddling buckets): consumers treat the dc entries as a set.
//    full_bp_small.hip decodes from (vn_adj16, cn_adj16) with 4 bits of LDS per CN.
//
// sampler_common.h holds what this file shares with sampler_v2_deg.hip and sampler.hip: the histogram words of a thread, the
// scan, the two-calls-per-thread look-up, the worklist's resolve loop, the steps of a channel word, and on the host the
// validation, the threshold and the LDS layout.  Here stay both worklist pushes, the exact fallback, the row assembly in
// registers, the split Philox draw and the third generation.
#include "sampler_common.h"
#include "philox.h"

namespace {

using scldpc_dev::channel_erased;
using scldpc_dev::channel_tail;
using scldpc_dev::channel_undope;
using scldpc_dev::clear_hist_words;
using scldpc_dev::load_hist_words;
using scldpc_dev::store_hist_words;
using scldpc_dev::philox4x32_10;
using scldpc_dev::philox_prefix;
using scldpc_dev::philox_tail;
using scldpc_dev::philox_uniform;
using scldpc_dev::PhiloxPrefix;
using scldpc_dev::PhiloxUniform;
using scldpc_dev::wave_inclusive_scan;

constexpr int kThreads = scldpc::kSamplerThreads;
constexpr int kWaves = kThreads / 64;
using scldpc::kMaxDoped;
using scldpc::kWorkCap;                 // keys of buckets that span two CNs, per position (expected: 0.03 * S <= 250)

// atomicAdd on an LDS word, returning the old value, written as the instruction itself: given a uniform operand under a
// one-lane branch, the compiler's atomic optimizer wraps an atomicAdd in a lane election, a multiply and a multiply-add
// of its own (some 20 vector cycles per call).  The caller's barrier orders the word against its readers.
__device__ __forceinline__ uint32_t lds_add_rtn(uint32_t *p, uint32_t v)
{
    const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)p;
    uint32_t old;
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(addr), "v"(v) : "memory");
    return old;
}

struct S2Args {
    int L, cns_pos, vns_pos, n, S, D, nb, nw;
    int ntrials;                        // workgroup b samples trials b, b + gridDim.x, … (gridDim.x == ntrials unless persistent)
    int force_exact;                    // diagnostics: rank this CN position by the exact fallback (-1: none, -2: every position)
    int ndoped;
    int doped[kMaxDoped];
    uint32_t seed_lo, seed_hi;
    unsigned long long trial0;
    uint32_t thresh;                    // erased iff (draw >> 1) < thresh
    int off_gpk, off_fix, off_stage, off_wsum;      // LDS offsets in 32-bit words
    uint16_t *vn_adj16;                 // uint16 [T][n][4], CN index local to its position
    uint16_t *cn_adj16;                 // uint16 [T][D*cns_pos][8] VNs of every CN (0xFFFF: none), or null
    uint32_t *chan;
};

// LDS layout (32-bit words) of the one-call-per-thread instances: a function of ROWS and of whether a stage is kept
template <int ROWS, int CNMODE>
struct V2Layout {
    static constexpr int nb = ROWS * kThreads;                          // histogram words; also the bound of S
    static constexpr int off_gpk = nb, off_fix = off_gpk + nb, off_stage = off_fix + nb / 2;
    static constexpr int off_wsum = off_stage + (CNMODE != 0 ? nb / 2 : 0);
};

// KMAX = Philox calls (4 sockets each) per thread and position: 1 up to 4096 sockets per position, 2 up to 8192
// ROWS = histogram words per thread (nb / 1024)
// CNMODE: what the rank-ordered stage holds — 0 nothing, 1 the sockets' VNs (global VN index, scldpc_sample_philox_device_cn16),
//         2 the sockets themselves (s = dv*t + i: the table scldpc_sw_bp_ring_device reads; any n)
template <int KMAX, int ROWS, int CNMODE, bool PERSIST = false>
__global__ __launch_bounds__(kThreads, KMAX == 1 ? 8 : 4) __attribute__((amdgpu_num_sgpr(72))) void sample_philox_v2_kernel(const S2Args a)
{
    constexpr int DV = 4, DC_SHIFT = 3, E = 4 * KMAX;
    // the bucket geometry follows from ROWS (nb = 1024 * ROWS histogram words of four fine buckets): shifts and masks are
    // immediates, so no vector instruction takes a scalar operand for them (an SGPR source doubles a two-operand op's price)
    constexpr int LG = ROWS == 1 ? 10 : ROWS == 2 ? 11 : ROWS == 4 ? 12 : 13;        // log2(nb) = socket bits
    constexpr int KSHIFT = 32 - LG - 2;                                 // key >> KSHIFT = fine bucket
    // One Philox call per thread (at most 4096 sockets per position): the scan leaves INCLUSIVE nibble prefixes in the
    // word, so a key's first rank and its bucket's end are right shifts and masks, and the histogram's overflow is found
    // from the scan's grand total instead of a per-key check.  Two calls per thread (KMAX = 2) keep the exclusive form.
    constexpr bool INCL = KMAX == 1;
    static_assert(ROWS * kThreads == (1 << LG) && (INCL ? ROWS <= 4 : ROWS == 8), "ROWS is 1, 2, 4 (KMAX 1) or 8 (KMAX 2)");
    extern __shared__ uint32_t lds[];
    // One call per thread: the regions are laid out for nb sockets (S <= nb = 1024 * ROWS), so every LDS address is the
    // thread's offset plus an immediate and no offset is held in (or reloaded into) a scalar register; launch_v2 sizes the
    // allocation by the same V2Layout.  Two calls per thread: the offsets come with the arguments, sized by S.
    using Lay = V2Layout<ROWS, CNMODE>;
    const int off_gpk = INCL ? Lay::off_gpk : a.off_gpk, off_fix = INCL ? Lay::off_fix : a.off_fix;
    const int off_stage = INCL ? Lay::off_stage : a.off_stage, off_wsum = INCL ? Lay::off_wsum : a.off_wsum;
    uint32_t *hist = lds;                                               // nb words of four nibble-wide bucket counters
    uint32_t *gpk = lds + off_gpk;                                      // S words: packed keys of straddling buckets
    uint16_t *fix = reinterpret_cast<uint16_t *>(lds + off_fix);        // S CN-local ids of this position's sockets
    uint16_t *stage = reinterpret_cast<uint16_t *>(lds + off_stage);    // the S sockets (or their VNs) in rank order
    uint32_t *wsum = lds + off_wsum;                                    // 16 wave totals + the worklist counter
    uint32_t *wl = wsum + 32;                                           // worklist: 2 words per key of a straddling bucket

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave: kept scalar)
    const int S = a.S, nb = INCL ? ROWS * kThreads : a.nb;
    const int ncalls = S >> 2;                                          // S % 4 == 0 (checked on the host)
    bool own[KMAX];                                                     // call k of this thread: sockets 4*(tid + 1024 k) .. +3
#pragma unroll
    for (int k = 0; k < KMAX; k++) own[k] = tid + k * kThreads < ncalls;
    auto sock = [&](int e) { return (uint32_t)((tid + (e >> 2) * kThreads) * 4 + (e & 3)); };
    // what the stage holds for socket sck = 4*t + u at CN position p: edge u of VN t of position p - u (BPF:1712)
    auto stage_entry = [&](int p, uint32_t sck) -> uint16_t {
        const int u = (int)(sck & 3u), t = (int)(sck >> 2);
        if ((unsigned)(p - u) >= (unsigned)a.L) return (uint16_t)0xFFFFu;
        return CNMODE == 1 ? (uint16_t)((p - u) * a.vns_pos + t) : (uint16_t)sck;
    };

    // (the layout of a hist word while counting and after the scan: scan_hist, sampler_common.h)
    STAMP_DECL
    for (int b = tid; b < nb; b += kThreads) hist[b] = 0;
    if (tid == 0) { wsum[kWaves] = 0; wsum[kWaves + 1] = 0; }
    __syncthreads();
    auto sample_trial = [&](const int tr) {
    const unsigned long long trial = a.trial0 + (unsigned long long)tr;
    const uint32_t t_lo = (uint32_t)trial, t_hi = (uint32_t)(trial >> 32);
    // The keys of position p+1 are drawn (pure VALU) while the few worklist lanes of position p chase their bucket mates
    // through the LDS: nxt[] carries them across the barrier.
    // Thread t draws the keys of sockets 4t .. 4t+3 of every CN position, and socket 4t+i of CN position q+i is edge i of
    // VN (q, t) (BPF:1712): the row of a VN is assembled in its thread's registers over dv consecutive positions.
    // Entering step p: rowP = [edge 0 @ p-3 | edge 1 @ p-2], rowQ = [edge 0 @ p-2 | edge 1 @ p-1], rowR = [edge 0 @ p-1 | edge 2 @ p-1]
    uint32_t rowP[KMAX], rowQ[KMAX], rowR[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) rowP[k] = rowQ[k] = rowR[k] = 0;
    // The draw of position p is philox4x32_10(c0 = thread, c1 = p, c2 | c3 = trial, key = seed).  What its first rounds make
    // of the thread, the trial and the seed alone (philox.h: four words, three products) is computed once per trial; what
    // they make of the position, the trial and the seed is uniform and runs on the scalar unit: 15 vector products per
    // draw are left of 19.
    PhiloxPrefix pre[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) pre[k] = philox_prefix((uint32_t)(tid + k * kThreads), t_lo, t_hi, a.seed_lo, a.seed_hi);
    uint32_t nxt[E];
    {
        const PhiloxUniform un = philox_uniform(0u, t_lo, a.seed_lo, a.seed_hi);
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            uint32_t r[4] = {0, 0, 0, 0};
            if (own[k]) philox_tail(pre[k], un, a.seed_lo, a.seed_hi, r);
#pragma unroll
            for (int u = 0; u < 4; u++) nxt[4 * k + u] = r[u];
        }
    }
    for (int p = 0; p < a.D; p++) {
        STAMP(0);
        // ---- bucket histogram of this position's keys
        uint32_t key[E], slot[E], crowded = 0;
        // byte address of a key's word = (bucket >> 2) * 4, nibble shift = (bucket & 3) * 4: right shifts and masks only
        auto word_of = [](uint32_t k) { return (k >> KSHIFT) & ~3u; };
        auto nib_of = [](uint32_t k) { return (k >> (KSHIFT - 2)) & 12u; };
#pragma unroll
        for (int e = 0; e < E; e++) {
            key[e] = nxt[e];                                            // (threads without sockets hold zero keys and add zero)
            const uint32_t sh = nib_of(key[e]);
            uint32_t *w = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(hist) + word_of(key[e]));
            slot[e] = (atomicAdd(w, (own[e >> 2] ? 1u : 0u) << sh) >> sh) & 0xFu;
            if constexpr (!INCL) crowded = max(crowded, slot[e]);
        }
        // A bucket count must fit its nibble (0.24 keys per bucket on average: 15 in one never happens in practice) and the
        // straddlers their worklist: when either fails the position is ranked again by the exact fallback below — same
        // CN ids by construction, only slower — instead of trapping the process.  (INCL: a word of more than 15 keys,
        // which includes a wrapped nibble, makes that word's scanned total smaller than its true count, so the scan's
        // grand total falls short of S: one uniform compare for the whole position.)
        if (!INCL && crowded >= 15u) wsum[kWaves + 1] = 1u;
        __syncthreads();
        STAMP(1);

        // ---- exclusive scan of the bucket counts; false: the histogram's ranks do not hold (exact fallback)
        const bool ranked = scldpc_dev::scan_hist<ROWS, INCL>(hist, wsum, tid, lane, wave, S);
        STAMP(2);

        // ---- classify: every key gets rank g0 + arrival slot — any bijection onto its bucket's ranks gives the right CN
        //      (g0 / dc) when the bucket lies inside one block of dc ranks.  CN ids go into the ring, sockets into the
        //      rank-ordered stage.  Keys of buckets that span two CNs (3 %) are also put on a worklist for their true rank.
        // Worklist entry of a straddler: [bucket's end rank:16 | bucket's first rank:16], then its packed key
        // pk = key << LG | socket (also stored at its provisional rank in gpk, where its bucket mates meet it): bucket mates
        // share the key's top LG + 2 bits, so the shift drops none of the bits that order them.
        if (ranked) {                                                   // (an overflowed histogram has no ranks worth scattering by)
            uint32_t rk[E], g0a[E], g1a[E];
            bool st[E], sx[E];                                          // straddler; the same before the own[] mask (INCL)
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
                    sx[e] = ((g0a[e] ^ (g1a[e] - 1u)) >> DC_SHIFT) != 0u;
                    st[e] = own[e >> 2] && sx[e];
                }
            } else {
                scldpc_dev::bucket_ranges_excl<KSHIFT>(hist, key, [&](int e) { return own[e >> 2]; }, g0a, g1a);
#pragma unroll
                for (int e = 0; e < E; e++) {
                    rk[e] = g0a[e] + slot[e];
                    st[e] = own[e >> 2] && ((g1a[e] - 1u) >> DC_SHIFT) != (g0a[e] >> DC_SHIFT);
                }
            }
            if constexpr (INCL) {
                // the wave's straddlers (3 % of the keys) take consecutive worklist entries: ballots and one LDS atomic per
                // wave, no divergent loop.  The votes are the compares' own masks cut by the owners' mask (a ballot of
                // `own && straddles` goes through a VGPR and back).
                const unsigned long long ownv = __builtin_amdgcn_ballot_w64(own[0]);
                unsigned long long vote[E];
                int total = 0;
#pragma unroll
                for (int e = 0; e < E; e++) { vote[e] = __builtin_amdgcn_ballot_w64(sx[e]) & ownv; total += __builtin_popcountll(vote[e]); }
                if (total != 0) {
                    // (the first lane is found again from tid here, by an instruction the compiler cannot hoist: as a loop
                    // invariant its 64-bit lane mask is spilled to a VGPR lane under the 72-SGPR cap and costs two
                    // v_readlane per position)
                    uint32_t ln, got = 0;
                    asm volatile("v_and_b32 %0, 63, %1" : "=v"(ln) : "v"(tid));
                    if (ln == 0u) got = lds_add_rtn(&wsum[kWaves], (uint32_t)total);
                    int base = __builtin_amdgcn_readfirstlane((int)got);
                    // past the list's end nothing is written: the count still grows, and the exact fallback ranks the
                    // position (from the keys, not from gpk)
                    if (base + total <= kWorkCap) {
                        // entry w of the list as a word pair of the whole LDS: the list's offset rides in the scalar base
                        static_assert((Lay::off_wsum + 32) % 2 == 0, "the worklist starts on a word pair");
                        uint2 *wl2 = reinterpret_cast<uint2 *>(lds);
                        base += (Lay::off_wsum + 32) / 2;
#pragma unroll
                        for (int e = 0; e < E; e++) {
                            if (st[e]) {
                                const uint32_t w = __builtin_amdgcn_mbcnt_hi((uint32_t)(vote[e] >> 32),
                                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)vote[e], (uint32_t)base));
                                const uint32_t pk = (key[e] << LG) | sock(e);
                                gpk[rk[e]] = pk;
                                uint32_t *ent = reinterpret_cast<uint32_t *>(wl2 + w);
                                ent[0] = g0a[e] | (g1a[e] << 16);
                                ent[1] = pk;
                            }
                            base += __builtin_popcountll(vote[e]);
                        }
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
                uint2 v;
                v.x = (rk[4 * k] >> DC_SHIFT) | ((rk[4 * k + 1] >> DC_SHIFT) << 16);
                v.y = (rk[4 * k + 2] >> DC_SHIFT) | ((rk[4 * k + 3] >> DC_SHIFT) << 16);
                reinterpret_cast<uint2 *>(fix)[tid + k * kThreads] = v;
            }
            if constexpr (CNMODE != 0) {
#pragma unroll
                for (int k = 0; k < KMAX; k++) {
                    if (!own[k]) continue;
#pragma unroll
                    for (int u = 0; u < 4; u++) stage[rk[4 * k + u]] = stage_entry(p, sock(4 * k + u));
                }
            }
        }
        __syncthreads();
        STAMP(3);

        // ---- the worklist: true rank among the bucket mates; counters cleared for the next position
        {
            clear_hist_words<ROWS>(hist, tid);
            int nwork = (int)wsum[kWaves];                              // 3 % of S on average (<= 250 keys); the list holds 1024
            const bool exact = !ranked || nwork > kWorkCap || a.force_exact == p || a.force_exact == -2;
            if (exact) {
                // every key's true rank among all S keys, ties by socket (what the histogram path computes where it matters):
                // S comparisons per key — never taken in a real run, see above
                asm volatile("; ledger: cold");                         // (no instruction: tools/isa_ledger.py skips this path)
                nwork = 0;
#pragma unroll
                for (int e = 0; e < E; e++) if (own[e >> 2]) gpk[sock(e)] = key[e];
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
                for (int k = 0; k < KMAX; k++) {
                    if (!own[k]) continue;
                    uint2 v;
                    v.x = (xr[4 * k] >> DC_SHIFT) | ((xr[4 * k + 1] >> DC_SHIFT) << 16);
                    v.y = (xr[4 * k + 2] >> DC_SHIFT) | ((xr[4 * k + 3] >> DC_SHIFT) << 16);
                    reinterpret_cast<uint2 *>(fix)[tid + k * kThreads] = v;
                    if constexpr (CNMODE != 0) {
#pragma unroll
                        for (int u = 0; u < 4; u++) stage[xr[4 * k + u]] = stage_entry(p, sock(4 * k + u));
                    }
                }
            }
            scldpc_dev::resolve_worklist<LG, CNMODE != 0>(nwork, tid, wl, gpk, stage, fix, [&](uint32_t sck) { return stage_entry(p, sck); },
                                                          [](uint32_t r) { return r >> DC_SHIFT; });
        }
        if (p + 1 < a.D) {
            // the round keys are recomputed from the seed here (twenty scalar adds) rather than kept in twenty SGPRs across
            // the whole loop, which the 72-SGPR budget of two workgroups per CU would spill into VGPR lanes
            uint32_t k_lo = a.seed_lo, k_hi = a.seed_hi;
            uint32_t tl = t_lo;                                         // (likewise the trial: no product of it is kept either)
            asm volatile("" : "+s"(k_lo), "+s"(k_hi), "+s"(tl));
            const PhiloxUniform un = philox_uniform((uint32_t)(p + 1), tl, k_lo, k_hi);
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                uint32_t r[4] = {0, 0, 0, 0};
                if (own[k]) philox_tail(pre[k], un, k_lo, k_hi, r);
#pragma unroll
                for (int u = 0; u < 4; u++) nxt[4 * k + u] = r[u];
            }
        }
        __syncthreads();
        if (tid == 0) { wsum[kWaves] = 0; wsum[kWaves + 1] = 0; }        // read again only after the next two barriers
        STAMP(4);

        // ---- VN position q = p-dv+1 now has all its dv edges (BPF:1703-1716); CN position p its sockets
        const int qpos = p - (DV - 1);
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            // this step drew edge 0 of VN position p, edge 1 of p-1, edge 2 of p-2 and edge 3 of p-3 = qpos
            uint2 c = make_uint2(0u, 0u);                               // [edge 0 | edge 1], [edge 2 | edge 3] of this step
            if (own[k]) c = reinterpret_cast<const uint2 *>(fix)[tid + k * kThreads];
            if (qpos >= 0 && own[k]) {
                // (the offset inside a trial fits 32 bits: one scalar product, no high half to carry)
                const size_t j = (size_t)tr * a.n + (size_t)((uint32_t)qpos * (uint32_t)a.vns_pos + (uint32_t)(tid + k * kThreads));
                uint2 v;
                v.x = rowP[k];
                v.y = (rowR[k] >> 16) | (c.y & 0xFFFF0000u);
                reinterpret_cast<uint2 *>(a.vn_adj16)[j] = v;
            }
            rowP[k] = rowQ[k];
            rowQ[k] = (rowR[k] & 0xFFFFu) | (c.x & 0xFFFF0000u);
            rowR[k] = (c.x & 0xFFFFu) | (c.y << 16);
        }
        if constexpr (CNMODE != 0) {
            uint2 *dst = reinterpret_cast<uint2 *>(a.cn_adj16) + ((size_t)tr * a.D + p) * (size_t)(S >> 2);
            const uint2 *src = reinterpret_cast<const uint2 *>(stage);
            for (int w = tid; w < (S >> 2); w += kThreads) dst[w] = src[w];
        }
        STAMP(5);
    }

    // ---- channel: 32 VNs per output word, 8 Philox calls
    uint32_t *chan = a.chan + (size_t)tr * a.nw;
    const PhiloxUniform chun = philox_uniform(0x80000000u, t_lo, a.seed_lo, a.seed_hi);     // once per trial
    for (int w = tid; w < a.nw; w += kThreads) {
        uint32_t word = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            uint32_t r[4];
            philox_tail(philox_prefix((uint32_t)(w * 8 + c), t_lo, t_hi, a.seed_lo, a.seed_hi), chun, a.seed_lo, a.seed_hi, r);
#pragma unroll
            for (int u = 0; u < 4; u++) word |= channel_erased(r[u], a.thresh) << (c * 4 + u);
        }
        const int j0 = w * 32;
        word = channel_tail(word, j0, a.n);
        for (int d = 0; d < a.ndoped; d++) word = channel_undope(word, j0, a.doped[d], a.vns_pos);
        chan[w] = word;
    }
    STAMP(6);
    };
    // PERSIST (diagnostics): workgroup b samples trials b, b + gridDim.x, …; otherwise exactly one
    if constexpr (PERSIST) {
        for (int tr = blockIdx.x; tr < a.ntrials; tr += gridDim.x) {
            sample_trial(tr);
            __syncthreads();                            // the stage of the last position has been copied out
        }
    } else {
        sample_trial((int)blockIdx.x);
    }
    STAMP_FLUSH();
}


// ------------------------------------------------------------------------------------------------------------------------
// Third generation of the same sampler (same law, same Philox keys, same tables bit for bit), re-cut along what the gfx950
// vector unit and the barriers charge for (tools/calib/valu.hip, profiles/r03_valu_classes.txt):
//  * add / sub / and / or / xor / mov / right shifts / v_bitop3 issue at one wave-instruction per 2 cycles and SIMD; left
//    shifts, multiplies, every other three-operand form, v_cndmask, DPP, and ANY operation with a scalar-register source
//    take 4.  So the bucket geometry is a template parameter (shifts and masks become immediates, no SGPR operands), byte
//    addresses and nibble shifts are cut out of the key by right shifts and masks, and selects are avoided.
//  * three barriers per CN position instead of five: the histogram is double-buffered, so position p+1 is counted while the
//    straddlers of p are ranked (phase A); the prefix scan is wave-local — the 16 wave totals are added at look-up time
//    through a ds_bpermute instead of a second pass over the counters (phase B, beside the copy-out of position p-1); the
//    scan leaves INCLUSIVE nibble prefixes in the word, so a key's first rank and its bucket's size are two shifts and two
//    masks (phase C).
// hist word after the scan: [wave-local prefix:12 | i3 i2 i1 i0 : inclusive prefixes of the four bucket counters | 0:4].
// CNMODE 1: the VN that socket sck = 4*t + u of CN position p stands for (edge u of VN t of position p - u)
__device__ __forceinline__ uint32_t wl_entry_vn(const S2Args &a, int p, uint32_t sck)
{
    return (uint32_t)((p - (int)(sck & 3u)) * a.vns_pos + (int)(sck >> 2));
}

template <int LG, int CNMODE>
__global__ __launch_bounds__(kThreads, 8) __attribute__((amdgpu_num_sgpr(72))) void sample_philox_v3_kernel(const S2Args a)
{
    constexpr int DV = 4, DC_SHIFT = 3, E = 4;
    constexpr int NB = 1 << LG, ROWS = NB / kThreads;                   // histogram words (4 buckets each); words per thread
    constexpr int KSHIFT = 32 - LG - 2;                                 // key >> KSHIFT = fine bucket
    constexpr uint32_t LOWMASK = (1u << KSHIFT) - 1u;
    constexpr int SBITS = LG;
    static_assert(ROWS == 1 || ROWS == 2 || ROWS == 4, "one Philox call per thread: at most 4096 sockets per position");
    extern __shared__ uint32_t lds[];
    uint32_t *hist0 = lds;                                              // two buffers of NB words
    uint32_t *gpk = lds + a.off_gpk;
    uint16_t *fix = reinterpret_cast<uint16_t *>(lds + a.off_fix);
    uint16_t *stage = reinterpret_cast<uint16_t *>(lds + a.off_stage);
    uint32_t *wsum = lds + a.off_wsum;                                  // [0,16) wave totals, [16] worklist count, [18 + parity] overflow flags
    uint32_t *wl = wsum + 32;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S;
    const bool own = tid < (S >> 2);                                    // sockets 4*tid .. 4*tid + 3
    const unsigned long long trial = a.trial0 + blockIdx.x;
    const uint32_t t_lo = (uint32_t)trial, t_hi = (uint32_t)(trial >> 32);
    const int tr = blockIdx.x;

    STAMP_DECL
    for (int b = tid; b < 2 * NB; b += kThreads) hist0[b] = 0;
    if (tid < 32) wsum[tid] = 0;
    __syncthreads();

    uint32_t rowP = 0, rowQ = 0, rowR = 0;
    uint32_t key[E] = {0, 0, 0, 0}, slot[E] = {0, 0, 0, 0};
    // what the rank-ordered stage holds for this thread's socket 4*tid + u at the CN position being classified: the VN
    // (p - u) * V + tid (kept as one running register and V in a VGPR: subtractions with a scalar operand cost double)
    uint32_t ent0 = CNMODE == 1 ? (uint32_t)tid : (uint32_t)(4 * tid);
    uint32_t vV = (uint32_t)a.vns_pos;
    asm volatile("" : "+v"(vV));

    // Positions flow through three phases, one barrier each; iteration p runs A(p), B(p), C(p):
    //   A(p): count the keys of p into hist[p & 1]; rank the straddlers of p-1 (patching fix / stage of p-1); clear hist[(p-1) & 1]
    //   B(p): wave-local scan of hist[p & 1]; copy position p-1 out (VN rows from registers, CN rows from the stage)
    //   C(p): look every key of p up: CN ids into fix, sockets into the stage, straddlers onto the worklist
    for (int p = 0; p <= a.D; p++) {
        uint32_t *hc = hist0 + (p & 1) * NB, *hp = hist0 + ((p & 1) ^ 1) * NB;
        const bool live = p < a.D;
        STAMP(0);
        // ================================================ phase A ================================================
        if (p > 0) {
            // the worklist of p-1: true rank among the bucket mates (or, never in a real run, the exact fallback)
            int nwork = (int)wsum[16];
            const bool exact = wsum[18 + ((p - 1) & 1)] != 0u || nwork > kWorkCap || a.force_exact == p - 1 || a.force_exact == -2;
            if (exact) {
                uint32_t k2[4] = {0, 0, 0, 0};
                uint32_t f_lo = a.seed_lo, f_hi = a.seed_hi;
                asm volatile("" : "+s"(f_lo), "+s"(f_hi));              // (no round keys hoisted out of the position loop)
                if (own) philox4x32_10((uint32_t)tid, (uint32_t)(p - 1), t_lo, t_hi, f_lo, f_hi, k2);
                if (own) { gpk[4 * tid] = k2[0]; gpk[4 * tid + 1] = k2[1]; gpk[4 * tid + 2] = k2[2]; gpk[4 * tid + 3] = k2[3]; }
                __syncthreads();
                uint32_t xr[4] = {0, 0, 0, 0};
                for (int s2 = 0; s2 < S; s2++) {
                    const uint32_t kk = gpk[s2];
#pragma unroll
                    for (int u = 0; u < 4; u++) xr[u] += (kk < k2[u]) || (kk == k2[u] && s2 < 4 * tid + u);
                }
                if (own) {
                    uint2 v;
                    v.x = (xr[0] >> DC_SHIFT) | ((xr[1] >> DC_SHIFT) << 16);
                    v.y = (xr[2] >> DC_SHIFT) | ((xr[3] >> DC_SHIFT) << 16);
                    reinterpret_cast<uint2 *>(fix)[tid] = v;
                    if constexpr (CNMODE != 0) {
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const int pu = p - 1 - u;
                            stage[xr[u]] = (unsigned)pu < (unsigned)a.L ? (uint16_t)(CNMODE == 1 ? pu * a.vns_pos + tid : 4 * tid + u) : (uint16_t)0xFFFFu;
                        }
                    }
                }
                nwork = 0;
            }
            for (int w = tid; w < nwork; w += kThreads) {
                const uint32_t ea = wl[2 * w], pk = wl[2 * w + 1];
                const uint32_t g0 = ea & 0xFFFFu, cnt = (ea >> 16) & 0xFu, sl = (ea >> 20) & 0xFu;
                uint32_t r = g0;
                for (uint32_t m = 0; m < cnt; m++)
                    if (m != sl) r += gpk[g0 + m] < pk;
                const uint32_t sck = pk & ((1u << SBITS) - 1u);
                if constexpr (CNMODE != 0) stage[r] = (uint16_t)(ea >> 24 ? 0xFFFFu : (CNMODE == 1 ? wl_entry_vn(a, p - 1, sck) : sck));
                fix[sck] = (uint16_t)(r >> DC_SHIFT);
            }
            {   // the counters of p-1 are free: every look-up of phase C(p-1) lies behind the last barrier
                clear_hist_words<ROWS>(hp, tid);
            }
        }
        STAMP(1);                                                       // A: worklist of p-1 + clear
        if (live) {
            {   // the keys of p (threads without sockets hold zero keys and add zero); the round keys are recomputed by
                // scalar adds rather than held in twenty SGPRs across the loop
                uint32_t k_lo = a.seed_lo, k_hi = a.seed_hi;
                asm volatile("" : "+s"(k_lo), "+s"(k_hi));
                uint32_t r[4] = {0, 0, 0, 0};
                if (own) philox4x32_10((uint32_t)tid, (uint32_t)p, t_lo, t_hi, k_lo, k_hi, r);
#pragma unroll
                for (int u = 0; u < 4; u++) key[u] = r[u];
            }
            uint32_t crowded = 0;
#pragma unroll
            for (int e = 0; e < E; e++) {
                // byte address of the word = (bucket >> 2) * 4, nibble shift = (bucket & 3) * 4: right shifts and masks only
                const uint32_t boff = (key[e] >> KSHIFT) & ~3u, sh = (key[e] >> (KSHIFT - 2)) & 12u;
                const uint32_t old = atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(hc) + boff), (own ? 16u : 0u) << sh);
                slot[e] = (old >> (sh + 4u)) & 0xFu;
                crowded |= slot[e] + 1u;
            }
            if (crowded & 16u) wsum[18 + (p & 1)] = 1u;                 // a bucket met its 16th key: its nibble wrapped
        }
        STAMP(2);                                                       // A: keys + histogram
        __syncthreads();
        STAMP(3);                                                       // barrier wait
        // ================================================ phase B ================================================
        if (tid == 0) { wsum[16] = 0; wsum[18 + ((p & 1) ^ 1)] = 0; }  // worklist count and the flag of p-1: consumed in phase A
        if (live) {
            uint32_t x[ROWS], tot = 0, over = 0;
            load_hist_words<ROWS>(hc, tid, x);
            uint32_t v[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                // counters sit in bits [4, 20): c0..c3.  Inclusive prefixes by one multiply (valid while the word's total <= 15)
                const uint32_t y = x[r] * 0x1111u;                      // nibble k of bits [4, 20) = c0 + .. + ck
                const uint32_t sb = (x[r] & 0x0F0F0u) + ((x[r] >> 4) & 0x0F0F0u);
                v[r] = ((sb + (sb >> 8)) >> 4) & 0xFFu;                  // the true total (two byte sums <= 30 each)
                over |= v[r];
                x[r] = y & 0xFFFF0u;
                tot += v[r];
            }
            if (over & ~15u) wsum[18 + (p & 1)] = 1u;                   // sixteen keys in four adjacent buckets: exact fallback
            const uint32_t inc = wave_inclusive_scan(tot);
            uint32_t pre = inc - tot;
#pragma unroll
            for (int r = 0; r < ROWS; r++) { x[r] |= pre << 20; pre += v[r]; }
            store_hist_words<ROWS>(hc, tid, x);
            if (lane == 63) wsum[wave] = inc;
        }
        if (p > 0) {
            // ---- VN position q = p-1-dv+1 now has all its dv edges (BPF:1703-1716); CN position p-1 its sockets
            const int pp = p - 1, qpos = pp - (DV - 1);
            uint2 c = make_uint2(0u, 0u);                               // [edge 0 | edge 1], [edge 2 | edge 3] of step pp
            if (own) c = reinterpret_cast<const uint2 *>(fix)[tid];
            if (qpos >= 0 && own) {
                const size_t j = (size_t)tr * a.n + (size_t)qpos * a.vns_pos + (size_t)tid;
                uint2 vv;
                vv.x = rowP;
                vv.y = (rowR >> 16) | (c.y & 0xFFFF0000u);
                reinterpret_cast<uint2 *>(a.vn_adj16)[j] = vv;
            }
            rowP = rowQ;
            rowQ = (rowR & 0xFFFFu) | (c.x & 0xFFFF0000u);
            rowR = (c.x & 0xFFFFu) | (c.y << 16);
            if constexpr (CNMODE != 0) {
                uint2 *dst = reinterpret_cast<uint2 *>(a.cn_adj16) + ((size_t)tr * a.D + pp) * (size_t)(S >> 2);
                const uint2 *src = reinterpret_cast<const uint2 *>(stage);
                if (own) dst[tid] = src[tid];
            }
        }
        STAMP(4);                                                       // B: scan + copy-out
        __syncthreads();
        STAMP(5);                                                       // barrier wait
        // ================================================ phase C ================================================
        if (live && wsum[18 + (p & 1)] == 0u) {
            // exclusive prefix of the 16 wave totals, in lanes 0..15 of every wave; a key's wave is its top four bits
            const uint32_t wt = lane < kWaves ? wsum[lane] : 0u;
            uint32_t wi = wt;
            wi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)wi, 0x111, 0xF, 0xF, false);
            wi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)wi, 0x112, 0xF, 0xF, false);
            wi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)wi, 0x114, 0xF, 0xF, false);
            wi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)wi, 0x118, 0xF, 0xF, false);
            const uint32_t wex = wi - wt;
            uint32_t h[E], wb[E], rk[E], g0a[E], cnta[E];
#pragma unroll
            for (int e = 0; e < E; e++) h[e] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(hc) + ((key[e] >> KSHIFT) & ~3u));
#pragma unroll
            for (int e = 0; e < E; e++) wb[e] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((key[e] >> 26) & 0x3Cu), (int)wex);
            bool st[E];
            bool anyst = false;
#pragma unroll
            for (int e = 0; e < E; e++) {
                const uint32_t t1 = h[e] >> ((key[e] >> (KSHIFT - 2)) & 12u);   // [.. | incl | excl]
                const uint32_t excl = t1 & 15u, incl = (t1 >> 4) & 15u;
                g0a[e] = (h[e] >> 20) + wb[e] + excl;
                cnta[e] = incl - excl;
                rk[e] = g0a[e] + slot[e];
                st[e] = own && ((g0a[e] ^ (g0a[e] + cnta[e] - 1u)) >> DC_SHIFT) != 0u;
                anyst = anyst || st[e];
            }
            if (own) {
                uint2 vv;                                                // provisional CN ids (final unless on the worklist)
                vv.x = (rk[0] >> DC_SHIFT) | ((rk[1] >> DC_SHIFT) << 16);
                vv.y = (rk[2] >> DC_SHIFT) | ((rk[3] >> DC_SHIFT) << 16);
                reinterpret_cast<uint2 *>(fix)[tid] = vv;
            }
            // chain ends: sockets of VN positions outside [0, L) stand for no VN (BPF:1703-1716)
            const bool edge = p < DV - 1 || p >= a.L;
            if constexpr (CNMODE != 0) {
                if (own) {
                    uint32_t ent[E];
                    ent[0] = ent0;
#pragma unroll
                    for (int u = 1; u < 4; u++) ent[u] = CNMODE == 1 ? ent[u - 1] - vV : ent[u - 1] + 1u;
                    if (!edge) {
#pragma unroll
                        for (int u = 0; u < 4; u++) stage[rk[u]] = (uint16_t)ent[u];
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; u++) stage[rk[u]] = (unsigned)(p - u) < (unsigned)a.L ? (uint16_t)ent[u] : (uint16_t)0xFFFFu;
                    }
                }
            }
            if (__builtin_amdgcn_ballot_w64(anyst)) {
                // the wave's straddlers take consecutive worklist entries: one LDS atomic per wave, no select chains
                unsigned long long vote[E];
                int total = 0;
#pragma unroll
                for (int e = 0; e < E; e++) { vote[e] = __builtin_amdgcn_ballot_w64(st[e]); total += __builtin_popcountll(vote[e]); }
                int base = 0;
                if (lane == 0) base = atomicAdd(reinterpret_cast<int *>(&wsum[16]), total);
                base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if (st[e]) {
                        const int w = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(vote[e] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vote[e], 0u));
                        const uint32_t pk = ((key[e] & LOWMASK) << SBITS) | (uint32_t)(4 * tid + e);
                        gpk[g0a[e] + slot[e]] = pk;
                        const uint32_t none = CNMODE != 0 && edge && !((unsigned)(p - e) < (unsigned)a.L) ? 1u : 0u;
                        if (w < kWorkCap) { wl[2 * w] = g0a[e] | (cnta[e] << 16) | (slot[e] << 20) | (none << 24); wl[2 * w + 1] = pk; }
                    }
                    base += __builtin_popcountll(vote[e]);
                }
            }
        }
        if constexpr (CNMODE == 1) ent0 += vV;                           // the VN of socket 0 moves one position on
        STAMP(6);                                                       // C: classify
        __syncthreads();
        STAMP(7);                                                       // barrier wait
    }

    // ---- channel: 32 VNs per output word, 8 Philox calls
    uint32_t *chan = a.chan + (size_t)tr * a.nw;
    for (int w = tid; w < a.nw; w += kThreads) {
        uint32_t word = 0;
        uint32_t c_lo = a.seed_lo, c_hi = a.seed_hi;
        asm volatile("" : "+s"(c_lo), "+s"(c_hi));
#pragma unroll
        for (int c = 0; c < 8; c++) {
            uint32_t r[4];
            philox4x32_10((uint32_t)(w * 8 + c), 0x80000000u, t_lo, t_hi, c_lo, c_hi, r);
#pragma unroll
            for (int u = 0; u < 4; u++) word |= channel_erased(r[u], a.thresh) << (c * 4 + u);
        }
        const int j0 = w * 32;
        word = channel_tail(word, j0, a.n);
        for (int d = 0; d < a.ndoped; d++) word = channel_undope(word, j0, a.doped[d], a.vns_pos);
        chan[w] = word;
    }
    STAMP(8);                                                           // channel
    STAMP_FLUSH();
}

int launch_v2(const char *who, int cnmode, const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
              double eps, int32_t ndoped, const int32_t *doped_positions, uint16_t *d_vn_adj16, uint16_t *d_table,
              uint32_t *d_chan_bits, void *stream)
{
    S2Args a{};
    if (int rc = scldpc::check_sample_call(who, p, ntrials < 0 || (ntrials > 0 && (!d_vn_adj16 || !d_chan_bits)), ntrials, eps,
                                           ndoped, doped_positions, &a.ndoped, a.doped)) return rc;
    if (ntrials == 0) return SCLDPC_OK;
    if (!d_table) cnmode = 0;

    a.L = p->L; a.cns_pos = p->cns_pos; a.vns_pos = p->vns_pos;
    a.n = scldpc::n_of(p); a.S = p->cns_pos * p->dc; a.D = p->L + p->dv - 1; a.nw = scldpc::nw_of(p);
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.thresh = scldpc::erasure_threshold(eps);
    // Third generation (one Philox call per thread: at most 4096 sockets per position; two histogram buffers): measured equal to
    // the second within +-4 % at N = 1000 (faster without the CN table and at N <= 512, slower with it: DESIGN.md §5), so
    // it is opt-in (SCLDPC_SAMPLER_GEN=3) and the second generation stays the default.
    const char *gen_env = getenv("SCLDPC_SAMPLER_GEN");
    const bool one_call = a.S <= 4 * kThreads;              // nb <= 4096
    const bool v3 = one_call && gen_env && atoi(gen_env) == 3;
    // the second generation's one-call instances address their regions by V2Layout's immediates: sized for nb sockets rather than S
    int lg;
    size_t lds_bytes;
    if (int rc = scldpc::v2_lds_layout(who, a.S, v3 ? 2 : 1, one_call && !v3, cnmode != 0, &a, &lg, &lds_bytes)) return rc;
    a.vn_adj16 = d_vn_adj16; a.cn_adj16 = d_table; a.chan = d_chan_bits;
    a.ntrials = ntrials;

    using Kern = void (*)(const S2Args);
    static const Kern table[4][3] = {
        {sample_philox_v2_kernel<1, 1, 0>, sample_philox_v2_kernel<1, 1, 1>, sample_philox_v2_kernel<1, 1, 2>},
        {sample_philox_v2_kernel<1, 2, 0>, sample_philox_v2_kernel<1, 2, 1>, sample_philox_v2_kernel<1, 2, 2>},
        {sample_philox_v2_kernel<1, 4, 0>, sample_philox_v2_kernel<1, 4, 1>, sample_philox_v2_kernel<1, 4, 2>},
        {sample_philox_v2_kernel<2, 8, 0>, sample_philox_v2_kernel<2, 8, 1>, sample_philox_v2_kernel<2, 8, 2>},
    };
    const int rows = a.nb / kThreads;                       // 1, 2, 4 (one Philox call per thread) or 8 (two)
    static const Kern table3[3][3] = {
        {sample_philox_v3_kernel<10, 0>, sample_philox_v3_kernel<10, 1>, sample_philox_v3_kernel<10, 2>},
        {sample_philox_v3_kernel<11, 0>, sample_philox_v3_kernel<11, 1>, sample_philox_v3_kernel<11, 2>},
        {sample_philox_v3_kernel<12, 0>, sample_philox_v3_kernel<12, 1>, sample_philox_v3_kernel<12, 2>},
    };
    const int grid = v3 ? ntrials : scldpc::debug_grid("SAMPLER", ntrials);
    Kern kern = v3 ? table3[lg - 10][cnmode] : table[rows == 1 ? 0 : rows == 2 ? 1 : rows == 4 ? 2 : 3][cnmode];
    if (grid < ntrials && rows == 4 && cnmode == 1) kern = sample_philox_v2_kernel<1, 4, 1, true>;     // diagnostics: persistent launch
    else if (grid < ntrials) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "SCLDPC_DEBUG_GRID_SAMPLER: only the <1,4,1> kernel has a persistent form");
    if (int rc_ = scldpc::allow_max_lds(reinterpret_cast<const void *>(kern))) return rc_;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds_bytes, static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

bool v2_shape(const scldpc_code_params *p)
{
    if (scldpc::check_params(p)) return false;
    const int S = p->cns_pos * p->dc;
    return p->dv == 4 && p->dc == 8 && (S & 3) == 0 && S <= 8192 && p->vns_pos * p->dv == S;
}

}  // namespace

// 1 when scldpc_sample_philox_device_cn16 takes this ensemble, else 0 (callers then use scldpc_sample_philox_device_adj16)
extern "C" int scldpc_sample_philox_cn16_supported(const scldpc_code_params *p)
{
    return v2_shape(p) && scldpc::n_of(p) < 65535;
}

// 1 when scldpc_sample_philox_device_sock16 takes this ensemble (any chain length: the table holds sockets, not VNs)
extern "C" int scldpc_sample_philox_sock16_supported(const scldpc_code_params *p)
{
    return v2_shape(p);
}

extern "C" int scldpc_sample_philox_device_cn16(const scldpc_code_params *p, uint64_t seed, uint64_t trial0,
                                                int32_t ntrials, double eps, int32_t ndoped,
                                                const int32_t *doped_positions, uint16_t *d_vn_adj16,
                                                uint16_t *d_cn_adj16, uint32_t *d_chan_bits, void *stream)
{
    const char *who = "scldpc_sample_philox_device_cn16";
    if (int rc = scldpc::check_params(p)) return rc;
    if (!scldpc_sample_philox_cn16_supported(p))
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: takes dv = 4, dc = 8, at most 8192 sockets per position and "
                                 "fewer than 65535 VNs (got dv=%d dc=%d cns_pos=%d n=%d)", who, p->dv, p->dc, p->cns_pos,
                                 scldpc::n_of(p));
    return launch_v2(who, 1, p, seed, trial0, ntrials, eps, ndoped, doped_positions, d_vn_adj16, d_cn_adj16, d_chan_bits,
                     stream);
}

extern "C" int scldpc_sample_philox_device_sock16(const scldpc_code_params *p, uint64_t seed, uint64_t trial0,
                                                  int32_t ntrials, double eps, int32_t ndoped,
                                                  const int32_t *doped_positions, uint16_t *d_vn_adj16,
                                                  uint16_t *d_cn_sock16, uint32_t *d_chan_bits, void *stream)
{
    const char *who = "scldpc_sample_philox_device_sock16";
    if (int rc = scldpc::check_params(p)) return rc;
    if (!scldpc_sample_philox_sock16_supported(p))
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: takes dv = 4, dc = 8 and at most 8192 sockets per position "
                                 "(got dv=%d dc=%d cns_pos=%d)", who, p->dv, p->dc, p->cns_pos);
    return launch_v2(who, 2, p, seed, trial0, ntrials, eps, ndoped, doped_positions, d_vn_adj16, d_cn_sock16, d_chan_bits,
                     stream);
}
