// Sweep peeling + stopping-set statistics (simulate_sc_ldpc's loop body, PD:650-691) with 4 bits of LDS per check node — gfx950.
//
// peel_sweep.hip keeps a 16- or 32-bit word per CN and gives a trial a 1024-thread workgroup: two trials per CU at most.  Its
// frontier machine is full_bp.hip's, and this file is to it what full_bp_small.hip is to full_bp.hip: a CN keeps ONLY its
// count of erased neighbours (a nibble); when the count drops to one the CN's dc sockets are read from the CN -> socket table
// (scldpc_sample_philox_device_sock16 / _deg_sock16 / scldpc_cn_sockets_device) and the one neighbour whose bit in the
// erased-VN bitmap U is still set is released.  A 256-thread workgroup decodes a trial and up to seven share a CU.
//
// The peeling is full_bp_small.hip's fixpoint branch (scan -> shared queue while the frontier is wide -> private per-wave
// queues below kSwitchWidth; every release claims its VN in U BEFORE it decrements the VN's CNs, see there), copied, not
// shared: its lambdas close over the kernel's state, and that kernel's template list is long enough.  What the sweep adds:
//   * cn_lim is the caller's total_size, anything in [0, nk]: CNs at or above it are counted, never fire, never enter a queue;
//   * a CN below sweep_start that holds one VN from the outset never fires (PD:273-277).  Those are written to `frozen` (one
//     bit per CN below min(sweep_start, total_size)) before anything is released, and every scan leaves out exactly those.
//     A frozen CN cannot be queued by a 2 -> 1 transition, so only the scans need the rule;
//   * a scan is walked a queue-full at a time from per-wave cursors, and what a wave's private half-queue cannot take spills to
//     the idle queue: at the shipped sizes the first frontier is longer than a queue (1170 CNs for 768 entries at (4,8), L = 50,
//     M = 1000) and a wave's private frontier longer than its half-queue, and neither costs a second scan.  Only entries a full
//     queue DROPS start one (column 6 counts them);
//   * lost set (PD:659-666): U := U AND lost, VN j lost iff one of its CNs lies in [lost_lo, lost_hi) and all lie below total_size;
//   * components (PD:677-691, extract_stopping_sets PD:1077-1095): only "is this VN's component larger than two" is asked,
//     a local question (peel_sweep.hip's header): the nibbles are recounted over the lost VNs alone, and VN a sits in a larger
//     component iff one of its CNs counts >= 3, or its count-2 CNs name two different partners, or its single partner b has a
//     CN counting >= 3 or a partner other than a.  The partner at a count-2 CN is the other socket of its row whose U bit is set.
// The residual of the peeling does not depend on its order, so rows and lost bits equal peel_sweep_kernel's bit for bit.
//
// The WIDE form (scldpc_peel_sweep_device_sock16_wide) is the same kernel for trials of more than 65 536 CNs: queue entries are
// 32-bit CN ids, and one 1024-thread workgroup (16 waves, four per SIMD, at most 128 VGPRs) owns the CU's LDS, one trial per CU.
// Its carve (make_args with wide = true), in this order and each region rounded up to 16 bytes:
//     ceil(nk / 8) count words | ceil(n / 32) VN words | ceil(fz_lim / 8) frozen bytes | L position flags | 16 scalars
// and then two queues that share what is left of 160 KiB - 512 B evenly, in 32-bit entries, with no upper cap.  The shape rule
// (wide_shape_limit; host side, pure): the pairs (3,6), (4,8), (5,10); vns_pos * dv <= 65 535 (16-bit sockets) and cns_pos <=
// 65 536 (16-bit position-local CN ids); an exact multiply-high division for vns_pos and cns_pos (magic_of); and at least
// kWideMinQueue = 1024 entries per queue.  No lower bound on nk: small shapes run through it too.  (4,8), L = 50, M = 5000 keeps
// about 8 000 entries per queue; (4,8), L = 90, M = 5000 (172.5 KB of state) is refused.
// The 16-wave private-queue phase: the waves go private below kSwitchWidthWide = 512 frontier entries, 32 per wave as in the
// narrow form (128 over four waves).  Wave v's part of the idle queue is wcap = (qcap / 16) & ~1 entries, two halves of
// half_cap = wcap / 2 between which its levels alternate; it takes entries v, v + 16, ... (at most 32) into the first half, so
// the phase needs half_cap >= 32 (the narrow form asks 64 of its four waves), which every supported shape has (qcap >= 1024).
// What a half cannot take spills behind the first 512 entries of the queue being read, as in the narrow form.
//
// The TAIL-BITING form (TB; scldpc_peel_sweep_device_sock16_tb / _tb_wide, include/scldpc_ensembles.h) is the same kernel on a
// chain closed into a ring: edge i of VN position q lies in CN position (q + i) mod L, socket dv * t + i of a CN of position pc
// belongs to VN position (pc - i) mod L, and every CN of positions 0 .. L - 1 has dc sockets.  Only the four places that turn a VN
// position plus an edge index into a CN position or back know it — the build, the release step, the lost pass, the
// neighbourhood — and each wraps with a compare and an add (L >= dv: one wrap at most).  The CNs of positions L .. L + dv - 2
// exist (nk and total_size are the chain's) and count zero.  The position flagged for a component stays the VN's own, j / vns_pos:
// edge 0 of a row lies in CN position q, which is the position peel_sweep.hip flags from the int32 rows.
#include "common.h"
#include "kernel_util.h"
#include "table_rows.h"
#include "../../include/scldpc_ensembles.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

using namespace scldpc_dev;

constexpr int kBlock = 256;             // threads per trial
constexpr int kPerCu = 7;               // workgroups per CU the LDS carve aims at (SGPRs <= 96, VGPRs <= 72)
constexpr int kRingPerCu = 4;           // the same for the tail-biting instances (instance_of)
constexpr int kSwitchWidth = 128;       // frontier entries below which the waves go private
constexpr int kMinQueueWords = 128;     // a queue shorter than 256 entries is no fast path: take fewer workgroups per CU
constexpr int kMinDebugQcap = 8;        // floor of SCLDPC_DEBUG_SWEEP_QCAP
constexpr int kBlockWide = 1024;        // the wide form: one workgroup per CU, four waves per SIMD
constexpr int kSwitchWidthWide = 512;   // 32 frontier entries per wave, as kSwitchWidth
constexpr int kWideMinQueue = 1024;     // entries per queue below which the wide form refuses the shape
static_assert(kSwitchWidth <= 64 * (kBlock / 64), "a wave takes at most one frontier entry per lane into its private queue");
static_assert(kSwitchWidthWide <= 64 * (kBlockWide / 64), "a wave takes at most one frontier entry per lane into its private queue");

enum { S_NE = 0, S_N0, S_N1, S_OVF, S_Q, S_MORE, S_ANY, S_LOST, S_EXP, S_BLK, S_N = 16 };

struct SwArgs {
    int L, V, C, n, nk, nw, ncw;                    // ncw = words of 8 count nibbles
    int cn_lim, fz_lim, lost_lo, lost_hi;           // cn_lim = total_size; fz_lim = min(sweep_start, total_size)
    uint32_t magic_v, magic_c;
    int kswitch;
    int off_U, off_fz, off_q0, off_q1, off_pos, off_scal, total, qcap;      // LDS offsets in 32-bit words; qcap in queue entries
    const uint16_t *vn_adj16;                       // [T][n][dv]  CN index local to its position
    const uint16_t *cn_sock16;                      // [T][nk][dc] sockets dv*t + i of every CN (0xFFFF: none)
    const uint32_t *chan;
    int32_t *out;                                   // [T][8]: lost, lost_exp, positions flagged, 0, 0, rounds, re-scans, #erased
    uint32_t *lost_out;                             // optional [T][nw]
};

// bit k of a byte <-> bit 4k (one per count nibble)
__device__ __forceinline__ uint32_t pack8(uint32_t y)
{
    y &= 0x11111111u;
    y = (y | (y >> 3)) & 0x03030303u;
    y = (y | (y >> 6)) & 0x000F000Fu;
    return (y | (y >> 12)) & 0xFFu;
}
__device__ __forceinline__ uint32_t spread8(uint32_t b)
{
    b = (b | (b << 12)) & 0x000F000Fu;
    b = (b | (b << 6)) & 0x03030303u;
    return (b | (b << 3)) & 0x11111111u;
}

// DV, DC: the degree pair, fixed at compile time (the rows of both tables are unrolled; table_rows.h).
// OCC: waves per SIMD the registers are bounded for where an instance cannot hold kPerCu (0: kPerCu).
// WIDE: 32-bit queue entries and a 1024-thread workgroup, one per CU (the header comment).
// TB: the chain is a ring of L positions (the header comment); resolved at compile time, the chain's instances keep their code.
template <int DV, int DC, int OCC = 0, bool WIDE = false, bool TB = false>
__global__ __launch_bounds__(WIDE ? kBlockWide : kBlock, WIDE ? kBlockWide / 256 : OCC ? OCC : kPerCu) __attribute__((amdgpu_num_sgpr(96)))
void peel_sweep_small_kernel(const SwArgs a)
{
    static_assert(DC <= 15 && DC % 2 == 0 && DV < DC, "a CN's count of erased neighbours is a nibble; CN rows are read as 32-bit words");
    constexpr int BLOCK = WIDE ? kBlockWide : kBlock, kWaves = BLOCK / 64;
    constexpr int kMinHalf = WIDE ? kSwitchWidthWide / kWaves : 64;      // a wave's half-queue below this keeps the waves shared
    using QT = std::conditional_t<WIDE, uint32_t, uint16_t>;
    extern __shared__ uint32_t lds[];
    uint32_t *cnt = lds;                                                 // nk nibbles
    uint32_t *U = lds + a.off_U;
    uint8_t *fz = reinterpret_cast<uint8_t *>(lds + a.off_fz);           // frozen: byte w = the CNs of count word w
    QT *q[2] = {reinterpret_cast<QT *>(lds + a.off_q0), reinterpret_cast<QT *>(lds + a.off_q1)};
    int *pos_flag = reinterpret_cast<int *>(lds + a.off_pos);
    int *scal = reinterpret_cast<int *>(lds + a.off_scal);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int trial = blockIdx.x;
    const int n = a.n, nk = a.nk, cn_lim = a.cn_lim, nw = a.nw, V = a.V, C = a.C, qcap = a.qcap;
    const auto *vrow = reinterpret_cast<const typename VnUnit<DV>::type *>(a.vn_adj16) + (size_t)trial * n * VnUnit<DV>::per_row;
    const auto *crow = reinterpret_cast<const typename CnUnit<DC>::type *>(a.cn_sock16) + (size_t)trial * nk * CnUnit<DC>::per_row;
    auto vn_row = [&](int j) { if constexpr (DV == 4) return load_row(vrow, j); else return load_row<DV>(vrow, j); };
    auto cn_row = [&](int c) { if constexpr (DC == 8) return load_row(crow, c); else return load_row<DC>(crow, c); };
    auto u_bit = [&](int j) { return (U[j >> 5] >> (j & 31)) & 1u; };
    auto count_of = [&](int c) { return (cnt[c >> 3] >> ((c & 7) * 4)) & 15u; };
    const uint32_t *ch = a.chan + (size_t)trial * nw;
    // CN of edge i of a VN whose position starts at CN `base` = position * C (l: the row's position-local id); on the ring a CN
    // position at or beyond L wraps by -L
    auto cn_of_edge = [&](int base, int i, int l) {
        if constexpr (TB) {
            int c = base + i * C;
            if (c >= a.L * C) c -= a.L * C;
            return c + l;
        } else {
            return base + i * C + l;
        }
    };

    // ---- channel bits, clear the counts -------------------------------------------------------------------------
    for (int c = tid; c < a.ncw; c += BLOCK) cnt[c] = 0;
    int ne_local = 0;
    for (int w = tid; w < nw; w += BLOCK) {
        const uint32_t x = chan_tail(ch[w], w, nw, n);
        U[w] = x;
        ne_local += __popc(x);
    }
    if (tid < S_N) scal[tid] = 0;
    for (int i = tid; i < a.L; i += BLOCK) pos_flag[i] = 0;
    __syncthreads();
    ne_local = wave_sum(ne_local);
    if (lane == 0 && ne_local) atomicAdd(&scal[S_NE], ne_local);

    // ---- build: every erased VN counts itself into its DV CNs; rows are loaded unconditionally (coalesced loads) -------
    constexpr int NB = 8;                                                // rows in flight per thread
    for (int j0 = tid; j0 < n; j0 += NB * BLOCK) {
        Row<DV> r[NB];
        bool er[NB];
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int j = j0 + u * BLOCK;
            er[u] = false;
            if (j < n) { r[u] = vn_row(j); er[u] = u_bit(j); }
        }
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int j = j0 + u * BLOCK;
            if (er[u]) {
                const int base = (int)__umulhi((uint32_t)j, a.magic_v) * C;
                int cc[DV];
#pragma unroll
                for (int i = 0; i < DV; i++) cc[i] = cn_of_edge(base, i, (int)r[u][i]);
#pragma unroll
                for (int i = 0; i < DV; i++) atomicAdd(&cnt[cc[i] >> 3], 1u << ((cc[i] & 7) * 4));
            }
        }
    }
    __syncthreads();

    // ---- one release step: CN c is believed to have exactly one erased neighbour -----------------------------------
    // out[i] = 1 + the CN on edge i of the released VN if this release left it with one erased neighbour, else 0
    auto step = [&](int c, uint32_t (&out)[DV]) {
#pragma unroll
        for (int i = 0; i < DV; i++) out[i] = 0;
        const Row<DC> s = cn_row(c);
        uint32_t jk[DC];
        bool none[DC];
#pragma unroll
        for (int k = 0; k < DC; k++) { jk[k] = s[k]; none[k] = jk[k] == 0xFFFFu; }
        const int vbase = (int)__umulhi((uint32_t)c, a.magic_c) * V;     // CN position * V; socket s = DV * t + i -> global VN index
#pragma unroll
        for (int k = 0; k < DC; k++) {
            if constexpr (TB) {                                          // a VN position below 0 wraps by +L (n = L * V)
                int vb = vbase - (int)(jk[k] % DV) * V;
                if (vb < 0) vb += n;
                jk[k] = (uint32_t)vb + (jk[k] / DV);
            } else {
                jk[k] = (uint32_t)(vbase - (int)(jk[k] % DV) * V) + (jk[k] / DV);
            }
        }
        uint32_t wd[DC];
#pragma unroll
        for (int k = 0; k < DC; k++) wd[k] = U[none[k] ? 0u : jk[k] >> 5];              // no VN: any word, masked below
        int j = -1;
#pragma unroll
        for (int k = 0; k < DC; k++)
            if (!none[k] && ((wd[k] >> (jk[k] & 31u)) & 1u)) j = (int)jk[k];
        if (j < 0) return;                                               // its last neighbour is being released elsewhere
        const Row<DV> r = vn_row(j);                                     // issued before the claim: overlaps its round trip
        const uint32_t bit = 1u << (j & 31);
        if (!(atomicAnd(&U[j >> 5], ~bit) & bit)) return;
        const int base = (int)__umulhi((uint32_t)j, a.magic_v) * C;
        int cc[DV];
#pragma unroll
        for (int i = 0; i < DV; i++) cc[i] = cn_of_edge(base, i, (int)r[i]);
        uint32_t o[DV];
#pragma unroll
        for (int i = 0; i < DV; i++) o[i] = atomicSub(&cnt[cc[i] >> 3], 1u << ((cc[i] & 7) * 4));
#pragma unroll
        for (int i = 0; i < DV; i++) {
            const uint32_t old = (o[i] >> ((cc[i] & 7) * 4)) & 15u;
            if (old == 2u && cc[i] < cn_lim) out[i] = (uint32_t)cc[i] + 1u;             // transition to one VN: may fire (PD:305-308)
        }
    };
    // the CNs of a count word that a scan takes, as a mask of the nibbles' top bits: count one, below cn_lim, and not frozen.
    auto ones_of = [&](int w) {
        const uint32_t y = cnt[w] ^ 0x11111111u;                         // nibble == 1  <=>  zero nibble of y
        uint32_t z = ~(((y & 0x77777777u) + 0x77777777u) | y) & 0x88888888u;
        if (w * 8 + 8 > cn_lim) {                                        // the word that holds cn_lim
            const int keep = cn_lim - w * 8;
            z = keep <= 0 ? 0u : (z & ((1u << (4 * keep)) - 1u));
        }
        return z;
    };
    auto scan_word = [&](int w) {
        uint32_t z = ones_of(w);
        if (w * 8 < a.fz_lim) z &= ~(spread8(fz[w]) << 3);
        return z;
    };
    // What is frozen is decided before anything is released: count one from the outset and below sweep_start (PD:273-277).
    // (A scan walks the count words a queue-full at a time, so later parts of it see counts that releases have changed.)
    for (int w = tid; w * 8 < a.fz_lim; w += BLOCK) {
        const int below = a.fz_lim - w * 8;
        const uint32_t z = ones_of(w);
        fz[w] = (uint8_t)pack8((below >= 8 ? z : (z & ((1u << (4 * below)) - 1u))) >> 3);
    }
    __syncthreads();
    // a wave appends its lanes' out[] entries to queue qn behind *push (one prefix scan + one LDS atomic per wave)
    auto append = [&](const uint32_t (&out)[DV], int *push, QT *qn, bool &overflow) {
        int mine = 0;
#pragma unroll
        for (int i = 0; i < DV; i++) mine += out[i] != 0u;
        const int incl = (int)wave_inclusive_scan((uint32_t)mine);
        const int tot = __builtin_amdgcn_readlane(incl, 63);
        if (tot) {
            int base = 0;
            if (lane == 0) base = atomicAdd(push, tot);
            int idx = __builtin_amdgcn_readfirstlane(base) + incl - mine;
#pragma unroll
            for (int i = 0; i < DV; i++)
                if (out[i]) { if (idx < qcap) qn[idx] = (QT)(out[i] - 1u); else overflow = true; idx++; }
        }
    };

    // ---- peel: barrier rounds over a shared queue while the frontier is wide (a scan opens the run and repairs an
    //      overflow), then every wave runs the CNs its own releases create from a private queue, level after level ----
    int rounds = 0, scans = 0;
    if (scal[S_NE] > 0) {                                                // (the build's barrier is behind every wave's count)
        const int kSwitch = a.kswitch;
        const int wcap = (qcap / kWaves) & ~1, half_cap = wcap / 2;
        // A scan is walked a queue-full at a time: wave v owns the groups of 64 count words v * 64 + k * BLOCK and keeps its
        // cursor kw; while a scan is pending every round tops its queue up, behind what the last round pushed, from the cursors.
        // A group that does not fit is left for the next round (what it did queue is queued again then: a CN met twice is
        // harmless, its second step finds no neighbour to claim).  So a frontier longer than a queue costs no second scan;
        // only entries DROPPED by a full queue (pushes, spills) start one, from cursor 0.
        int ncur = 0, cur = 0, rd_off = 0, kw = 0;                       // this round reads q[cur] + rd_off, pushes into q[cur ^ 1]
        bool pending = true;
        scans = 1;
        for (;;) {
            QT *qc = q[cur] + rd_off, *qn = q[cur ^ 1];
            const int cap_c = qcap - rd_off;
            if (pending) {                                               // scal[S_Q] == ncur, behind a barrier
                while (wave * 64 + kw * BLOCK < a.ncw) {
                    if (__builtin_amdgcn_readfirstlane(*(volatile int *)&scal[S_Q]) >= cap_c) break;
                    const int w = wave * 64 + kw * BLOCK + lane;
                    uint32_t z = w < a.ncw ? scan_word(w) : 0u;
                    const int mine = __popc(z);
                    const int incl = (int)wave_inclusive_scan((uint32_t)mine);
                    const int tot = __builtin_amdgcn_readlane(incl, 63);
                    if (tot) {
                        int base = 0;
                        if (lane == 0) base = atomicAdd(&scal[S_Q], tot);
                        base = __builtin_amdgcn_readfirstlane(base);
                        int idx = base + incl - mine;
                        while (z) {
                            const int k = (__ffs((int)z) - 1) >> 2;
                            z &= z - 1;
                            if (idx < cap_c) qc[idx] = (QT)(w * 8 + k);
                            idx++;
                        }
                        if (base + tot > cap_c) break;                   // this group did not fit: again next round
                    }
                    kw++;
                }
                if (lane == 0 && wave * 64 + kw * BLOCK < a.ncw) scal[S_MORE] = 1;
                __syncthreads();
                ncur = min(scal[S_Q], cap_c);
                pending = scal[S_MORE] != 0;
                __syncthreads();
            }
            if (tid == 0) { scal[S_MORE] = 0; scal[S_N0 + ((rounds + 1) & 1)] = 0; }
            int *push = &scal[S_N0 + (rounds & 1)];
            bool overflow = false;
            // entries a wave's private half-queue cannot take go to the part of qc behind the kSwitch entries the waves start from
            QT *spill = qc + kSwitch;
            const int spill_cap = cap_c - kSwitch;
            const bool shared = pending || ncur > kSwitch || half_cap < kMinHalf || spill_cap < 0;
            if (shared) {
                for (int k0 = wave * 64; k0 < ncur; k0 += BLOCK) {
                    uint32_t out[DV] = {};
                    if (k0 + lane < ncur) step((int)qc[k0 + lane], out);
                    append(out, push, qn, overflow);
                }
            } else {
                // private phase: wave w takes entries w, w + kWaves, … into its own part of qn and runs to exhaustion
                QT *mine = qn + wave * wcap;
                int cntw = (ncur - wave + kWaves - 1) / kWaves, cur = 0;
                if (cntw < 0) cntw = 0;
                if (lane < cntw) mine[lane] = qc[wave + lane * kWaves];
                while (cntw > 0) {
                    QT *src = mine + cur * half_cap, *dst = mine + (cur ^ 1) * half_cap;
                    int ncnt = 0;
                    for (int b0 = 0; b0 < cntw; b0 += 64) {
                        uint32_t out[DV] = {};
                        if (b0 + lane < cntw) step((int)src[b0 + lane], out);
                        {   // append: wave-synchronous, no atomics
                            int mine_n = 0;
#pragma unroll
                            for (int i = 0; i < DV; i++) mine_n += out[i] != 0u;
                            const int incl = (int)wave_inclusive_scan((uint32_t)mine_n);
                            int idx = ncnt + incl - mine_n;
#pragma unroll
                            for (int i = 0; i < DV; i++)
                                if (out[i]) {
                                    if (idx < half_cap) {
                                        dst[idx] = (QT)(out[i] - 1u);
                                    } else {                             // rare: the next shared round runs these
                                        const int s = atomicAdd(push, 1);
                                        if (s < spill_cap) spill[s] = (QT)(out[i] - 1u); else overflow = true;
                                    }
                                    idx++;
                                }
                            ncnt += __builtin_amdgcn_readlane(incl, 63);
                        }
                    }
                    cntw = min(ncnt, half_cap);
                    cur ^= 1;
                }
            }
            if (overflow) scal[S_OVF] = 1;
            __syncthreads();
            rounds++;
            const int pushed = *push;
            const bool dropped = scal[S_OVF] != 0;                       // a full queue dropped CNs: find them by a scan
            __syncthreads();
            if (dropped) {
                ncur = 0; kw = 0; rd_off = 0; pending = true; scans++;
            } else if (shared) {
                ncur = min(pushed, qcap); cur ^= 1; rd_off = 0;
            } else {
                ncur = min(pushed, spill_cap); rd_off += kSwitch;        // the spilled entries, where they lie in q[cur]
            }
            if (!pending && ncur == 0) break;
            // (wide: S_OVF is cleared only where it was set; then a scan is pending and the barrier below stands between this
            // store and the next round's overflow flags, whichever of the sixteen waves runs ahead)
            if (tid == 0) { if (!WIDE || dropped) scal[S_OVF] = 0; scal[S_Q] = ncur; }
            if (pending) __syncthreads();                                // the scan appends behind scal[S_Q]
        }
    }

    // ---- lost set (PD:659-666), components of more than two (PD:677-691) -- only where something is left ----------------
    {
        uint32_t any = 0;
        for (int w = tid; w < nw; w += BLOCK) any |= U[w];
        if (any) scal[S_ANY] = 1;
    }
    __syncthreads();
    if (scal[S_ANY]) {
        for (int c = tid; c < a.ncw; c += BLOCK) cnt[c] = 0;             // counts over the lost VNs only, from here on
        __syncthreads();
        int lost = 0, lost_exp = 0;
        for (int w = tid; w < nw; w += BLOCK) {
            uint32_t x = U[w], keep = 0;
            while (x) {
                const int b = __ffs((int)x) - 1;
                x &= x - 1;
                const int j = w * 32 + b;
                const Row<DV> r = vn_row(j);
                const int base = (int)__umulhi((uint32_t)j, a.magic_v) * C;
                int cc[DV];
                bool in_range = false, all_inside = true;
#pragma unroll
                for (int i = 0; i < DV; i++) {
                    cc[i] = cn_of_edge(base, i, (int)r[i]);
                    in_range |= cc[i] >= a.lost_lo && cc[i] < a.lost_hi;                // PD:661-664
                    all_inside &= cc[i] < cn_lim;                                       // PD:665
                }
                if (in_range && all_inside) {
                    keep |= 1u << b;
#pragma unroll
                    for (int i = 0; i < DV; i++) atomicAdd(&cnt[cc[i] >> 3], 1u << ((cc[i] & 7) * 4));
                }
            }
            U[w] = keep;                                                 // U := lost
            lost += __popc(keep);
        }
        __syncthreads();
        // what VN j's CNs say: -2 = some CN holds >= 3 lost VNs or two different partners show up; -1 = no partner; else the partner
        auto neighbourhood = [&](int j) {
            const Row<DV> r = vn_row(j);
            const int pos = (int)__umulhi((uint32_t)j, a.magic_v);
            int partner = -1;
#pragma unroll
            for (int i = 0; i < DV; i++) {
                int pc = pos + i;                                        // the CN position of edge i
                if constexpr (TB) { if (pc >= a.L) pc -= a.L; }
                const int c = pc * C + (int)r[i];
                const uint32_t k = count_of(c);
                if (k >= 3u) return -2;
                if (k == 2u) {
                    const Row<DC> s = cn_row(c);
                    int other = -1;
#pragma unroll
                    for (int e = 0; e < DC; e++) {
                        const uint32_t se = s[e];
                        if (se == 0xFFFFu) continue;
                        int vp = pc - (int)(se % DV);                    // c lies in CN position pc
                        if constexpr (TB) { if (vp < 0) vp += a.L; }
                        const int j2 = vp * V + (int)(se / DV);
                        if (j2 != j && u_bit(j2)) other = j2;
                    }
                    if (partner >= 0 && other != partner) return -2;
                    partner = other;
                }
            }
            return partner;
        };
        for (int w = tid; w < nw; w += BLOCK) {
            uint32_t x = U[w];
            while (x) {
                const int b = __ffs((int)x) - 1;
                x &= x - 1;
                const int j = w * 32 + b;
                int pa = neighbourhood(j);
                if (pa >= 0 && neighbourhood(pa) != j) pa = -2;          // one partner: is {a, partner} closed?
                if (pa == -2) {                                          // component of > 2 VNs
                    lost_exp++;
                    const int pos = (int)__umulhi((uint32_t)j, a.magic_v);              // cc[0] / cns_pos = int(u.birthday / cns_per_pos), PD:160,687
                    if (atomicExch(&pos_flag[pos], 1) == 0) atomicAdd(&scal[S_BLK], 1);
                }
            }
        }
        lost = wave_sum(lost);
        lost_exp = wave_sum(lost_exp);
        if (lane == 0 && lost) atomicAdd(&scal[S_LOST], lost);
        if (lane == 0 && lost_exp) atomicAdd(&scal[S_EXP], lost_exp);
        __syncthreads();
    }
    if (a.lost_out)
        for (int w = tid; w < nw; w += BLOCK) a.lost_out[(size_t)trial * nw + w] = U[w];
    if (tid == 0) {
        int32_t *o = a.out + (size_t)trial * 8;
        o[0] = scal[S_LOST]; o[1] = scal[S_EXP]; o[2] = scal[S_BLK]; o[3] = 0; o[4] = 0; o[5] = rounds; o[6] = scans > 0 ? scans - 1 : 0;
        o[7] = scal[S_NE];
    }
}

// The LDS carve for `per_cu` workgroups per CU: counts, U, the frozen bitmap (sized by fz_lim, not by nk), the position flags,
// the scalars, then two queues of what is left (narrow: at most 2048 words each, as full_bp_small.hip's, two entries per word;
// wide: per_cu = 1, one entry per word, no cap, at least kWideMinQueue entries)
int make_args(const scldpc_code_params *p, int fz_lim, int per_cu, SwArgs *a, bool wide = false)
{
    const int n = scldpc::n_of(p), nk = scldpc::nk_of(p);
    a->L = p->L; a->V = p->vns_pos; a->C = p->cns_pos; a->n = n; a->nk = nk;
    a->nw = (n + 31) / 32; a->ncw = (nk + 7) / 8;
    a->fz_lim = fz_lim;
    int off = 0;
    auto take = [&](int words) { int o = off; off += (words + 3) & ~3; return o; };
    take(a->ncw);
    a->off_U = take(a->nw);
    a->off_fz = take(((fz_lim + 7) / 8 + 3) / 4);
    a->off_pos = take(p->L);
    a->off_scal = take(S_N);
    const int budget = scldpc::kMaxLdsBytes / per_cu / 4 - 128;           // words per workgroup
    int qwords = ((budget - off) / 2) & ~3;                              // per queue
    if (qwords > 2048 && !wide) qwords = 2048;
    if (qwords < (wide ? kWideMinQueue : kMinQueueWords)) return -1;
    a->qcap = wide ? qwords : 2 * qwords;
    a->off_q0 = take(qwords);
    a->off_q1 = take(qwords);
    a->total = off;
    return 0;
}

// as many workgroups per CU as the instance aims at, fewer while the queues do not fit; the workgroups per CU, or -1
int carve(const scldpc_code_params *p, int fz_lim, int per_cu, SwArgs *a)
{
    while (per_cu > 1 && make_args(p, fz_lim, per_cu, a) != 0) per_cu--;
    return make_args(p, fz_lim, per_cu, a) == 0 ? per_cu : -1;
}

using Kernel = void (*)(const SwArgs);
// The instances with their VGPRs / SGPRs at -O3 for gfx950 (make resources), and the workgroups per CU each is
// bounded for
struct Instance { Kernel kern; int per_cu; };
Instance instance_of(int dv, int dc, bool wide = false, bool tb = false)
{
    if (tb) {
        // The ring peels at all L positions at once where the chain peels in a wave: its levels are some L / dv times as wide
        // (about 1200 CNs behind the first frontier at (4,8), L = 50, M = 1000, against the 768 entries a carve for seven
        // workgroups leaves).  So the narrow ring instances aim the carve at kRingPerCu workgroups per CU, i.e. at longer queues:
        // no scan after the first in 2048 trials of each full-size shape, and the decoder no slower than at seven, six or five
        // (profiles/sweep_ens_per_cu_ab.txt).  The register bounds stay the chain's.
        if (dv == 4 && dc == 8) return wide ? Instance{peel_sweep_small_kernel<4, 8, 0, true, true>, 1} : Instance{peel_sweep_small_kernel<4, 8, 0, false, true>, kRingPerCu};
        if (dv == 3 && dc == 6) return wide ? Instance{peel_sweep_small_kernel<3, 6, 0, true, true>, 1} : Instance{peel_sweep_small_kernel<3, 6, 0, false, true>, kRingPerCu};
        if (dv == 5 && dc == 10) return wide ? Instance{peel_sweep_small_kernel<5, 10, 0, true, true>, 1} : Instance{peel_sweep_small_kernel<5, 10, 6, false, true>, kRingPerCu};
        return {nullptr, 0};
    }
    if (wide) {
        if (dv == 4 && dc == 8) return {peel_sweep_small_kernel<4, 8, 0, true>, 1};
        if (dv == 3 && dc == 6) return {peel_sweep_small_kernel<3, 6, 0, true>, 1};
        if (dv == 5 && dc == 10) return {peel_sweep_small_kernel<5, 10, 0, true>, 1};
        return {nullptr, 0};
    }
    if (dv == 4 && dc == 8) return {peel_sweep_small_kernel<4, 8>, kPerCu};
    if (dv == 3 && dc == 6) return {peel_sweep_small_kernel<3, 6>, kPerCu};
    if (dv == 5 && dc == 10) return {peel_sweep_small_kernel<5, 10, 6>, 6};        // six waves per SIMD (12 B of scratch at seven)
    return {nullptr, 0};
}

// the shape rule of the 4-bit decoders' _deg entry points (narrow, socket table) plus this kernel's own carve
const char *shape_limit(const scldpc_code_params *p, int fz_lim)
{
    if (const char *why = scldpc::small_deg_shape_limit(p)) return why;
    SwArgs a{};
    if (carve(p, fz_lim, 1, &a) < 0) return "LDS: the CN counts, the VN bits and the bitmap of sweep_start CNs leave no room for the queues";
    return nullptr;
}

// The shape rule of the wide form (the header comment): the pair, 16-bit sockets and position-local CN ids, exact division,
// and a carve at one workgroup per CU that leaves kWideMinQueue entries per queue.  No bound on nk either way.
const char *wide_shape_limit(const scldpc_code_params *p, int fz_lim)
{
    if (scldpc::check_params(p)) return "invalid code parameters";
    if (p->dc > 15) return "dc must be at most 15 (a CN's count of erased neighbours is kept in 4 bits)";
    if (!instance_of(p->dv, p->dc, true).kern) {
        static thread_local char text[96];
        snprintf(text, sizeof text, "no instance for dv = %d, dc = %d (takes (3,6), (4,8) and (5,10))", p->dv, p->dc);
        return text;
    }
    if ((int64_t)p->vns_pos * p->dv > 65535) return "sockets: vns_pos * dv must fit 16 bits (at most 65535)";
    if (p->cns_pos > 65536) return "at most 65536 CNs per position (16-bit position-local CN ids)";
    const char *lds = "LDS: the CN counts, the VN bits and the bitmap of sweep_start CNs leave fewer than 1024 entries per queue "
                      "(160 KiB - 512 B per trial)";
    const int64_t n64 = (int64_t)p->L * p->vns_pos, nk64 = (int64_t)(p->L + p->dv - 1) * p->cns_pos;
    if (n64 / 8 + nk64 / 2 > scldpc::kMaxLdsBytes) return lds;          // (also keeps n and nk far inside 32 bits)
    uint32_t m;
    if (!scldpc::magic_of(p->vns_pos, scldpc::n_of(p) + 32, &m) || !scldpc::magic_of(p->cns_pos, scldpc::nk_of(p), &m))
        return "no exact multiply-high division for this vns_pos / cns_pos";
    SwArgs a{};
    if (make_args(p, fz_lim, 1, &a, true) != 0) return lds;
    return nullptr;
}

// what the ring asks beyond the chain's shape rules: with fewer positions than edges two edges of a VN would meet in one position
constexpr const char *kRingLimit = "tail-biting needs L >= dv";

// The one body of the four entry points (tb: the tail-biting instances).  The checks come in one fixed order: the parameters, the CN ranges, the shape (judged
// even for an empty batch), the buffers; nothing is dereferenced before all have passed.
int sweep_launch(const char *who, bool wide, bool tb, const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                 const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size, int32_t sweep_start, int32_t lost_lo,
                 int32_t lost_hi, int32_t *d_out, uint32_t *d_lost_bits, void *stream)
{
    using namespace scldpc;
    if (int rc = check_params(p)) return rc;
    const int64_t nk64 = (int64_t)(p->L + p->dv - 1) * p->cns_pos;
    if (total_size < 0 || total_size > nk64 || sweep_start < 0 || lost_lo < 0 || lost_hi > nk64)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: CN ranges outside [0,%lld]", who, (long long)nk64);
    const int fz_lim = std::min(sweep_start, total_size);
    if (const char *why = wide ? wide_shape_limit(p, fz_lim) : shape_limit(p, fz_lim))
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: %s", who, why);
    if (tb && p->L < p->dv)                                              // (part of the ring's shape rule: as the sampler's)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: %s (got L = %d, dv = %d)", who, kRingLimit, p->L, p->dv);
    if (ntrials < 0 || (ntrials > 0 && (!d_out || !d_vn_adj16 || !d_cn_sock16 || !d_chan_bits)))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer or negative ntrials", who);
    if (ntrials == 0) return SCLDPC_OK;

    SwArgs a{};
    const Instance inst = instance_of(p->dv, p->dc, wide, tb);
    int per_cu = inst.per_cu;
    // A/B only (tools/sweep_small_speedup.py): aim the carve at fewer workgroups per CU, i.e. at longer queues
    if (const char *v = getenv("SCLDPC_DEBUG_SWEEP_PER_CU")) per_cu = std::max(1, std::min(atoi(v), per_cu));
    if (!inst.kern || (wide ? make_args(p, fz_lim, 1, &a, true) : carve(p, fz_lim, per_cu, &a)) < 0)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: LDS: the CN counts and VN bits do not fit", who);
    magic_of(p->vns_pos, a.n + 32, &a.magic_v);
    magic_of(p->cns_pos, a.nk, &a.magic_c);
    a.cn_lim = total_size; a.lost_lo = lost_lo; a.lost_hi = lost_hi;
    a.vn_adj16 = d_vn_adj16; a.cn_sock16 = d_cn_sock16; a.chan = d_chan_bits; a.out = d_out; a.lost_out = d_lost_bits;
    a.kswitch = wide ? kSwitchWidthWide : kSwitchWidth;
    // tests and A/B only: a shorter queue, so that small shapes overflow and re-scan (a private half-queue below 64 entries,
    // wide: 32, keeps the waves on the shared queue).  The LDS taken stays that of the full carve.
    if (const char *v = getenv("SCLDPC_DEBUG_SWEEP_QCAP")) a.qcap = std::max(kMinDebugQcap, std::min(atoi(v), a.qcap));
    if (int rc = allow_max_lds(reinterpret_cast<const void *>(inst.kern))) return rc;
    hipLaunchKernelGGL(inst.kern, dim3(ntrials), dim3(wide ? kBlockWide : kBlock), 4u * (size_t)a.total,
                       static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

}  // namespace

// 1 when scldpc_peel_sweep_device_sock16 takes this ensemble (for sweep_start = 0; a launch judges its own sweep_start)
extern "C" int scldpc_peel_sweep_sock16_supported(const scldpc_code_params *p) { return shape_limit(p, 0) == nullptr; }

// 1 when scldpc_peel_sweep_device_sock16_wide takes this ensemble (for sweep_start = 0; a launch judges its own sweep_start)
extern "C" int scldpc_peel_sweep_wide_supported(const scldpc_code_params *p) { return wide_shape_limit(p, 0) == nullptr; }

// One trial of simulate_sc_ldpc's loop body per batch entry (PD:650-691) from the 2-byte VN -> CN table and the CN -> socket
// table: d_out and d_lost_bits as scldpc_peel_sweep_device_adj16 writes them (columns 0, 1, 2, 7 and the bitmap bit for bit;
// column 5 counts this kernel's barrier rounds, column 6 its scans after the first).  The checks come in one fixed order:
// the parameters, the CN ranges, the shape (judged even for an empty batch), the buffers.
extern "C" int scldpc_peel_sweep_device_sock16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                               const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size,
                                               int32_t sweep_start, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                               uint32_t *d_lost_bits, void *stream)
{
    return sweep_launch("scldpc_peel_sweep_device_sock16", false, false, p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, total_size,
                        sweep_start, lost_lo, lost_hi, d_out, d_lost_bits, stream);
}

// The same from the wide form: 32-bit queue entries, one 1024-thread workgroup per CU, any number of CNs per trial whose 4-bit
// state leaves 1024 entries per queue in one CU's LDS (wide_shape_limit).  Same outputs, same order of the checks.
extern "C" int scldpc_peel_sweep_device_sock16_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                    const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size,
                                                    int32_t sweep_start, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                                    uint32_t *d_lost_bits, void *stream)
{
    return sweep_launch("scldpc_peel_sweep_device_sock16_wide", true, false, p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, total_size,
                        sweep_start, lost_lo, lost_hi, d_out, d_lost_bits, stream);
}

// 1 when scldpc_peel_sweep_device_sock16_tb / _tb_wide takes this ensemble as a ring (for sweep_start = 0): the chain's rule and L >= dv
extern "C" int scldpc_peel_sweep_tb_supported(const scldpc_code_params *p) { return shape_limit(p, 0) == nullptr && p->L >= p->dv; }
extern "C" int scldpc_peel_sweep_tb_wide_supported(const scldpc_code_params *p) { return wide_shape_limit(p, 0) == nullptr && p->L >= p->dv; }

// scldpc_peel_sweep_device_sock16 on the tables of a tail-biting code (scldpc_sample_philox_ensemble_device_adj16_sock): the TB
// instances.  Columns 0, 1, 2, 7 of d_out and d_lost_bits equal scldpc_peel_sweep_device on the int32 rows of the same code.
extern "C" int scldpc_peel_sweep_device_sock16_tb(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                  const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size,
                                                  int32_t sweep_start, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                                  uint32_t *d_lost_bits, void *stream)
{
    return sweep_launch("scldpc_peel_sweep_device_sock16_tb", false, true, p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, total_size,
                        sweep_start, lost_lo, lost_hi, d_out, d_lost_bits, stream);
}

// The same from the wide form
extern "C" int scldpc_peel_sweep_device_sock16_tb_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                       const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t total_size,
                                                       int32_t sweep_start, int32_t lost_lo, int32_t lost_hi, int32_t *d_out,
                                                       uint32_t *d_lost_bits, void *stream)
{
    return sweep_launch("scldpc_peel_sweep_device_sock16_tb_wide", true, true, p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, total_size,
                        sweep_start, lost_lo, lost_hi, d_out, d_lost_bits, stream);
}
