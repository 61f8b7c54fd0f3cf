// The fixpoint of unlimited flooding BP (decodeBP, BPF:900-1140) with 4 bits of LDS per check node — gfx950.
//
// full_bp.hip keeps [count | fold of the erased neighbours' ids] per CN (16 bits) so that a CN with one erased neighbour
// names it without a lookup; the 52 KiB of CN words then limit a CU to two trials in flight, and the decoder is bound by
// the latency of its ~230 dependent levels.  Here a CN keeps ONLY the count (a nibble): when it drops to
// one, its dc neighbours are read from the CN -> VN table the second-generation sampler emits (sampler_v2.hip) and the
// one neighbour whose bit in the erased-VN bitmap U is still set is the one to resolve.  A trial needs 13 + 6 KiB of
// state + queues = 23 KiB, a 256-thread workgroup decodes it, and seven trials share a CU: 3.5 times the trials in
// flight for one more dependent gather per level (measured A/B of workgroup sizes 64 … 512, five to eight trials per
// CU and the switch-over width: DESIGN.md §5).
//
// Safe without a barrier per level because every release claims its VN in U (atomic test-and-clear) BEFORE it decrements
// the VN's CNs: whoever sees a CN's count reach one (its decrement returned two, or a scan read one) sees at most one
// neighbour with its U bit still set — the unclaimed one — and if that neighbour is being released elsewhere at that
// moment the bit is already clear and the entry is dropped (that release will take the count to zero).
//
// LEVEL = true is the same machine walked one flooding iteration per barrier round (scldpc_full_bp_device_cn16): a round
// releases exactly the CNs whose count was one when it began, so round t is the reference's iteration t (SURVEY.md §7.4 A;
// full_bp.hip does the same on 16-bit CN words with two trials per CU) — iteration count, the cap MaxNumIt (BPF:1065), the
// stop tests (BPF:1044-1045) and deg_1_iter's invariant (BPF:1035-1039) included.  Rounds whose frontier does not fit the
// queue (the first one or two) take it from a snapshot bitmap, one queue-full at a time; that bitmap costs a seventh trial
// per CU (six fit).
//
// WIDE is the LEVEL machine (with or without the trajectory rows) for trials of more than 65536 CNs — bp_traj's shipped N = 5000,
// L = 50 has 132 500: queue entries are 32-bit CN ids, one 1024-thread workgroup takes a CU and all of its 160 KiB, and the CN ->
// socket table comes from scldpc_cn_sockets_device where the second-generation sampler stops (8192 sockets per position).
// Socket table only; CAPS has a wide form (the checkpoints sit inside the LEVEL loop), the fixpoint form (its private-queue carve
// assumes four waves) and PERSIST have none.
//
// Outputs: the counters of scldpc_full_bp_fixpoint_device (everything decodeBP reports except the iteration count), or
// with LEVEL all of scldpc_full_bp_device's counters.
// The size-2 stopping-set expurgation only looks at what the reference reports: the FIRST position with a positive
// expurgated count (is_first_printed, BPF:1074, 1126-1132), so only that position's erased VNs are examined.
#include "common.h"
#include "kernel_util.h"
#include "table_rows.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

using namespace scldpc_dev;

enum { SC_NE = 0, SC_REM, SC_N0, SC_N1, SC_OVF, SC_Q, SC_N = 8 };
// LEVEL: per-iteration counters rotated three ways, so that one barrier per iteration is enough (as in full_bp.hip)
enum { LV_VALID = 2, LV_EXTRA0 = 3, LV_PUSH = 6, LV_DROP = 9, LV_REM = 12, LV_OVF = 15, LV_N = 18 };

struct SmArgs {
    int L, V, C, n, nk, cn_lim, nw, ncw;            // ncw = words of 8 count nibbles
    uint32_t magic_v, magic_c;
    int ntrials;                                    // workgroup b decodes trials b, b + gridDim.x, …
    int kswitch;                                    // frontier width below which the waves go private
    int max_it;                                     // LEVEL: MaxNumIt, <= 0 = unlimited
    int rows_cap;                                   // TRAJ: rows kept per trial
    int32_t *rows;                                  // TRAJ: [T][rows_cap][3] = deg_1_iter, recovered, first erased position
    int off_U, off_q0, off_q1, off_pos, off_scal, off_fb, total, qcap;      // LDS offsets in 32-bit words; qcap in entries (u16; WIDE: u32)
    const uint16_t *vn_adj16;                       // [T][n][dv]  CN index local to its position
    const uint16_t *cn_adj16;                       // [T][nk][dc] VNs of every CN (0xFFFF: none); SOCK: their sockets dv*t + i instead
    const uint32_t *chan;
    int32_t *counters;
    uint32_t *erased_out;
    int ncaps;                                      // CAPS: caps[0] < caps[1] < … (>= 1); counters [ncaps][ntrials][8]
    int caps[SCLDPC_MAX_CAPS];
};

// Row<D>, VnUnit / CnUnit and load_row — a table row in registers, loaded no wider than its alignment allows: table_rows.h

// Seven 4-wave workgroups per CU are 7 waves per SIMD: at most 96 SGPRs and 72 VGPRs per wave (MI355X_MICROARCH.md).
// SOCK: the CN -> VN table holds sockets (s = dv*t + i = edge i of VN t of position CNpos - i: scldpc_sample_philox_device_sock16's
// table, any chain length) instead of global VN ids (which need n < 65535).
// TRAJ (with LEVEL): the trajectory rows of the BPT build — per iteration deg_1_iter, the VNs recovered and the position of
// the first erased VN (BPT:988, 1037-1038, 1051), incl. iteration 0's count of degree-1 CNs whose only VN is known (BPF:973).
// CAPS (with LEVEL): several MaxNumIt at once.  On the BEC the flooding iterations do not depend on the cap, which only ends
// the loop (BPF:1065): where a single-cap decode tests it, the decoder takes a checkpoint instead — the counters that decode
// would report, written to that cap's block of counters [ncaps][ntrials][8] — and goes on to the next cap.  Caps the decode
// does not reach (a stop test or a broken invariant ended it first) get its final state.
// WIDE (LEVEL, LEVEL + TRAJ or LEVEL + CAPS with SOCK, nothing else): queue entries are 32-bit CN ids and ONE 1024-thread workgroup owns
// the CU and all of its LDS (four waves per SIMD, at most 128 VGPRs) — trials of more than 65536 CNs, e.g. bp_traj's default
// N = 5000, L = 50 (nk = 132 500).  There is no wide fixpoint form (the private-queue carve below assumes four waves) and no wide
// PERSIST.  A checkpoint of the wide CAPS form is the narrow one's: residual() strides by BLOCK and never touches the queues.
// DV, DC: the degree pair, fixed at compile time (the rows of both tables are unrolled).  A VN row is DV uint16 and only 2-byte
// aligned unless DV = 4 (one 8-byte load); a CN row is DC uint16, DC even, so 4-byte aligned (DC = 8: one 16-byte load).  Pairs
// other than (4,8) have the socket-table forms without PERSIST only (kernel_of).
// OCC: waves per SIMD the registers are bounded for where an instance cannot hold its form's (0: the form's).
template <int BLOCK, bool LEVEL, bool PERSIST, bool SOCK, bool TRAJ = false, bool CAPS = false, bool WIDE = false, int DV = 4, int DC = 8,
          int OCC = 0>
__global__ __launch_bounds__(BLOCK, OCC ? OCC : WIDE ? 4 : PERSIST ? 8 : 7) __attribute__((amdgpu_num_sgpr(96))) void full_bp_small_kernel(const SmArgs a)
{
    static_assert(!WIDE || (BLOCK == 1024 && LEVEL && SOCK && !PERSIST), "the wide form: LEVEL [+ TRAJ | CAPS], socket table");
    static_assert(!(TRAJ && CAPS), "the checkpoints have no rows form");
    static_assert((DV == 4 && DC == 8) || (SOCK && !PERSIST), "other degree pairs: the socket table, no PERSIST");
    static_assert(DC <= 15 && DC % 2 == 0 && DV < DC, "a CN's count of erased neighbours is a nibble; CN rows are read as 32-bit words");
    using QT = std::conditional_t<WIDE, uint32_t, uint16_t>;             // a queue entry: a CN id
    constexpr int kWaves = BLOCK / 64;
    extern __shared__ uint32_t lds[];
    uint32_t *cnt = lds;                                                 // nk nibbles
    uint32_t *U = lds + a.off_U;
    QT *q[2] = {reinterpret_cast<QT *>(lds + a.off_q0), reinterpret_cast<QT *>(lds + a.off_q1)};
    int *pos_cnt = reinterpret_cast<int *>(lds + a.off_pos);
    int *pos_ss = pos_cnt + a.L;
    int *scal = reinterpret_cast<int *>(lds + a.off_scal);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto decode_trial = [&](const int trial) {
    STAMP_DECL
    const int n = a.n, nk = a.nk, cn_lim = a.cn_lim, nw = a.nw, V = a.V, C = a.C, L = a.L, qcap = a.qcap;
    const auto *vrow = reinterpret_cast<const typename VnUnit<DV>::type *>(a.vn_adj16) + (size_t)trial * n * VnUnit<DV>::per_row;
    const auto *crow = reinterpret_cast<const typename CnUnit<DC>::type *>(a.cn_adj16) + (size_t)trial * nk * CnUnit<DC>::per_row;
    auto vn_row = [&](int j) { if constexpr (DV == 4) return load_row(vrow, j); else return load_row<DV>(vrow, j); };
    auto cn_row = [&](int c) { if constexpr (DC == 8) return load_row(crow, c); else return load_row<DC>(crow, c); };
    const uint32_t *ch = a.chan + (size_t)trial * nw;

    // ---- channel bits, clear the counts -------------------------------------------------------------------------
    for (int c = tid; c < a.ncw; c += BLOCK) cnt[c] = 0;
    int ne_local = 0;
    for (int w = tid; w < nw; w += BLOCK) {
        const uint32_t x = chan_tail(ch[w], w, nw, n);
        U[w] = x;
        ne_local += __popc(x);
    }
    if (tid < LV_N) scal[tid] = 0;
    for (int i = tid; i < 2 * L; i += BLOCK) pos_cnt[i] = 0;
    __syncthreads();
    ne_local = wave_sum(ne_local);
    if (lane == 0 && ne_local) atomicAdd(&scal[SC_NE], ne_local);

    // ---- build: every erased VN counts itself into its DV CNs; rows are loaded unconditionally (coalesced loads) -------
    constexpr int NB = 8;                                                // rows in flight per thread
    for (int j0 = tid; j0 < n; j0 += NB * BLOCK) {
        Row<DV> r[NB];
        bool er[NB];
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int j = j0 + u * BLOCK;
            er[u] = false;
            if (j < n) { r[u] = vn_row(j); er[u] = (U[j >> 5] >> (j & 31)) & 1u; }
        }
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int j = j0 + u * BLOCK;
            if (er[u]) {
                const int base = (int)__umulhi((uint32_t)j, a.magic_v) * C;
                int cc[DV];
#pragma unroll
                for (int i = 0; i < DV; i++) cc[i] = base + i * C + (int)r[u][i];
#pragma unroll
                for (int i = 0; i < DV; i++) atomicAdd(&cnt[cc[i] >> 3], 1u << ((cc[i] & 7) * 4));
            }
        }
    }
    __syncthreads();
    STAMP(0);                                                            // channel + build
    const int nch = scal[SC_NE];

    // ---- one release step: CN c is believed to have exactly one erased neighbour -----------------------------------
    // out[i] = 1 + the CN on edge i of the released VN if this release left it with one erased neighbour, else 0
    int removed = 0, drops = 0;                                          // drops (LEVEL): counts taken from one to zero
    auto step = [&](int c, uint32_t (&out)[DV]) {
#pragma unroll
        for (int i = 0; i < DV; i++) out[i] = 0;
        const Row<DC> s = cn_row(c);
        uint32_t jk[DC];
        bool none[DC];
#pragma unroll
        for (int k = 0; k < DC; k++) { jk[k] = s[k]; none[k] = jk[k] == 0xFFFFu; }
        if constexpr (SOCK) {                                            // socket s = DV * t + i -> global VN index
            const int vbase = (int)__umulhi((uint32_t)c, a.magic_c) * V;                   // CN position * V
#pragma unroll
            for (int k = 0; k < DC; k++) jk[k] = (uint32_t)(vbase - (int)(jk[k] % DV) * V) + (jk[k] / DV);
        }
        uint32_t wd[DC];
#pragma unroll
        for (int k = 0; k < DC; k++) wd[k] = U[none[k] ? 0u : jk[k] >> 5];              // no VN: any word, masked below
        int j = -1;
#pragma unroll
        for (int k = 0; k < DC; k++)
            if (!none[k] && ((wd[k] >> (jk[k] & 31u)) & 1u)) j = (int)jk[k];
        if (j < 0) return;                                               // its last neighbour is being released elsewhere
        const Row<DV> r = vn_row(j);                      // issued before the claim: overlaps its round trip
        const uint32_t bit = 1u << (j & 31);
        if (!(atomicAnd(&U[j >> 5], ~bit) & bit)) return;
        removed++;
        const int base = (int)__umulhi((uint32_t)j, a.magic_v) * C;
        int cc[DV];
#pragma unroll
        for (int i = 0; i < DV; i++) cc[i] = base + i * C + (int)r[i];
        uint32_t o[DV];
#pragma unroll
        for (int i = 0; i < DV; i++) o[i] = atomicSub(&cnt[cc[i] >> 3], 1u << ((cc[i] & 7) * 4));
#pragma unroll
        for (int i = 0; i < DV; i++) {
            const uint32_t old = (o[i] >> ((cc[i] & 7) * 4)) & 15u;
            if (old == 2u && cc[i] < cn_lim) out[i] = (uint32_t)cc[i] + 1u;
            if constexpr (LEVEL) drops += (old == 1u && cc[i] < cn_lim);
        }
    };
    // the CNs of a count word whose count is one, as a mask of the nibbles' top bits, CNs >= cn_lim dropped
    auto ones_of = [&](int w) {
        const uint32_t y = cnt[w] ^ 0x11111111u;                         // nibble == 1  <=>  zero nibble of y
        uint32_t z = ~(((y & 0x77777777u) + 0x77777777u) | y) & 0x88888888u;
        if (w * 8 + 8 > cn_lim) {                                        // the word that holds cn_lim
            const int keep = cn_lim - w * 8;
            z = keep <= 0 ? 0u : (z & ((1u << (4 * keep)) - 1u));
        }
        return z;
    };
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

    int rounds = 0, ne = 0, status = 0, be = 0, ee = 0, bee = 0;
    // ---- what decodeBP reports after its loop (BPF:1067-1138), from U and the counts as they stand: be, ee, bee --------
    // erased VNs per position into pos_cnt (zero on entry), the blocks in error, the size-2 stopping sets of the first
    // failing position.  It reads pos_cnt up to its end: a caller that clears it again puts a barrier in between.
    auto residual = [&]() {
    if (ne > 0) {
        // ---- erased VNs per position (word w of U may straddle two positions) ----------------------------------------
        for (int w = tid; w < nw; w += BLOCK) {
            uint32_t x = U[w];
            int p0 = (int)__umulhi((uint32_t)(w * 32), a.magic_v);
            int room = (p0 + 1) * V - w * 32;                            // bits of this word left in position p0
            while (x) {
                const uint32_t lo = room >= 32 ? x : (x & ((1u << room) - 1u));
                if (lo) atomicAdd(&pos_cnt[p0], __popc(lo));
                x = room >= 32 ? 0u : (x >> room);
                p0++;
                room = V;
            }
        }
        __syncthreads();
        // ---- size-2 stopping sets (BPF:1067-1133) of the first failing position(s) only ----------------------------
        int q0 = 0;
        for (;;) {
            while (q0 < L && pos_cnt[q0] == 0) q0++;
            if (q0 >= L) break;
            for (int t = tid; t < V; t += BLOCK) {
                const int j = q0 * V + t;
                if (!((U[j >> 5] >> (j & 31)) & 1u)) continue;
                const Row<DV> r = vn_row(j);
                const int base = q0 * C;
                int cc[DV];
#pragma unroll
                for (int i = 0; i < DV; i++) cc[i] = base + i * C + (int)r[i];
                bool pair = true;                                        // all DV CNs of the VN have two erased neighbours …
#pragma unroll
                for (int i = 0; i < DV; i++) pair = pair && ((cnt[cc[i] >> 3] >> ((cc[i] & 7) * 4)) & 15u) == 2u;
                if (!pair) continue;
                int partner = -1;                                        // … and the other one is the same VN for all of them
                for (int i = 0; i < DV && pair; i++) {                   // the other erased neighbour of each CN
                    const Row<DC> s = cn_row(cc[i]);
                    int other = -1;
                    for (int k = 0; k < DC; k++) {
                        const uint32_t jk = s[k];
                        if (jk == 0xFFFFu) continue;
                        // (cc[i] lies in CN position q0 + i)
                        const int j2 = SOCK ? (q0 + i - (int)(jk % DV)) * V + (int)(jk / DV) : (int)jk;
                        if (j2 != j && ((U[j2 >> 5] >> (j2 & 31)) & 1u)) other = j2;
                    }
                    if (other < 0 || (i > 0 && other != partner)) pair = false;
                    partner = other;
                }
                if (pair && (int)__umulhi((uint32_t)partner, a.magic_v) == q0) atomicAdd(&pos_ss[q0], 1);
            }
            __syncthreads();
            const int e = pos_cnt[q0] - pos_ss[q0];
            if (e > 0) { ee = e; bee = 1; break; }                       // only the FIRST such position (BPF:1126-1132)
            q0++;
        }
        for (int pos = 0; pos < L; pos++) be += pos_cnt[pos] > 0;
    }
    };
    auto put = [&](int32_t *o, int ne, int be, int ee, int bee, int rounds, int status) {
        o[SCLDPC_C_NUM_ERASURES] = ne;
        o[SCLDPC_C_NUM_BLOCKS_ERR] = be;
        o[SCLDPC_C_NUM_ERASURES_EXP] = ee;
        o[SCLDPC_C_NUM_BLOCKS_ERR_EXP] = bee;
        o[SCLDPC_C_NUM_ERASURES_P1] = 0;
        o[SCLDPC_C_ITERATIONS] = rounds;                                 // LEVEL: flooding iterations; else barrier rounds
        o[SCLDPC_C_STATUS] = status;
        o[SCLDPC_C_CHANNEL_ERASURES] = nch;
    };
    auto cap_counters = [&](int k) { return a.counters + ((size_t)k * a.ntrials + trial) * SCLDPC_NCOUNTERS; };

    int ci = 0;                                                          // CAPS: the next cap to reach
    if constexpr (LEVEL) {
        // ---- one flooding iteration per barrier round (decodeBP's do-while, BPF:927-1065) ------------------------------
        uint8_t *fb = reinterpret_cast<uint8_t *>(lds + a.off_fb);       // snapshot of a scan round: one byte per count word
        int prec = n, iter = 0, ncur = 0, nfront = 0, first_word = 0;
        if constexpr (TRAJ) {
            // degree-1 CNs whose single VN is known count into iteration 0's deg_1_iter (BPF:969-978).  Only the first and the
            // last dv-1 CN positions of the chain hold CNs of degree below dc: their rows say how many neighbours they have.
            int extra = 0;
            const int head = (DV - 1) * C, tail0 = L * C;
            for (int i = tid; i < 2 * head; i += BLOCK) {
                const int c = i < head ? i : tail0 + (i - head);
                if (c >= cn_lim || c >= nk) continue;
                const Row<DC> s = cn_row(c);
                int deg = 0;
#pragma unroll
                for (int k = 0; k < DC; k++) deg += s[k] != 0xFFFFu;
                extra += deg == 1 && ((cnt[c >> 3] >> ((c & 7) * 4)) & 15u) == 0u;
            }
            extra = wave_sum(extra);
            if (lane == 0 && extra) atomicAdd(&scal[LV_EXTRA0], extra);
        }
        bool scan = true;                                                // iteration 0 has no queue yet
        ne = nch;
        for (;;) {
            const int g = iter % 3, gn = (iter + 1) % 3;
            QT *qc = q[iter & 1], *qn = q[(iter + 1) & 1];
            if (tid == 0) { scal[LV_PUSH + gn] = 0; scal[LV_DROP + gn] = 0; scal[LV_REM + gn] = 0; scal[LV_OVF + gn] = 0; }
            int *push = &scal[LV_PUSH + g];                              // counts every 2 -> 1, queued or not
            bool overflow = false;
            removed = 0; drops = 0;
            auto run_queue = [&](int nq) {
                for (int k0 = wave * 64; k0 < nq; k0 += BLOCK) {
                    uint32_t out[DV] = {};
                    if (k0 + lane < nq) step((int)qc[k0 + lane], out);
                    append(out, push, qn, overflow);
                }
            };
            if (scan) {
                // snapshot {c < cn_lim : count == 1} BEFORE any release of this round (releases must not promote CNs into it),
                // then one queue-full of it at a time
                int valid = 0;
                for (int w = tid; w < a.ncw; w += BLOCK) {
                    uint32_t y = ones_of(w) >> 3;                        // bit 4k: CN 8w+k
                    y = (y | (y >> 3)) & 0x03030303u;
                    y = (y | (y >> 6)) & 0x000F000Fu;
                    y = (y | (y >> 12)) & 0xFFu;                         // bit k: CN 8w+k
                    fb[w] = (uint8_t)y;
                    valid += __popc(y);
                }
                if (iter == 0) {
                    valid = wave_sum(valid);
                    if (lane == 0 && valid) atomicAdd(&scal[LV_VALID], valid);
                }
                if (tid == 0) scal[SC_Q] = 0;
                __syncthreads();
                if (iter == 0) nfront = scal[LV_VALID];
                for (;;) {
                    for (int w0 = wave * 64; w0 < a.ncw; w0 += BLOCK) {  // thread t owns bytes t, t + BLOCK, …
                        const int w = w0 + lane;
                        uint32_t y = w < a.ncw ? (uint32_t)fb[w] : 0u;
                        const int mine = __popc(y);
                        const int incl = (int)wave_inclusive_scan((uint32_t)mine);
                        const int tot = __builtin_amdgcn_readlane(incl, 63);
                        if (tot == 0) continue;
                        int base = 0;
                        if (lane == 0) base = atomicAdd(&scal[SC_Q], tot);
                        int idx = __builtin_amdgcn_readfirstlane(base) + incl - mine;
                        uint32_t left = 0;
                        while (y) {
                            const int k = __ffs((int)y) - 1;
                            y &= y - 1;
                            if (idx < qcap) qc[idx] = (QT)(w * 8 + k); else left |= 1u << k;
                            idx++;
                        }
                        if (mine) fb[w] = (uint8_t)left;
                    }
                    __syncthreads();
                    const int found = scal[SC_Q];
                    __syncthreads();
                    if (tid == 0) scal[SC_Q] = 0;
                    run_queue(min(found, qcap));
                    if (found <= qcap) break;
                    __syncthreads();                                     // this queue-full is done before qc is refilled
                }
            } else {
                run_queue(ncur);
            }
            STAMP(4);                                                    // (LEVEL) this wave's releases of the iteration
            {   // one reduction for both counts: a CN is queued once in its life and an iteration's entries are dealt to the four
                // waves, so a wave releases at most nk / 4 + 64 <= 16 448 VNs per iteration (15 bits) and zeroes at most four
                // times as many CNs (17 bits).
                // WIDE: 16 waves, and a scan round runs several queue-fulls.  A queue-full of m entries gives a wave at most
                // m / 16 + 64 of them; an iteration's queue-fulls hold each CN at most once (sum of m <= nk) and all but the
                // last are full (at most nk / qcap + 1 of them), so a wave releases at most nk / 16 + 64 (nk / qcap + 1) VNs
                // per iteration.  wide_shape() refuses shapes where that exceeds 32 767 (with qcap >= 1024 and the LDS's
                // nk < 190 000 it is below 23 900), and four times as many zeroed CNs still fit the upper 17 bits.
                // Other DV: a release decrements DV counts, so drops <= DV * removed.  With r = nk / waves + 64 (nk / qcap + 1)
                // bounding a wave's releases per iteration (the narrow form's scan rounds run several queue-fulls as well),
                // the _deg forms are refused unless r <= 32 767 and DV * r < 2^17 (shape_limit).  Where the queues have
                // their full length the narrow r is at most 16 384 + 64 * 17 = 17 472, DV * r <= 87 360 for DV = 5; a
                // carve squeezed to its shortest queue (256 entries) on 65 536 CNs would reach r = 32 832 and is refused.
                const uint32_t both = (uint32_t)wave_sum((int)((uint32_t)removed | ((uint32_t)drops << 15)));
                removed = (int)(both & 0x7FFFu); drops = (int)(both >> 15);
            }
            if (lane == 0) {
                if (removed) atomicAdd(&scal[LV_REM + g], removed);
                if (drops) atomicAdd(&scal[LV_DROP + g], drops);
            }
            if (overflow) scal[LV_OVF + g] = 1;
            STAMP(5);                                                    // reductions
            __syncthreads();                                             // end of flooding iteration `iter`
            STAMP(6);                                                    // waiting for the other waves
            // ---- bookkeeping, identical in every thread (full_bp.hip)
            const int deg1 = nfront + ((TRAJ && iter == 0) ? scal[LV_EXTRA0] : 0);      // deg_1_iter, BPF:969-978
            ne -= scal[LV_REM + g];
            const int recovered = prec - ne;
            if constexpr (TRAJ) {
                if (wave == 0 && a.rows && rounds < a.rows_cap) {
                    // first erased VN (BPT:1037-1038): U only loses bits, so resume from the last hit
                    int fw = first_word, first = n;
                    while (fw < nw) {
                        const uint32_t w = (fw + lane < nw) ? U[fw + lane] : 0u;
                        const unsigned long long m = __ballot(w != 0u);
                        if (m) {
                            const int l0 = __ffsll((long long)m) - 1;
                            const uint32_t w0 = (uint32_t)__shfl((int)w, l0, 64);
                            fw += l0;
                            first = fw * 32 + (__ffs((int)w0) - 1);
                            break;
                        }
                        fw += 64;
                    }
                    first_word = fw;
                    if (lane == 0) {
                        int32_t *r = a.rows + ((size_t)trial * a.rows_cap + rounds) * 3;
                        r[0] = deg1; r[1] = recovered; r[2] = (int)__umulhi((uint32_t)first, a.magic_v);
                    }
                }
                __syncthreads();                                         // wave 0 read U above: the next round's releases stay behind it
            }
            rounds++;
            if (deg1 < recovered && iter > 0) { status = -1; break; }    // BPF:1035-1039
            if (ne == 0 || ne == prec) break;                            // BPF:1044-1045
            prec = ne;
            // next frontier: queued 2 -> 1 CNs minus those that went on to 0 within this round
            nfront = scal[LV_PUSH + g] - (scal[LV_DROP + g] - nfront);
            scan = scal[LV_OVF + g] != 0;
            ncur = scan ? 0 : scal[LV_PUSH + g];
            iter++;
            if (!CAPS && a.max_it > 0 && iter >= a.max_it) break;        // BPF:1065
            if constexpr (CAPS) {
                if (iter >= a.caps[ci]) {                                // checkpoint: a decode with MaxNumIt = caps[ci] ends here
                    be = ee = bee = 0;
                    residual();
                    if (tid == 0) put(cap_counters(ci), ne, be, ee, bee, rounds, 0);
                    __syncthreads();                                     // U, the counts and pos_cnt read: releases may go on
                    for (int i = tid; i < 2 * L; i += BLOCK) pos_cnt[i] = 0;     // (the next checkpoint is behind a barrier)
                    if (++ci == a.ncaps) break;
                }
            }
            STAMP(7);                                                    // bookkeeping
        }
        __syncthreads();
        STAMP(1);
    } else {
        // ---- peel: barrier rounds over a shared queue while the frontier is wide (a scan opens the run and repairs an
        //      overflow), then every wave runs the CNs its own releases create from a private queue, level after level ----
        const int kSwitch = a.kswitch;
        const int wcap = (qcap / kWaves) & ~1, half_cap = wcap / 2;
        int ncur = 0;
        bool scan = true;
        for (;;) {
            QT *qc = q[rounds & 1], *qn = q[(rounds + 1) & 1];
            if (scan) {
                // every CN < cn_lim whose count is one right now, compacted into qc
                for (int w0 = wave * 64; w0 < a.ncw; w0 += BLOCK) {
                    const int w = w0 + lane;
                    uint32_t z = w < a.ncw ? ones_of(w) : 0u;
                    const int mine = __popc(z);
                    const int incl = (int)wave_inclusive_scan((uint32_t)mine);
                    const int tot = __builtin_amdgcn_readlane(incl, 63);
                    if (tot == 0) continue;
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&scal[SC_Q], tot);
                    base = __builtin_amdgcn_readfirstlane(base);
                    int idx = base + incl - mine;
                    while (z) {
                        const int k = (__ffs((int)z) - 1) >> 2;
                        z &= z - 1;
                        if (idx < qcap) qc[idx] = (QT)(w * 8 + k);
                        idx++;
                    }
                }
                __syncthreads();
                ncur = scal[SC_Q];
                if (ncur > qcap) { ncur = qcap; if (tid == 0) scal[SC_OVF] = 1; }      // the rest: next scan
                __syncthreads();
            }
            if (tid == 0) { scal[SC_Q] = 0; scal[SC_N0 + ((rounds + 1) & 1)] = 0; }
            int *push = &scal[SC_N0 + (rounds & 1)];
            bool overflow = false;
            if (ncur > kSwitch || half_cap < 64) {
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
                                if (out[i]) { if (idx < half_cap) dst[idx] = (QT)(out[i] - 1u); else overflow = true; idx++; }
                            ncnt += __builtin_amdgcn_readlane(incl, 63);
                        }
                    }
                    cntw = min(ncnt, half_cap);
                    cur ^= 1;
                }
            }
            if (overflow) scal[SC_OVF] = 1;
            __syncthreads();
            rounds++;
            const int pushed = *push;
            scan = scal[SC_OVF] != 0;            // a full queue dropped CNs: find them by a scan
            __syncthreads();
            if (tid == 0) scal[SC_OVF] = 0;
            ncur = scan ? 0 : min(pushed, qcap);
            if (!scan && ncur == 0) break;
        }
        STAMP(1);                                                            // peeling
        removed = wave_sum(removed);
        if (lane == 0 && removed) atomicAdd(&scal[SC_REM], removed);
        __syncthreads();
        ne = nch - scal[SC_REM];
    }

    if (!CAPS || ci < a.ncaps) {
        be = ee = bee = 0;
        residual();
    }
    STAMP(2);                                                            // per-position counts + expurgation
    STAMP_FLUSH();
    if (a.erased_out)
        for (int w = tid; w < nw; w += BLOCK) a.erased_out[(size_t)trial * nw + w] = U[w];
    if (tid == 0) {
        if constexpr (CAPS) {
            for (int k = ci; k < a.ncaps; k++) put(cap_counters(k), ne, be, ee, bee, rounds, status);    // not reached
        } else {
            put(a.counters + (size_t)trial * SCLDPC_NCOUNTERS, ne, be, ee, bee, rounds, status);
        }
    }
    };
    // PERSIST: workgroup b decodes trials b, b + gridDim.x, …; otherwise exactly one
    if constexpr (PERSIST) {
        for (int trial = blockIdx.x; trial < a.ntrials; trial += gridDim.x) {
            decode_trial(trial);
            __syncthreads();                                             // LDS is re-used by the workgroup's next trial
        }
    } else {
        decode_trial((int)blockIdx.x);
    }
}

// The one LDS carve.  wide: 32-bit queue entries (one per word), and no 2048-word cap on a queue: that cap was tuned for seven
// workgroups per CU, the wide form's one workgroup takes what the state leaves
int make_args(const scldpc_code_params *p, int32_t is_term, SmArgs *a, int per_cu, bool level = false, bool wide = false)
{
    const int n = scldpc::n_of(p), nk = scldpc::nk_of(p);
    a->L = p->L; a->V = p->vns_pos; a->C = p->cns_pos; a->n = n; a->nk = nk;
    a->cn_lim = is_term ? nk : p->L * p->cns_pos;                        // BPT:944-948
    a->nw = (n + 31) / 32; a->ncw = (nk + 7) / 8;
    int off = 0;
    auto take = [&](int words) { int o = off; off += (words + 3) & ~3; return o; };
    take(a->ncw);
    a->off_U = take(a->nw);
    a->off_pos = take(2 * p->L);
    a->off_scal = take(LV_N);
    a->off_fb = level ? take((a->ncw + 3) / 4) : 0;                      // snapshot bytes of the scan rounds
    const int budget = scldpc::kMaxLdsBytes / per_cu / 4 - 128;           // words per workgroup
    int qwords = ((budget - off) / 2) & ~3;                              // per queue; two uint16 entries per word
    if (qwords > 2048 && !wide) qwords = 2048;
    if (qwords < 128) return -1;
    a->qcap = wide ? qwords : 2 * qwords;
    a->off_q0 = take(qwords);
    a->off_q1 = take(qwords);
    a->total = off;
    return 0;
}

constexpr int kBlockSmall = 256;        // threads per trial
constexpr int kPerCu = 7;               // workgroups per CU the LDS carve aims at (SGPRs <= 96, VGPRs <= 72)
constexpr int kSwitchWidth = 128;       // frontier entries below which the waves go private
constexpr int kBlockWide = 1024;        // the wide form: one workgroup per CU, four waves per SIMD
constexpr int kWideMinQueue = 1024;     // entries per queue below which the wide form is not worth selecting
// floor of SCLDPC_DEBUG_DECODER_QCAP: every queue store is guarded by idx < qcap and a scan round takes min(found, qcap)
// entries, so a queue of one entry stays in bounds and still makes progress
constexpr int kMinDebugQcap = 1;
static_assert(kSwitchWidth <= 64 * (kBlockSmall / 64), "a wave takes at most one frontier entry per lane into its private queue");

// The degree pairs with instances (kernel_of): their index, or -1
constexpr int pair_of(int dv, int dc) { return dv == 4 && dc == 8 ? 0 : dv == 3 && dc == 6 ? 1 : dv == 5 && dc == 10 ? 2 : -1; }

// The carve a launch uses: as many workgroups per CU as the form aims at (wide: one), fewer while the queues do not fit.
// Returns the workgroups per CU, or -1.
int carve(const scldpc_code_params *p, int32_t is_term, bool level, bool wide, SmArgs *a, int per_cu = kPerCu)
{
    if (wide) per_cu = 1;
    while (per_cu > 1 && make_args(p, is_term, a, per_cu, level, wide) != 0) per_cu--;
    return make_args(p, is_term, a, per_cu, level, wide) == 0 ? per_cu : -1;
}

// Which limit keeps this ensemble from the forms with 16-bit (wide = false) or 32-bit queue entries, reading the CN -> VN
// (sock = false) or the CN -> socket table; nullptr: none.  The wide forms' LEVEL carve at one workgroup per CU must leave
// kWideMinQueue entries per queue (a shorter queue would still decode correctly — overflow falls back to scan rounds — but is
// no fast path), and the packed reduction of the kernel needs nk / 16 + 64 (nk / qcap + 1) <= 32 767 (see there).
// deg: the entry points that take the degree pairs of pair_of() (socket table only), and with them the bounds of the
// kernel's packed reduction for the carve the launch will use, narrow or wide.
const char *shape_limit(const scldpc_code_params *p, bool wide, bool sock, bool deg = false)
{
    if (scldpc::check_params(p)) return "invalid code parameters";
    if (!deg) {
        if (p->dv != 4 || p->dc != 8) return "takes dv = 4, dc = 8 only";
    } else {
        if (p->dc > 15) return "dc must be at most 15 (a CN's count of erased neighbours is kept in 4 bits)";
        if (pair_of(p->dv, p->dc) < 0) {
            static thread_local char text[96];
            snprintf(text, sizeof text, "no instance for dv = %d, dc = %d (takes (3,6), (4,8) and (5,10))", p->dv, p->dc);
            return text;
        }
    }
    if (sock && (int64_t)p->vns_pos * p->dv > 65535) return "sockets: vns_pos * dv must fit 16 bits (at most 65535)";
    if (p->cns_pos > 65536) return "at most 65536 CNs per position (16-bit position-local CN ids)";
    const int64_t n64 = (int64_t)p->L * p->vns_pos, nk64 = (int64_t)(p->L + p->dv - 1) * p->cns_pos;
    if (!wide && nk64 > 65536) return "at most 65536 CNs per trial (16-bit queue entries; the _wide forms take more)";
    if (!sock && n64 >= 65535) return "global VN ids in the CN -> VN table: fewer than 65535 VNs (use the _sock16 form beyond)";
    if (n64 / 8 + nk64 / 2 > scldpc::kMaxLdsBytes) return "LDS: the CN counts and VN bits of a trial exceed 160 KiB";
    SmArgs a{};
    uint32_t m;
    if (!scldpc::magic_of(p->vns_pos, scldpc::n_of(p) + 32, &m) || !scldpc::magic_of(p->cns_pos, scldpc::nk_of(p), &m))
        return "no exact multiply-high division for this vns_pos / cns_pos";
    if (make_args(p, 1, &a, 1, wide, wide) != 0) return "LDS: the CN counts and VN bits of a trial leave no room for the queues";
    if (wide && a.qcap < kWideMinQueue) return "queue: the LDS left by the state holds fewer than 1024 entries per queue";
    if (wide && a.nk / 16 + 64 * (a.nk / a.qcap + 1) > 32767) return "queue: a wave's releases per iteration could exceed 15 bits";
    if (deg) {
        if (!wide && carve(p, 1, true, false, &a) < 0) return "LDS: the CN counts and VN bits of a trial leave no room for the queues";
        const int r = a.nk / (wide ? kBlockWide / 64 : kBlockSmall / 64) + 64 * (a.nk / a.qcap + 1);
        if (r > 32767) return "queue: a wave's releases per iteration could exceed 15 bits";
        if (p->dv * r >= (1 << 17)) return "queue: the CNs a wave zeroes per iteration could exceed 17 bits";
    }
    return nullptr;
}

}  // namespace

const char *scldpc::small_deg_shape_limit(const scldpc_code_params *p) { return shape_limit(p, false, true, true); }

// 1 when the _wide forms take this ensemble: 32-bit queue entries, one 1024-thread workgroup per CU
extern "C" int scldpc_full_bp_wide_supported(const scldpc_code_params *p) { return shape_limit(p, true, true) == nullptr; }

// 1 when the _cn16 forms take this ensemble (global VN ids in the CN -> VN table: n < 65535)
extern "C" int scldpc_full_bp_cn16_supported(const scldpc_code_params *p) { return shape_limit(p, false, false) == nullptr; }

// 1 when the _sock16 forms take this ensemble (sockets in the CN -> VN table: any n whose state fits the LDS)
extern "C" int scldpc_full_bp_sock16_supported(const scldpc_code_params *p) { return shape_limit(p, false, true) == nullptr; }

namespace {

// What an entry point asks of the kernel.  M_FIX: the fixpoint; M_LEVEL: one flooding iteration per barrier round; M_TRAJ: the
// same with the trajectory rows; M_CAPS: the same with a checkpoint at every cap.
enum Mode { M_FIX, M_LEVEL, M_TRAJ, M_CAPS };
constexpr bool kCnTable = false, kSockTable = true, kNarrow = false, kWide = true, kDeg = true;
struct Form {
    Mode mode;
    bool sock;          // the CN table holds sockets instead of global VN ids
    bool wide;          // 32-bit queue entries, one 1024-thread workgroup per CU (LEVEL, TRAJ or CAPS with sockets only)
    bool deg = false;   // the _deg entry points: the degree pair of the parameters picks the instance (sockets only)
    // the A/B knobs SCLDPC_DEBUG_GRID_DECODER and SCLDPC_DEBUG_LDS_PAD_DECODER act on these forms only.  The two knobs of the
    // tests act wherever they mean something (launch): SCLDPC_DEBUG_DECODER_QCAP shortens the queues of every form, and
    // SCLDPC_DEBUG_DECODER_KSWITCH moves the switch-over width of every fixpoint instance, the _deg ones included.
    bool knobs() const { return mode != M_CAPS && !wide && !deg; }
};

// the arguments of a call; an entry point leaves what it does not have at zero
struct Call {
    const scldpc_code_params *p;
    int32_t ntrials;
    const uint16_t *vn_adj16, *cn_adj16;
    const uint32_t *chan;
    int32_t max_it, is_term;
    int32_t *counters;
    uint32_t *erased;
    void *stream;
    int32_t *rows; int32_t rows_cap;                // TRAJ
    int32_t ncaps; const int32_t *caps;             // CAPS
};

using Kernel = void (*)(const SmArgs);
constexpr int form_key(Mode mode, bool sock, bool wide, bool persist, int pair = 0)
{
    return pair * 32 + mode * 8 + sock * 4 + wide * 2 + persist;
}

// The instances <BLOCK, LEVEL, PERSIST, SOCK, TRAJ, CAPS, WIDE, DV, DC> with their VGPRs / SGPRs at -O3 for gfx950; no scratch
// except where noted (as found; not looked into here).  persist: workgroup b decodes trials b, b + gridDim.x, … — reached through
// SCLDPC_DEBUG_GRID_DECODER only, CN -> VN table only.  pair: pair_of(dv, dc); the twelve (4,8) instances first, then five per
// further pair (socket table: fixpoint, LEVEL, TRAJ, wide LEVEL, wide TRAJ), then the five CAPS instances of the wide form and of
// the further pairs.  nullptr: no such instance.
Kernel kernel_of(const Form &f, bool persist, int pair = 0)
{
    constexpr int S = kBlockSmall, W = kBlockWide;
    switch (form_key(f.mode, f.sock, f.wide, persist, pair)) {
    case form_key(M_FIX, kCnTable, kNarrow, false):      return full_bp_small_kernel<S, false, false, false>;                   // 64 / 93
    case form_key(M_FIX, kSockTable, kNarrow, false):    return full_bp_small_kernel<S, false, false, true>;                    // 64 / 94
    case form_key(M_FIX, kCnTable, kNarrow, true):       return full_bp_small_kernel<S, false, true, false>;                    // 64 / 78, 136 B of scratch
    case form_key(M_LEVEL, kCnTable, kNarrow, false):    return full_bp_small_kernel<S, true, false, false>;                    // 63 / 94
    case form_key(M_LEVEL, kSockTable, kNarrow, false):  return full_bp_small_kernel<S, true, false, true>;                     // 63 / 94
    case form_key(M_LEVEL, kCnTable, kNarrow, true):     return full_bp_small_kernel<S, true, true, false>;                     // 64 / 78, 108 B of scratch
    case form_key(M_TRAJ, kCnTable, kNarrow, false):     return full_bp_small_kernel<S, true, false, false, true>;              // 67 / 94
    case form_key(M_TRAJ, kSockTable, kNarrow, false):   return full_bp_small_kernel<S, true, false, true, true>;               // 67 / 94
    case form_key(M_CAPS, kCnTable, kNarrow, false):     return full_bp_small_kernel<S, true, false, false, false, true>;       // 61 / 94
    case form_key(M_CAPS, kSockTable, kNarrow, false):   return full_bp_small_kernel<S, true, false, true, false, true>;        // 63 / 94
    case form_key(M_LEVEL, kSockTable, kWide, false):    return full_bp_small_kernel<W, true, false, true, false, false, true>; // 63 / 94
    case form_key(M_TRAJ, kSockTable, kWide, false):     return full_bp_small_kernel<W, true, false, true, true, false, true>;  // 67 / 94
    case form_key(M_FIX, kSockTable, kNarrow, false, 1):   return full_bp_small_kernel<S, false, false, true, false, false, false, 3, 6>;   // 65 / 94
    case form_key(M_LEVEL, kSockTable, kNarrow, false, 1): return full_bp_small_kernel<S, true, false, true, false, false, false, 3, 6>;    // 63 / 94
    case form_key(M_TRAJ, kSockTable, kNarrow, false, 1):  return full_bp_small_kernel<S, true, false, true, true, false, false, 3, 6>;     // 67 / 94
    case form_key(M_LEVEL, kSockTable, kWide, false, 1):   return full_bp_small_kernel<W, true, false, true, false, false, true, 3, 6>;     // 63 / 94
    case form_key(M_TRAJ, kSockTable, kWide, false, 1):    return full_bp_small_kernel<W, true, false, true, true, false, true, 3, 6>;      // 67 / 94
    case form_key(M_FIX, kSockTable, kNarrow, false, 2):   return full_bp_small_kernel<S, false, false, true, false, false, false, 5, 10>;  // 71 / 94
    case form_key(M_LEVEL, kSockTable, kNarrow, false, 2): return full_bp_small_kernel<S, true, false, true, false, false, false, 5, 10>;   // 67 / 94
    case form_key(M_TRAJ, kSockTable, kNarrow, false, 2):  return full_bp_small_kernel<S, true, false, true, true, false, false, 5, 10, 6>; // 77 / 94, six waves per SIMD (28 B of scratch at seven): per_cu_of
    case form_key(M_LEVEL, kSockTable, kWide, false, 2):   return full_bp_small_kernel<W, true, false, true, false, false, true, 5, 10>;    // 67 / 94
    case form_key(M_TRAJ, kSockTable, kWide, false, 2):    return full_bp_small_kernel<W, true, false, true, true, false, true, 5, 10>;     // 81 / 94
    case form_key(M_CAPS, kSockTable, kWide, false):       return full_bp_small_kernel<W, true, false, true, false, true, true>;            // 63 / 94
    case form_key(M_CAPS, kSockTable, kNarrow, false, 1):  return full_bp_small_kernel<S, true, false, true, false, true, false, 3, 6>;     // 61 / 94
    case form_key(M_CAPS, kSockTable, kNarrow, false, 2):  return full_bp_small_kernel<S, true, false, true, false, true, false, 5, 10>;    // 69 / 94
    case form_key(M_CAPS, kSockTable, kWide, false, 1):    return full_bp_small_kernel<W, true, false, true, false, true, true, 3, 6>;      // 61 / 94
    case form_key(M_CAPS, kSockTable, kWide, false, 2):    return full_bp_small_kernel<W, true, false, true, false, true, true, 5, 10>;     // 69 / 94
    }
    return nullptr;
}

// Workgroups per CU the carve of an instance aims at: the narrow forms' seven, except where kernel_of() bounds the registers
// for fewer waves per SIMD
int per_cu_of(const Form &f, int pair) { return f.wide ? 1 : (pair == pair_of(5, 10) && f.mode == M_TRAJ) ? 6 : kPerCu; }

// Every decoder entry point below is one call of this.  The checks come in one fixed order — the parameters, the form's own
// arguments (rows, caps), the shape, the buffers — so a call with several defects reports the first of these.  The shape is
// judged even for an empty batch, which needs no buffers.
int launch(const char *who, const Form &f, const Call &c)
{
    if (int rc = scldpc::check_params(c.p)) return rc;
    if (c.rows && c.rows_cap <= 0) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: d_rows given but rows_cap <= 0", who);
    if (f.mode == M_CAPS) {
        if (c.ncaps < 1 || c.ncaps > SCLDPC_MAX_CAPS || !c.caps)
            return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: takes 1 .. %d caps (ncaps = %d%s)", who, SCLDPC_MAX_CAPS, c.ncaps,
                                     c.caps ? "" : ", caps NULL");
        for (int k = 0; k < c.ncaps; k++)
            if (c.caps[k] < 1 || (k > 0 && c.caps[k] <= c.caps[k - 1]))
                return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: caps must be strictly increasing and >= 1 (caps[%d] = %d)", who,
                                         k, c.caps[k]);
    }
    if (const char *why = shape_limit(c.p, f.wide, f.sock, f.deg)) return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: %s", who, why);
    if (c.ntrials < 0 || (c.ntrials > 0 && (!c.counters || !c.vn_adj16 || !c.cn_adj16 || !c.chan)))
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer or negative ntrials", who);
    if (c.ntrials == 0) return SCLDPC_OK;

    SmArgs a{};
    const int pair = f.deg ? pair_of(c.p->dv, c.p->dc) : 0;
    if (carve(c.p, c.is_term, f.mode != M_FIX, f.wide, &a, per_cu_of(f, pair)) < 0)
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: LDS: the CN counts and VN bits do not fit", who);
    scldpc::magic_of(c.p->vns_pos, a.n + 32, &a.magic_v);
    scldpc::magic_of(c.p->cns_pos, a.nk, &a.magic_c);
    a.vn_adj16 = c.vn_adj16; a.cn_adj16 = c.cn_adj16; a.chan = c.chan;
    a.counters = c.counters; a.erased_out = c.erased;
    a.ntrials = c.ntrials;
    a.max_it = c.max_it;
    a.rows = c.rows; a.rows_cap = c.rows ? c.rows_cap : 0;
    a.ncaps = c.ncaps;
    for (int k = 0; k < c.ncaps; k++) a.caps[k] = c.caps[k];
    a.kswitch = kSwitchWidth;
    int grid = c.ntrials;
    size_t lds_bytes = 4u * (size_t)a.total;
    // tests and A/B only; a wave takes at most one entry per lane into its private queue, so the width is capped at 64 entries
    // per wave.  Only the fixpoint instances read it.
    if (f.mode == M_FIX)
        if (const char *v = getenv("SCLDPC_DEBUG_DECODER_KSWITCH")) a.kswitch = std::min(atoi(v), 64 * (kBlockSmall / 64));
    // tests only: shorter queues, so that small shapes clamp their scans, drop pushes and take their snapshots one queue-full
    // at a time (a private half-queue below 64 entries keeps the fixpoint form's waves on the shared queue).  It only ever
    // shrinks the queues; the LDS taken and its layout stay those of the full carve.
    if (const char *v = getenv("SCLDPC_DEBUG_DECODER_QCAP")) {
        a.qcap = std::max(kMinDebugQcap, std::min(atoi(v), a.qcap));
        // the kernel's packed reduction, for this queue: a wave releases at most nk / waves + 64 (nk / qcap + 1) VNs per
        // iteration, and never more than there are CNs (a CN is queued once per iteration)
        const int64_t waves = (f.wide ? kBlockWide : kBlockSmall) / 64;
        const int64_t r = std::min<int64_t>(a.nk, a.nk / waves + 64 * ((int64_t)a.nk / a.qcap + 1));
        if (r > 32767 || c.p->dv * r >= (1 << 17))
            return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: SCLDPC_DEBUG_DECODER_QCAP: with %d entries per queue a wave's releases "
                                     "per iteration could exceed the packed reduction's 15 / 17 bits at this shape", who, a.qcap);
    }
    if (f.knobs()) {
        grid = scldpc::debug_grid("DECODER", c.ntrials);
        lds_bytes = std::min(lds_bytes + scldpc::debug_lds_pad("DECODER"), (size_t)scldpc::kMaxLdsBytes);
    }
    if (f.sock && grid < c.ntrials)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: no persistent form with the socket table", who);
    // (as found: the rows form has no persistent instance either and takes a debug grid as it is — it then decodes the first
    // `grid` trials only)
    const Kernel kern = kernel_of(f, grid < c.ntrials && f.mode != M_TRAJ, pair);
    if (int rc = scldpc::allow_max_lds(reinterpret_cast<const void *>(kern))) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(f.wide ? kBlockWide : kBlockSmall), lds_bytes, static_cast<hipStream_t>(c.stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

}  // namespace

extern "C" int scldpc_full_bp_fixpoint_device_cn16(const scldpc_code_params *p, int32_t ntrials,
                                                   const uint16_t *d_vn_adj16, const uint16_t *d_cn_adj16,
                                                   const uint32_t *d_chan_bits, int32_t is_term, int32_t *d_counters,
                                                   uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_fixpoint_device_cn16", {M_FIX, kCnTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_adj16, d_chan_bits, 0, is_term, d_counters, d_erased_bits, stream});
}

// decodeBP with its iterations (count, cap MaxNumIt, stop tests): every counter of scldpc_full_bp_device, from both tables
extern "C" int scldpc_full_bp_device_cn16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                          const uint16_t *d_cn_adj16, const uint32_t *d_chan_bits, int32_t max_it,
                                          int32_t is_term, int32_t *d_counters, uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_device_cn16", {M_LEVEL, kCnTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_adj16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream});
}

// The same two decoders reading the CN -> SOCKET table of scldpc_sample_philox_device_sock16 / scldpc_cn_sockets_device
// (position-local 16-bit sockets): no limit on the number of VNs per trial — e.g. the published L = 100, N = 1000 runs.
extern "C" int scldpc_full_bp_fixpoint_device_sock16(const scldpc_code_params *p, int32_t ntrials,
                                                     const uint16_t *d_vn_adj16, const uint16_t *d_cn_sock16,
                                                     const uint32_t *d_chan_bits, int32_t is_term, int32_t *d_counters,
                                                     uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_fixpoint_device_sock16", {M_FIX, kSockTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, 0, is_term, d_counters, d_erased_bits, stream});
}

extern "C" int scldpc_full_bp_device_sock16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                            const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                            int32_t is_term, int32_t *d_counters, uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_device_sock16", {M_LEVEL, kSockTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream});
}

// decodeBP of the trajectory build (BPT:900-1140): the iterations with their rows — deg_1_iter, VNs recovered, position of the
// first erased VN (BPT:988, 1037-1038, 1051) — d_rows int32 [ntrials][rows_cap][3], d_counters[ITERATIONS] rows per trial.
extern "C" int scldpc_full_bp_traj_device_cn16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                               const uint16_t *d_cn_adj16, const uint32_t *d_chan_bits, int32_t max_it,
                                               int32_t is_term, int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                               uint32_t *d_erased_bits, void *stream)
{
    if (!d_rows) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "scldpc_full_bp_traj_device_cn16: null d_rows");
    return launch("scldpc_full_bp_traj_device_cn16", {M_TRAJ, kCnTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_adj16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream, d_rows, rows_cap});
}

extern "C" int scldpc_full_bp_traj_device_sock16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                 const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                                 int32_t is_term, int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                                 uint32_t *d_erased_bits, void *stream)
{
    if (!d_rows) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "scldpc_full_bp_traj_device_sock16: null d_rows");
    return launch("scldpc_full_bp_traj_device_sock16", {M_TRAJ, kSockTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream, d_rows, rows_cap});
}

// Several caps from one decode: block k of d_counters [ncaps][ntrials][8] is what scldpc_full_bp_device_*(max_it = caps[k])
// writes (include/scldpc.h)
extern "C" int scldpc_full_bp_caps_device_cn16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                               const uint16_t *d_cn_adj16, const uint32_t *d_chan_bits, int32_t ncaps,
                                               const int32_t *caps, int32_t is_term, int32_t *d_counters, void *stream)
{
    return launch("scldpc_full_bp_caps_device_cn16", {M_CAPS, kCnTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_adj16, d_chan_bits, 0, is_term, d_counters, nullptr, stream, nullptr, 0, ncaps, caps});
}

extern "C" int scldpc_full_bp_caps_device_sock16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                 const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t ncaps,
                                                 const int32_t *caps, int32_t is_term, int32_t *d_counters, void *stream)
{
    return launch("scldpc_full_bp_caps_device_sock16", {M_CAPS, kSockTable, kNarrow},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, 0, is_term, d_counters, nullptr, stream, nullptr, 0, ncaps, caps});
}

// The level-synchronous decoder for trials of more than 65536 CNs (32-bit queue entries, a 1024-thread workgroup per CU):
// arguments, counters, rows and cap blocks exactly as scldpc_full_bp_device_sock16 / scldpc_full_bp_traj_device_sock16 /
// scldpc_full_bp_caps_device_sock16
extern "C" int scldpc_full_bp_device_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                          const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                          int32_t is_term, int32_t *d_counters, uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_device_wide", {M_LEVEL, kSockTable, kWide},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream});
}

extern "C" int scldpc_full_bp_traj_device_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                               const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                               int32_t is_term, int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                               uint32_t *d_erased_bits, void *stream)
{
    if (!d_rows) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "scldpc_full_bp_traj_device_wide: null d_rows");
    return launch("scldpc_full_bp_traj_device_wide", {M_TRAJ, kSockTable, kWide},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream, d_rows, rows_cap});
}

extern "C" int scldpc_full_bp_caps_device_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                               const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t ncaps,
                                               const int32_t *caps, int32_t is_term, int32_t *d_counters, void *stream)
{
    return launch("scldpc_full_bp_caps_device_wide", {M_CAPS, kSockTable, kWide},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, 0, is_term, d_counters, nullptr, stream, nullptr, 0, ncaps, caps});
}

// The same five decoders for the regular pairs (3,6), (4,8) and (5,10): 4 bits of LDS per CN where scldpc_full_bp_device_adj16 and
// scldpc_full_bp_fixpoint_device_adj16 (decodeBP, BPF:900-1140; rows: the BPT build, BPT:988, 1037-1038, 1051) keep a 16-bit word.
// They read the 2-byte VN -> CN table [T][n][dv] of scldpc_sample_philox_device_adj16 and the CN -> socket table [T][nk][dc] of
// scldpc_cn_sockets_device; (4,8) runs the _sock16 / _wide instances.
extern "C" int scldpc_full_bp_deg_supported(const scldpc_code_params *p) { return shape_limit(p, false, true, true) == nullptr; }

extern "C" int scldpc_full_bp_deg_wide_supported(const scldpc_code_params *p) { return shape_limit(p, true, true, true) == nullptr; }

extern "C" int scldpc_full_bp_fixpoint_device_deg(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                  const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t is_term,
                                                  int32_t *d_counters, uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_fixpoint_device_deg", {M_FIX, kSockTable, kNarrow, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, 0, is_term, d_counters, d_erased_bits, stream});
}

extern "C" int scldpc_full_bp_device_deg(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                         const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                         int32_t is_term, int32_t *d_counters, uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_device_deg", {M_LEVEL, kSockTable, kNarrow, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream});
}

extern "C" int scldpc_full_bp_traj_device_deg(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                              const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                              int32_t is_term, int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                              uint32_t *d_erased_bits, void *stream)
{
    if (!d_rows) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "scldpc_full_bp_traj_device_deg: null d_rows");
    return launch("scldpc_full_bp_traj_device_deg", {M_TRAJ, kSockTable, kNarrow, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream, d_rows, rows_cap});
}

extern "C" int scldpc_full_bp_device_deg_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                              const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                              int32_t is_term, int32_t *d_counters, uint32_t *d_erased_bits, void *stream)
{
    return launch("scldpc_full_bp_device_deg_wide", {M_LEVEL, kSockTable, kWide, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream});
}

extern "C" int scldpc_full_bp_traj_device_deg_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                   const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t max_it,
                                                   int32_t is_term, int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                                   uint32_t *d_erased_bits, void *stream)
{
    if (!d_rows) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "scldpc_full_bp_traj_device_deg_wide: null d_rows");
    return launch("scldpc_full_bp_traj_device_deg_wide", {M_TRAJ, kSockTable, kWide, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, max_it, is_term, d_counters, d_erased_bits, stream, d_rows, rows_cap});
}

// Several caps from one decode for the same pairs: block k of d_counters [ncaps][ntrials][8] is what scldpc_full_bp_device_deg /
// _deg_wide (max_it = caps[k]) writes; the shapes of the level forms.  (4,8) runs the _sock16 / _wide caps instances.
extern "C" int scldpc_full_bp_caps_device_deg(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                              const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t ncaps,
                                              const int32_t *caps, int32_t is_term, int32_t *d_counters, void *stream)
{
    return launch("scldpc_full_bp_caps_device_deg", {M_CAPS, kSockTable, kNarrow, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, 0, is_term, d_counters, nullptr, stream, nullptr, 0, ncaps, caps});
}

extern "C" int scldpc_full_bp_caps_device_deg_wide(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                   const uint16_t *d_cn_sock16, const uint32_t *d_chan_bits, int32_t ncaps,
                                                   const int32_t *caps, int32_t is_term, int32_t *d_counters, void *stream)
{
    return launch("scldpc_full_bp_caps_device_deg_wide", {M_CAPS, kSockTable, kWide, kDeg},
                  {p, ntrials, d_vn_adj16, d_cn_sock16, d_chan_bits, 0, is_term, d_counters, nullptr, stream, nullptr, 0, ncaps, caps});
}
