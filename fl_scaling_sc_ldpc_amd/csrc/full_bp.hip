// Full flooding BP over the BEC for a batch of sampled SC-LDPC codes — gfx950 (MI355X) kernel.
//
// Replaces decodeBP of the reference (BPF:900-1140; BPT adds per-iteration rows and truncation,
// BPT:912-1051) bit for bit, but does O(E) work per trial instead of O(E·iterations):
// on the BEC, the a-posteriori erasure set after flooding iteration t equals the residual of
// level-synchronous parallel peeling after t rounds, so the kernel keeps
//   * one bit per VN  (U = currently erased VNs), and
//   * one small word per CN holding cnt = #erased neighbours and a fold (sum or xor) of their ids —
//     when cnt == 1 the fold IS the one erased neighbour, so only the VN→CN table is ever read
//     from HBM (no CN→VN lists, no per-edge messages),
// all of it in LDS (one workgroup = one trial), and walks a frontier of CNs with cnt == 1.
//
// Two CN-word layouts:
//   Wide   32 bit  [cnt:4 | deg:4 | Σ global VN id:24]   any ensemble that fits; needed for trajectories (deg)
//   Packed 16 bit  [cnt:4 | ⊕ local VN id:12]            when dv·vns_pos <= 4096 (local id = edge·vns_pos + t):
//                  half the LDS ⇒ two 1024-thread workgroups per CU hide each other's latencies.
//
// Iteration t of the reference == one frontier round (one barrier):
//   every CN with cnt == 1 at the start of the round releases its VN; the releasing thread fetches the
//   VN's dv CN ids (one 16-B load), decrements those CNs and queues the ones that drop 2 → 1.
//   deg_1_iter (BPF:969-978) needs no extra pass:  |F(t+1)| = pushes(t) − (drops_1→0(t) − |F(t)|).
// Afterwards the size-2 stopping-set expurgation (BPF:1067-1133) from the same CN words: an erased VN a
// belongs to such a pair iff every one of its CNs has cnt == 2 and the same partner, in a's position.
#include "flood_common.h"
#include "peel_fixpoint.h"

namespace {

using namespace scldpc_dev;

// per-iteration counters, rotated three ways so that one barrier per iteration is enough
enum { S_PUSH = 0, S_DROP = 3, S_REM = 6, S_OVF = 9, S_NE = 12, S_EXTRA0 = 13, S_VALID = 14, S_NSCAL = 16 };

using Layout = scldpc::FloodLayout;      // pos_a = erased VNs per position, pos_b = those in size-2 stopping sets

struct Args : Geo {             // Geo: vns_pos, magic_v, magic_c
    int dv, L, cns_pos, n, nk, cn_lim, max_it, rows_cap;
    int prebuilt;                   // WideG: the CN words were built by cn_build.hip (through LDS, not by global atomics)
    Layout lay;
    const void *vn_adj;             // int32 [T][n][dv] or uint16 [T][n][dv] (position-local ids)
    uint32_t *ws;                   // [T][nk] CN words in global memory (WideG only)
    const uint32_t *chan;
    int32_t *counters;
    int32_t *rows;
    uint32_t *erased_out;
};

template <class ST, bool TRAJ, int DV, bool A16, int BLOCK>
// Two 1024-thread workgroups per CU = 8 waves per SIMD, which the scalar file admits only up to 80 SGPRs per wave
// (⌊800 / (⌈sgpr/16⌉·16 + 16)⌋ waves): capped here, the overflow lives in VGPR lanes.
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_num_sgpr(72))) void full_bp_kernel(const Args a)
{
    extern __shared__ uint32_t lds[];
    const int trial = blockIdx.x;
    uint32_t *cn_state;
    if constexpr (ST::kGlobal) cn_state = a.ws + (size_t)trial * a.nk;
    else                       cn_state = lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *pos_cnt = reinterpret_cast<int *>(lds + a.lay.pos_a);
    int *pos_ss = reinterpret_cast<int *>(lds + a.lay.pos_b);
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    const int tid = threadIdx.x, lane = tid & 63;
    const int n = a.n, nk = a.nk, dv = (DV ? DV : a.dv), cn_lim = a.cn_lim, nw = a.lay.nw, qcap = a.lay.qcap;
    const int V = a.vns_pos;
    const char *adj = static_cast<const char *>(a.vn_adj) + (size_t)trial * n * dv * (A16 ? 2 : 4);
    const uint32_t *ch = a.chan + (size_t)trial * nw;

    // ---- load channel bits, clear CN words -------------------------------------------------
    const bool prebuilt = ST::kGlobal && a.prebuilt;
    if (!prebuilt) for (int c = tid; c < ST::words(nk); c += BLOCK) cn_state[c] = 0;
    int ne_local = load_channel<BLOCK>(ch, U, nw, n, tid);
    if (tid < S_NSCAL) scal[tid] = 0;
    for (int i = tid; i < a.L; i += BLOCK) { pos_cnt[i] = 0; pos_ss[i] = 0; }
    __syncthreads();
    STAMP_DECL
    STAMP(0);                                                       // clear + channel load
    ne_local = wave_sum(ne_local);
    if (lane == 0 && ne_local) atomicAdd(&scal[S_NE], ne_local);

    // Trajectory rows with packed words: deg_1_iter's iteration-0 quirk (BPF:969-978) asks for CNs of degree 1 whose only VN
    // is known.  Only the first and last dv-1 CN positions of the chain can have a degree below dc, so their degrees are
    // counted into a byte array that borrows queue 1 (first written by iteration 0's releases, after the scan has used it).
    constexpr bool kSideDeg = TRAJ && !ST::kHasDeg;
    uint32_t *degb = q[1];
    const int ms = dv - 1, tail0 = a.L * a.cns_pos;
    auto boundary = [&](int c) {                    // index into degb, or -1 for a CN of the chain's interior
        return c < ms * a.cns_pos ? c : c >= tail0 ? ms * a.cns_pos + (c - tail0) : -1;
    };
    if constexpr (kSideDeg) {
        for (int w = tid; w < (2 * ms * a.cns_pos + 3) / 4; w += BLOCK) degb[w] = 0;
        __syncthreads();
    }

    // ---- build: every erased VN adds itself to its dv CNs (TRAJ: every VN also adds to deg) ----
    build_cn_words<ST, DV, A16, BLOCK, TRAJ>(a, adj, dv, a.cns_pos, n, prebuilt ? n : tid, U, cn_state,
                                             [&](const Vn &, const int32_t (&c)[8], bool) {
        if constexpr (kSideDeg) {
            for (int i = 0; i < dv; i++) {
                const int b = boundary(c[i]);
                if (b >= 0) atomicAdd(&degb[b >> 2], 1u << ((b & 3) * 8));
            }
        }
    });
    __syncthreads();
    STAMP(1);                                                       // build

    int ne = scal[S_NE];
    const int nch = ne;
    int prec = n, iter = 0, ncur = 0, status = 0, rows_done = 0, nfront = 0;
    bool scan = true;                   // iteration 0 has no queue yet: frontier = all CNs with cnt == 1
    int first_word = 0;

    for (;;) {
        const int g = iter % 3, gn = (iter + 1) % 3;
        uint32_t *qc = q[iter & 1], *qn = q[(iter + 1) & 1];
        if (tid == 0) { scal[S_PUSH + gn] = 0; scal[S_DROP + gn] = 0; scal[S_REM + gn] = 0; scal[S_OVF + gn] = 0; }

        int removed = 0, drops = 0;
        auto release = [&](int c) {
            const int j = ST::lone_vn(cn_state, c, a);
            if (j < 0) return;                                      // its VN was just released via another CN
            const Vn v = make_vn(a, j);
            int32_t cc[8];
            load_adj<DV, A16>(adj, dv, j, v.pos, a.cns_pos, cc);    // issued before the ownership test: its latency
            const uint32_t bit = 1u << (j & 31);                    // overlaps the LDS round trip below
            const uint32_t old = atomicAnd(&U[j >> 5], ~bit);
            if (!(old & bit)) return;                               // lost the race for VN j
            removed++;
            uint32_t o[8];
#pragma unroll
            for (int i = 0; i < (DV ? DV : 8); i++)                 // the dv returning atomics go out back to back
                if (i < dv) o[i] = ST::remove_cnt(cn_state, cc[i], v, i, V);
#pragma unroll
            for (int i = 0; i < (DV ? DV : 8); i++)
                if (i < dv) ST::remove_fold(cn_state, cc[i], v, i, V);
#pragma unroll
            for (int i = 0; i < (DV ? DV : 8); i++) {
                if (i < dv && cc[i] < cn_lim) {
                    drops += (o[i] == 1u);
                    if (o[i] == 2u) {                               // 2 → 1: candidate for the next round
                        const int idx = atomicAdd(&scal[S_PUSH + g], 1);
                        if (idx < qcap) qn[idx] = (uint32_t)cc[i]; else scal[S_OVF + g] = 1;
                    }
                }
            }
        };
        if (scan) {
            // snapshot {c < cn_lim : cnt == 1} first: this round's releases must not promote CNs into it
            int valid = 0, extra = 0;
            snapshot_frontier<BLOCK>(fbits, 0, cn_lim, tid, [&](int c) {
                bool v = false;
                if (c < cn_lim) {
                    const uint32_t k = ST::cnt(cn_state, c);
                    v = k == 1u;
                    if (TRAJ && iter == 0) {                        // degree-1 CN whose only VN is known (BPF:973)
                        uint32_t d;
                        if constexpr (kSideDeg) { const int b = boundary(c); d = b < 0 ? 0xFFu : (degb[b >> 2] >> ((b & 3) * 8)) & 0xFFu; }
                        else                    d = ST::deg(cn_state, c);
                        extra += (k == 0u && d == 1u);
                    }
                }
                valid += v;
                return v;
            });
            if (iter == 0) {
                valid = wave_sum(valid);
                if (lane == 0 && valid) atomicAdd(&scal[S_VALID], valid);
                if (TRAJ) {
                    extra = wave_sum(extra);
                    if (lane == 0 && extra) atomicAdd(&scal[S_EXTRA0], extra);
                }
            }
            __syncthreads();
            if (iter == 0) nfront = scal[S_VALID];
            sweep_frontier<BLOCK>(fbits, 0, cn_lim, tid, release);
        } else {
            for (int k = tid; k < ncur; k += BLOCK) release((int)qc[k]);
        }
        STAMP(2);                                                   // release
        {   // one DPP reduction for both counts (each < 2^16 per wave)
            const uint32_t both = wave_inclusive_scan(((uint32_t)removed << 16) | (uint32_t)drops);
            if (lane == 63 && both) {
                if (both >> 16) atomicAdd(&scal[S_REM + g], (int)(both >> 16));
                if (both & 0xFFFFu) atomicAdd(&scal[S_DROP + g], (int)(both & 0xFFFFu));
            }
        }
        STAMP(3);                                                   // wave reductions
        __syncthreads();                                            // end of flooding iteration `iter`
        STAMP(4);                                                   // barrier wait

        // ---- bookkeeping, identical in every thread ----------------------------------------
        const int deg1 = nfront + ((TRAJ && iter == 0) ? scal[S_EXTRA0] : 0);
        ne -= scal[S_REM + g];
        const int recovered = prec - ne;
        if (TRAJ && (tid >> 6) == 0 && a.rows && rows_done < a.rows_cap) {
            // first erased VN (BPT:1037-1038): U only loses bits, so resume from the last hit
            int fw = first_word, first = n;
            while (fw < nw) {
                const uint32_t w = (fw + lane < nw) ? U[fw + lane] : 0u;
                const unsigned long long m = __ballot(w != 0u);
                if (m) {
                    const int l0 = __ffsll((long long)m) - 1;
                    const uint32_t w0 = __shfl(w, l0, 64);
                    fw += l0;
                    first = fw * 32 + (__ffs((int)w0) - 1);
                    break;
                }
                fw += 64;
            }
            first_word = fw;
            if (lane == 0) {
                int32_t *r = a.rows + ((size_t)trial * a.rows_cap + rows_done) * 3;
                r[0] = deg1; r[1] = recovered; r[2] = first / V;
            }
        }
        if (TRAJ) __syncthreads();      // wave 0 read U above: keep the next round's releases behind it
        rows_done++;
        if (deg1 < recovered && iter > 0) { status = -1; break; }   // BPF:1035-1039
        if (ne == 0 || ne == prec) break;                           // BPF:1044-1045
        prec = ne;
        // frontier of the next round: queued 2→1 CNs minus those that went on to 0 within this round
        nfront = scal[S_PUSH + g] - (scal[S_DROP + g] - nfront);
        scan = scal[S_OVF + g] != 0;
        ncur = scan ? 0 : scal[S_PUSH + g];
        iter++;
        if (a.max_it > 0 && iter >= a.max_it) break;                // BPF:1065
        STAMP(5);                                                   // bookkeeping
    }
    __syncthreads();
    STAMP(5);

    // ---- per-position erasure counts + size-2 stopping sets (BPF:1067-1133) -----------------
    if (ne > 0)
        count_size2_sets<ST, DV, A16, BLOCK>(a, adj, dv, a.cns_pos, cn_state, U, nw, tid, pos_ss,
                                             [&](const Vn &v) { atomicAdd(&pos_cnt[v.pos], 1); });
    __syncthreads();
    STAMP(6);                                                       // final counts + expurgation
    STAMP_FLUSH();
    store_bits<BLOCK>(a.erased_out, trial, U, nw, tid);
    if (tid == 0)
        write_full_bp_counters(a.counters + (size_t)trial * SCLDPC_NCOUNTERS, pos_cnt, pos_ss, a.L, ne, rows_done, status, nch);
}

// =================================================================================================
// Fixpoint variant: the residual of UNLIMITED flooding without walking its iterations one barrier at a time.
//
// On the BEC the set flooding BP converges to is the closure of "a CN with exactly one erased neighbour resolves it" and
// does not depend on the order in which CNs fire — only the iteration COUNT does.  When nobody asks
// for the count (no iteration cap, no trajectory rows) a lane that has released a VN may therefore go straight on with a
// CN that this very release left with one erased neighbour, instead of queueing it for the next barrier round: the
// ~230 dependent levels of a trial at eps = 0.48 become ~230 steps of (one row gather + two rounds of LDS atomics) in a
// row, with a barrier only when chains end and work is redistributed.  Everything reported except
// SCLDPC_C_ITERATIONS (here: the number of barrier rounds) is identical to full_bp_kernel's — tests compare them.
//
// The barrier-free loop and the update protocol that makes it safe live in peel_fixpoint.h.
// =================================================================================================
template <bool A16, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_num_sgpr(72))) void full_bp_fixpoint_kernel(const Args a)
{
    using ST = Packed;
    constexpr int DV = 4;
    extern __shared__ uint32_t lds[];
    const int trial = blockIdx.x;
    uint32_t *cn_state = lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *pos_cnt = reinterpret_cast<int *>(lds + a.lay.pos_a);
    int *pos_ss = reinterpret_cast<int *>(lds + a.lay.pos_b);
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    const int tid = threadIdx.x, lane = tid & 63;
    const int n = a.n, nk = a.nk, cn_lim = a.cn_lim, nw = a.lay.nw, qcap = a.lay.qcap;
    const int V = a.vns_pos, C = a.cns_pos, L = a.L;
    const char *adj = static_cast<const char *>(a.vn_adj) + (size_t)trial * n * DV * (A16 ? 2 : 4);
    const uint32_t *ch = a.chan + (size_t)trial * nw;

    for (int c = tid; c < ST::words(nk); c += BLOCK) cn_state[c] = 0;
    int ne_local = load_channel<BLOCK>(ch, U, nw, n, tid);
    if (tid < S_NSCAL) scal[tid] = 0;
    for (int i = tid; i < L; i += BLOCK) { pos_cnt[i] = 0; pos_ss[i] = 0; }
    __syncthreads();
    ne_local = wave_sum(ne_local);
    if (lane == 0 && ne_local) atomicAdd(&scal[S_NE], ne_local);
    build_cn_words<ST, DV, A16, BLOCK, false>(a, adj, DV, C, n, tid, U, cn_state, [](const Vn &, const int32_t (&)[8], bool) {});
    __syncthreads();
    STAMP_DECL
    STAMP(0);                                                       // channel + build
    const int nch = scal[S_NE];

    int removed = 0;
    PeelCtx x{L, V, C, cn_lim, qcap, adj, cn_state, U, fbits, q[0], q[1], &scal[S_PUSH], &scal[S_OVF]};
    const int rounds = peel_to_fixpoint<A16, BLOCK>(a, x, removed);
    STAMP(1);                                                       // peeling (barrier rounds + barrier-free phase)
    removed = wave_sum(removed);
    if (lane == 0 && removed) atomicAdd(&scal[S_REM], removed);
    __syncthreads();
    const int ne = nch - scal[S_REM];

    // ---- per-position erasure counts + size-2 stopping sets (BPF:1067-1133), as in full_bp_kernel ----
    if (ne > 0)
        count_size2_sets<ST, DV, A16, BLOCK>(a, adj, DV, C, cn_state, U, nw, tid, pos_ss,
                                             [&](const Vn &v) { atomicAdd(&pos_cnt[v.pos], 1); });
    __syncthreads();
    STAMP(2);                                                       // final counts + expurgation
    STAMP_FLUSH();
    store_bits<BLOCK>(a.erased_out, trial, U, nw, tid);
    if (tid == 0)                                                   // ITERATIONS = barrier rounds, NOT flooding iterations
        write_full_bp_counters(a.counters + (size_t)trial * SCLDPC_NCOUNTERS, pos_cnt, pos_ss, L, ne, rounds, 0, nch);
}

// what a workgroup keeps in LDS for a CN-word form (scldpc::FloodWords)
scldpc::FloodRegions regions_of(const scldpc_code_params *p, int words)
{
    return {scldpc::flood_cn_lds_words(words, scldpc::nk_of(p)), false, p->L, p->L, 256};
}

bool packed_ok(const scldpc_code_params *p)
{
    return (int64_t)p->dv * p->vns_pos <= 4096 && p->dc <= 15 && p->dv <= 8;
}

}  // namespace

extern "C" int64_t scldpc_full_bp_lds_bytes(const scldpc_code_params *p)
{
    using namespace scldpc;
    if (int rc = check_params(p)) return rc;
    Layout lay;
    if (packed_ok(p) && flood_carve(p, regions_of(p, kWordsPacked), kHalfLdsBytes, &lay) == 0) return 4ll * lay.total;
    if (flood_carve(p, regions_of(p, kWordsWide), kMaxLdsBytes, &lay) == 0) return 4ll * lay.total;
    if (flood_carve(p, regions_of(p, kWordsGlobal), kMaxLdsBytes, &lay) == 0) return 4ll * lay.total;   // CN words in the workspace
    return 4ll * nw_of(p) + (64 << 10);
}

static int launch_full_bp(const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                          const uint32_t *d_chan_bits, int32_t max_it, int32_t is_term,
                          int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                          uint32_t *d_erased_bits, const scldpc::Scratch &scratch, void *stream)
{
    using namespace scldpc;
    const char *who = "scldpc_full_bp_device";
    if (int rc = check_params(p)) return rc;
    if (int rc = flood_check_call(who, scratch, ntrials, !d_counters || !d_vn_adj || !d_chan_bits)) return rc;
    if (d_rows && rows_cap <= 0)
        return set_error(SCLDPC_ERR_BAD_ARG, "scldpc_full_bp_device: d_rows given but rows_cap <= 0");
    if (ntrials <= 0) return SCLDPC_OK;
    const int n = n_of(p), nk = nk_of(p);
    if (!flood_limits_ok(p))
        return set_error(SCLDPC_ERR_TOO_LARGE,
                         "scldpc_full_bp_device: needs dc <= 15, dv <= 8, dc*n < 2^24 (got dc=%d dv=%d n=%d)", p->dc, p->dv, n);
    const bool traj = d_rows != nullptr;
    Args a{};
    int words;
    auto carve = [&](int w) {
        // packed words: always two workgroups per CU (trajectory rows: the side array of boundary degrees must fit queue 1)
        if (w == kWordsPacked)
            return flood_carve(p, regions_of(p, w), kHalfLdsBytes, &a.lay) == 0 &&
                   (!traj || 2 * (p->dv - 1) * p->cns_pos <= 4 * a.lay.qcap);
        return flood_carve_roomy(p, regions_of(p, w), &a.lay);
    };
    if (int rc = flood_choose_words(who, "scldpc_full_bp_device: n=%d VN bits + nk=%d scan bits do not fit 160 KiB of LDS", p,
                                    ntrials, scratch, packed_ok(p), carve, &words, &a.ws)) return rc;
    if (words == kWordsQueryDone) return SCLDPC_OK;
    a.dv = p->dv; a.L = p->L; a.cns_pos = p->cns_pos; a.n = n; a.nk = nk;
    a.cn_lim = is_term ? nk : p->L * p->cns_pos;                    // BPT:944-948
    a.max_it = max_it; a.rows_cap = traj ? rows_cap : 0;
    if (int rc = flood_geo("scldpc_full_bp_device: reciprocal division inexact for this size", p, n, &a)) return rc;
    a.vn_adj = d_vn_adj; a.chan = d_chan_bits; a.counters = d_counters; a.rows = d_rows;
    a.erased_out = d_erased_bits;

    void (*kern)(const Args) = flood_pick(words, p->dv == 4, adj16, [&](auto st, auto dv, auto a16) -> void (*)(const Args) {
        using ST = decltype(st);
        constexpr int DV = decltype(dv)::value;
        constexpr bool A16 = decltype(a16)::value;
        return traj ? full_bp_kernel<ST, true, DV, A16, 1024> : full_bp_kernel<ST, false, DV, A16, 1024>;
    });
    if (words == kWordsGlobal && adj16)
        a.prebuilt = flood_prebuild("SCLDPC_DEBUG_FULLBP_PREBUILD", p, ntrials, d_vn_adj, d_chan_bits, a.ws, traj, stream);
    return flood_launch(kern, ntrials, 1024, stream, a);
}

extern "C" int scldpc_full_bp_device(const scldpc_code_params *p, int32_t ntrials,
                                     const int32_t *d_vn_adj, const uint32_t *d_chan_bits,
                                     int32_t max_it, int32_t is_term,
                                     int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                     uint32_t *d_erased_bits, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_full_bp(p, ntrials, d_vn_adj, false, d_chan_bits, max_it, is_term, d_counters, d_rows, rows_cap,
                          d_erased_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

extern "C" int scldpc_full_bp_device_adj16(const scldpc_code_params *p, int32_t ntrials,
                                           const uint16_t *d_vn_adj16, const uint32_t *d_chan_bits,
                                           int32_t max_it, int32_t is_term,
                                           int32_t *d_counters, int32_t *d_rows, int32_t rows_cap,
                                           uint32_t *d_erased_bits, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_full_bp(p, ntrials, d_vn_adj16, true, d_chan_bits, max_it, is_term, d_counters, d_rows, rows_cap,
                          d_erased_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

// workspace of scldpc_full_bp_device(_adj16) / scldpc_full_bp_fixpoint_device(_adj16) for ntrials trials (rows: trajectory mode)
int64_t scldpc_full_bp_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t want_rows)
{
    uint64_t need = 0;
    int32_t dummy_rows = 0;
    const int rc = launch_full_bp(p, ntrials, nullptr, true, nullptr, 0, 1, nullptr, want_rows ? &dummy_rows : nullptr,
                                  want_rows ? 1 : 0, nullptr, scldpc::Scratch{nullptr, 0, &need}, nullptr);
    return rc ? (int64_t)rc : (int64_t)need;
}

// The fixpoint of unlimited flooding by chain-following peeling (full_bp_fixpoint_kernel).  Ensembles the packed words do
// not cover (dv != 4, dv*vns_pos > 4096, LDS) take the level-synchronous kernel: same results, ITERATIONS = flooding iterations.
static int launch_full_bp_fixpoint(const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                                   const uint32_t *d_chan_bits, int32_t is_term, int32_t *d_counters,
                                   uint32_t *d_erased_bits, const scldpc::Scratch &scratch, void *stream)
{
    using namespace scldpc;
    if (int rc = check_params(p)) return rc;
    Args a{};
    const bool ok = p->dv == 4 && packed_ok(p) && flood_carve(p, regions_of(p, kWordsPacked), kHalfLdsBytes, &a.lay) == 0;
    if (!ok)
        return launch_full_bp(p, ntrials, d_vn_adj, adj16, d_chan_bits, 0, is_term, d_counters, nullptr, 0, d_erased_bits,
                              scratch, stream);
    if (int rc = flood_check_call("scldpc_full_bp_fixpoint_device", Scratch{}, ntrials, !d_counters || !d_vn_adj || !d_chan_bits))
        return rc;
    if (ntrials == 0) return SCLDPC_OK;
    const int n = n_of(p), nk = nk_of(p);
    a.dv = p->dv; a.L = p->L; a.cns_pos = p->cns_pos; a.n = n; a.nk = nk;
    a.cn_lim = is_term ? nk : p->L * p->cns_pos;                    // BPT:944-948
    // peel_to_fixpoint divides a local id (< dv*vns_pos <= 4096) by vns_pos as well
    if (int rc = flood_geo("scldpc_full_bp_fixpoint_device: reciprocal division inexact for this size", p, n > 4096 ? n : 4096, &a))
        return rc;
    a.vn_adj = d_vn_adj; a.chan = d_chan_bits; a.counters = d_counters; a.erased_out = d_erased_bits;
    void (*kern)(const Args) = adj16 ? full_bp_fixpoint_kernel<true, 1024> : full_bp_fixpoint_kernel<false, 1024>;
    return flood_launch(kern, ntrials, 1024, stream, a);
}

extern "C" int scldpc_full_bp_fixpoint_device(const scldpc_code_params *p, int32_t ntrials,
                                              const int32_t *d_vn_adj, const uint32_t *d_chan_bits, int32_t is_term,
                                              int32_t *d_counters, uint32_t *d_erased_bits, void *d_workspace,
                                              uint64_t workspace_bytes, void *stream)
{
    return launch_full_bp_fixpoint(p, ntrials, d_vn_adj, false, d_chan_bits, is_term, d_counters, d_erased_bits,
                                   scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

extern "C" int scldpc_full_bp_fixpoint_device_adj16(const scldpc_code_params *p, int32_t ntrials,
                                                    const uint16_t *d_vn_adj16, const uint32_t *d_chan_bits, int32_t is_term,
                                                    int32_t *d_counters, uint32_t *d_erased_bits, void *d_workspace,
                                                    uint64_t workspace_bytes, void *stream)
{
    return launch_full_bp_fixpoint(p, ntrials, d_vn_adj16, true, d_chan_bits, is_term, d_counters, d_erased_bits,
                                   scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}
