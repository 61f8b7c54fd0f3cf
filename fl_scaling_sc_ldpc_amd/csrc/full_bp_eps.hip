// Unlimited full BP of one sampled code at every point of a descending eps grid, in one launch (include/scldpc_bp_eps.h) —
// gfx950 kernel.
//
// On the BEC the set flooding BP converges to is the maximal stopping set inside the erased set E over the CNs below cn_lim
// (full_bp_fixpoint_kernel rests on it): the order in which CNs fire does not matter, only the iteration
// count does, and nobody asks for it here.  Maximal stopping sets are monotone in E, and that of E' ⊆ E lies inside the
// residual R of E: fixpoint(E') = fixpoint(R ∩ E').  The erased sets of a descending grid are nested, so stage k peels
// U = R_{k-1} ∩ {lev > k} instead of {lev > k}, exactly as peel_sweep_eps_kernel does for the sweep decoder; full BP has no
// sweep start, so there is no exception to the identity.  (With an iteration cap the result depends on the schedule: the
// entry takes none.)
//
// Per trial, one 1024-thread workgroup, built on flood_common.h (the same CN-word forms, rows and dv instances as
// full_bp_kernel).  The levels pass, the stage's U, the rebuild and the rounds are peel_sweep_eps_kernel's — kept as a copy
// here, not shared through a header: that kernel's stage goes on into PD's lost / component pass on REBUILT CN words, this one
// ends on the words as the peeling left them, and a shared body would have to be cut at every place where the two differ
// (cn_lim, the per-position arrays, what is cleared when) while that kernel's generated code must not move.
//   end of stage k  the CN words hold the counts over the residual R_k, which is the state full_bp_fixpoint_kernel ends on:
//            count_size2_sets with the per-position counts, write_full_bp_counters(ne = |R_k|, the stage's rounds, status 0,
//            #erased at point k), the erased bits.
//   Once R is empty every later point's row is zeros with its #erased, and the loop ends.
// pos_a holds pos_cnt [L] and pos_ss [L]; pos_b holds R (nw words) and the level counts (kBins words).
#include "flood_common.h"
#include "../../include/scldpc_bp_eps.h"
#include <string>

namespace {

using namespace scldpc_dev;

constexpr int kBlock = 1024;
constexpr int kBins = SCLDPC_EPS_MAX_POINTS + 4;        // level counts [0, K], rounded to 16 bytes
enum { S_PUSH = 0, S_OVF = 3, S_RCNT = 12, S_NSCAL = 16 };

using Layout = scldpc::FloodLayout;      // pos_a = pos_cnt, pos_ss; pos_b = R (nw words) + the level counts (kBins words)

struct Args : Geo {             // Geo: vns_pos, magic_v, magic_c
    int dv, L, cns_pos, n, ncn, cn_lim, npoints, ntrials, lev_wide;
    Layout lay;
    const void *vn_adj;
    const uint8_t *levels;      // [T][n]
    int32_t *counters;          // [K][T][SCLDPC_NCOUNTERS]
    uint32_t *erased_out;       // optional [K][T][nw]
    uint32_t *ws;               // [T][ncn] CN words in global memory (ensembles beyond the LDS)
};

// bits (lev > k) of the 32 VNs of word w; wide: the row is 4-byte aligned and n % 4 == 0.  per(l): called with every level.
template <class Per>
__device__ __forceinline__ uint32_t level_word(const uint8_t *lv, int w, int n, bool wide, uint32_t k, Per &&per)
{
    uint32_t x = 0;
    const int j0 = w * 32;
    if (wide) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            if (j0 + 4 * q >= n) break;                             // n % 4 == 0: a whole group or none
            const uint32_t v = *reinterpret_cast<const uint32_t *>(lv + j0 + 4 * q);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t l = (v >> (8 * u)) & 0xFFu;
                per(l);
                x |= (uint32_t)(l > k) << (4 * q + u);
            }
        }
    } else {
        for (int b = 0; b < 32 && j0 + b < n; b++) {
            const uint32_t l = lv[j0 + b];
            per(l);
            x |= (uint32_t)(l > k) << b;
        }
    }
    return x;
}

// Two 1024-thread workgroups per CU (8 waves per SIMD: at most 64 VGPRs, and 72 SGPRs as in full_bp.hip) wherever the LDS
// admits them, as peel_sweep_eps_kernel.  No spills: `make resources`, DESIGN.md.
template <int DV, bool A16, class ST>
__global__ __launch_bounds__(kBlock, 8) __attribute__((amdgpu_num_sgpr(72))) void full_bp_eps_kernel(const Args a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cn_state = ST::kGlobal ? a.ws + (size_t)blockIdx.x * a.ncn : lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *R = lds + a.lay.pos_b;
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *pos_cnt = reinterpret_cast<int *>(lds + a.lay.pos_a);
    int *pos_ss = pos_cnt + a.L;
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    int tid = threadIdx.x, lane = tid & 63;
    const int trial = blockIdx.x;
    const int n = a.n, ncn = a.ncn, dv = (DV ? DV : a.dv), cn_lim = a.cn_lim, nw = a.lay.nw, qcap = a.lay.qcap;
    const int K = a.npoints;
    int *bins = reinterpret_cast<int *>(R + ((nw + 3) & ~3));       // [K + 1]; after the suffix sums bins[k + 1] = #erased at point k
    const char *adj = static_cast<const char *>(a.vn_adj) + (size_t)trial * n * dv * (A16 ? 2 : 4);
    const uint8_t *lv = a.levels + (size_t)trial * n;
    const bool wide = a.lev_wide != 0;

    // ---- the levels, once: U = {lev >= 1} and the counts of the levels
    if (tid < kBins) bins[tid] = 0;
    __syncthreads();
    {
        int top = 0;
        for (int w = tid; w < nw; w += kBlock)
            U[w] = level_word(lv, w, n, wide, 0u, [&](uint32_t l) {
                if (l >= (uint32_t)K) top++;                        // (a byte above K is erased at every point, as K is)
                else if (l) atomicAdd(&bins[l], 1);
            });
        const uint32_t tot = wave_inclusive_scan((uint32_t)top);
        if (lane == 63 && tot) atomicAdd(&bins[K], (int)tot);
    }
    __syncthreads();
    if (tid == 0)
        for (int l = K - 1; l >= 1; l--) bins[l] += bins[l + 1];
    // (the first barrier of stage 0 orders this before any read of bins)

    int stage = 0, iter = 0;
    for (; stage < K; stage++) {
        // (tid made opaque per stage, as in peel_sweep_eps_kernel: what the phases derive from it is computed again in every
        // stage instead of being kept in registers across the loop)
        asm volatile("" : "+v"(tid));
        lane = tid & 63;
        // ---- U of this stage, the CN words over it
        if (stage > 0)
            for (int w = tid; w < nw; w += kBlock) {
                const uint32_t r = R[w];
                U[w] = r ? r & level_word(lv, w, n, wide, (uint32_t)stage, [](uint32_t) {}) : 0u;
            }
        for (int c = tid; c < ST::words(ncn); c += kBlock) cn_state[c] = 0;
        if (tid < S_NSCAL) scal[tid] = 0;
        for (int i = tid; i < 2 * a.L; i += kBlock) pos_cnt[i] = 0;  // pos_cnt and pos_ss
        __syncthreads();
        if (stage == 0) {
            build_cn_words<ST, DV, A16, kBlock, false>(a, adj, dv, a.cns_pos, n, tid, U, cn_state,
                                                       [](const Vn &, const int32_t (&)[8], bool) {});
        } else {
            for (int w = tid; w < nw; w += kBlock) {
                uint32_t x = U[w];
                while (x) {
                    const int b = __ffs((int)x) - 1;
                    x &= x - 1;
                    const Vn v = make_vn(a, w * 32 + b);
                    int32_t cc[8];
                    load_adj<DV, A16>(adj, dv, v.j, v.pos, a.cns_pos, cc);
                    for (int i = 0; i < dv; i++) ST::add(cn_state, cc[i], v, i, a.vns_pos, true, false);
                }
            }
        }
        __syncthreads();

        // ---- peeling to the fixpoint (the order is irrelevant for the residual): a scan of every CN < cn_lim holding one
        //      VN, then queue rounds, a re-scan after a queue overflow ----
        int ncur = 0;
        bool scan = true;
        iter = 0;
        for (;;) {
            const int g = iter % 3, gn = (iter + 1) % 3;
            uint32_t *qc = q[iter & 1], *qn = q[(iter + 1) & 1];
            if (tid == 0) { scal[S_PUSH + gn] = 0; scal[S_OVF + gn] = 0; }
            auto release = [&](int c) {
                const int j = ST::lone_vn(cn_state, c, a);
                if (j < 0) return;
                const Vn v = make_vn(a, j);
                int32_t cc[8];
                load_adj<DV, A16>(adj, dv, j, v.pos, a.cns_pos, cc);
                const uint32_t bit = 1u << (j & 31);
                if (!(atomicAnd(&U[j >> 5], ~bit) & bit)) return;
                uint32_t o[8];
                for (int i = 0; i < dv; i++) o[i] = ST::remove_cnt(cn_state, cc[i], v, i, a.vns_pos);
                for (int i = 0; i < dv; i++) ST::remove_fold(cn_state, cc[i], v, i, a.vns_pos);
                for (int i = 0; i < dv; i++) {
                    if (o[i] == 2u && cc[i] < cn_lim) {             // transition to one VN: fires in the next round
                        const int idx = atomicAdd(&scal[S_PUSH + g], 1);
                        if (idx < qcap) qn[idx] = (uint32_t)cc[i]; else scal[S_OVF + g] = 1;
                    }
                }
            };
            if (scan) {
                // every CN < cn_lim holding one VN: all of them at the outset, and after a queue overflow those that got
                // there by a transition
                snapshot_frontier<kBlock>(fbits, 0, cn_lim, tid, [&](int c) { return c < cn_lim && ST::cnt(cn_state, c) == 1u; });
                __syncthreads();
                sweep_frontier<kBlock>(fbits, 0, cn_lim, tid, release);
            } else {
                for (int k = tid; k < ncur; k += kBlock) release((int)qc[k]);
            }
            __syncthreads();
            const bool ovf = scal[S_OVF + g] != 0;
            ncur = ovf ? 0 : scal[S_PUSH + g];
            iter++;
            if (ovf) { scan = true; continue; }
            scan = false;
            if (ncur == 0) break;                                   // nothing queued: fixpoint
        }
        __syncthreads();

        // ---- R := the residual; decodeBP's end on the CN words as the peeling left them (BPF:1067-1133) ----
        {
            int rc = 0;
            for (int w = tid; w < nw; w += kBlock) {
                const uint32_t x = U[w];
                R[w] = x;
                rc += __popc(x);
            }
            const uint32_t tot = wave_inclusive_scan((uint32_t)rc);
            if (lane == 63 && tot) atomicAdd(&scal[S_RCNT], (int)tot);
        }
        __syncthreads();
        const int residual = scal[S_RCNT];
        if (residual == 0) break;                                   // the same answer in every thread; the tail below writes the rows
        count_size2_sets<ST, DV, A16, kBlock>(a, adj, dv, a.cns_pos, cn_state, U, nw, tid, pos_ss,
                                              [&](const Vn &v) { atomicAdd(&pos_cnt[v.pos], 1); });
        __syncthreads();
        const size_t row = (size_t)stage * a.ntrials + trial;
        if (a.erased_out)
            for (int w = tid; w < nw; w += kBlock) a.erased_out[row * nw + w] = U[w];
        if (tid == 0)                                               // ITERATIONS = the peeling rounds of this stage
            write_full_bp_counters(a.counters + row * SCLDPC_NCOUNTERS, pos_cnt, pos_ss, a.L, residual, iter, 0, bins[stage + 1]);
        __syncthreads();                                            // the next stage clears scal and the position arrays, and rewrites U
    }

    // ---- the residual is empty from `stage` on (stage == K: every point has its row): rows of zeros with the #erased; the
    //      stage that found it empty keeps its rounds
    for (int k = stage + tid; k < K; k += kBlock) {
        int32_t *o = a.counters + ((size_t)k * a.ntrials + trial) * SCLDPC_NCOUNTERS;
        o[SCLDPC_C_NUM_ERASURES] = 0; o[SCLDPC_C_NUM_BLOCKS_ERR] = 0; o[SCLDPC_C_NUM_ERASURES_EXP] = 0;
        o[SCLDPC_C_NUM_BLOCKS_ERR_EXP] = 0; o[SCLDPC_C_NUM_ERASURES_P1] = 0;
        o[SCLDPC_C_ITERATIONS] = k == stage ? iter : 0;
        o[SCLDPC_C_STATUS] = 0;
        o[SCLDPC_C_CHANNEL_ERASURES] = bins[k + 1];
    }
    if (a.erased_out)
        for (int k = stage; k < K; k++)
            for (int w = tid; w < nw; w += kBlock) a.erased_out[((size_t)k * a.ntrials + trial) * nw + w] = 0u;
}

}  // namespace

static int launch_full_bp_eps(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                              const uint8_t *d_levels, int32_t npoints, int32_t is_term, int32_t *d_counters,
                              uint32_t *d_erased_bits, const scldpc::Scratch &scratch, void *stream)
{
    using namespace scldpc;
    if (int rc = check_params(p)) return rc;
    if (int rc = flood_check_call(who, scratch, ntrials, !d_counters || !d_vn_adj || !d_levels)) return rc;
    const int n = n_of(p), ncn = nk_of(p);
    if (npoints < 1 || npoints > SCLDPC_EPS_MAX_POINTS)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 1 <= npoints <= %d (got npoints = %d)", who, SCLDPC_EPS_MAX_POINTS, npoints);
    if (ntrials <= 0) return SCLDPC_OK;
    if (!flood_limits_ok(p))
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: needs dc <= 15, dv <= 8, dc*n < 2^24", who);
    Args a{};
    int words;
    // packed 16-bit words for position-structured graphs only = the 2-byte adjacency; pos_cnt and pos_ss in pos_a, R and the
    // level counts in pos_b
    auto carve = [&](int w) {
        return flood_carve_roomy(p, {flood_cn_lds_words(w, ncn), false, 2 * p->L, ((nw_of(p) + 3) & ~3) + kBins, 256}, &a.lay);
    };
    const std::string nofit = std::string(who) + ": %d VN bits + %d scan bits do not fit 160 KiB of LDS";
    if (int rc = flood_choose_words(who, nofit.c_str(), p, ntrials, scratch, adj16 && (int64_t)p->dv * p->vns_pos <= 4096, carve,
                                    &words, &a.ws)) return rc;
    if (words == kWordsQueryDone) return SCLDPC_OK;
    if (const char *v = getenv("SCLDPC_DEBUG_EPS_QCAP")) {          // tests: forces the overflow re-scan at a small shape
        const int cap = atoi(v);
        if (cap > 0 && cap < a.lay.qcap) a.lay.qcap = cap;
    }
    a.dv = p->dv; a.L = p->L; a.cns_pos = p->cns_pos; a.n = n; a.ncn = ncn;
    a.cn_lim = is_term ? ncn : p->L * p->cns_pos;                   // BPT:944-948
    a.npoints = npoints; a.ntrials = ntrials;
    const std::string inexact = std::string(who) + ": reciprocal division inexact";
    if (int rc = flood_geo(inexact.c_str(), p, n > 4096 ? n : 4096, &a)) return rc;
    a.vn_adj = d_vn_adj; a.levels = d_levels; a.counters = d_counters; a.erased_out = d_erased_bits;
    a.lev_wide = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(d_levels) & 3) == 0;
    void (*kern)(const Args) = flood_pick(words, p->dv == 4, adj16, [](auto st, auto dv, auto a16) -> void (*)(const Args) {
        return full_bp_eps_kernel<decltype(dv)::value, decltype(a16)::value, decltype(st)>;
    });
    return flood_launch(kern, ntrials, kBlock, stream, a);
}

extern "C" int scldpc_full_bp_eps_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj,
                                         const uint8_t *d_levels, int32_t npoints, int32_t is_term, int32_t *d_counters,
                                         uint32_t *d_erased_bits, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_full_bp_eps("scldpc_full_bp_eps_device", p, ntrials, d_vn_adj, false, d_levels, npoints, is_term, d_counters,
                              d_erased_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

extern "C" int scldpc_full_bp_eps_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                               const uint8_t *d_levels, int32_t npoints, int32_t is_term, int32_t *d_counters,
                                               uint32_t *d_erased_bits, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_full_bp_eps("scldpc_full_bp_eps_device_adj16", p, ntrials, d_vn_adj16, true, d_levels, npoints, is_term,
                              d_counters, d_erased_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

// workspace of scldpc_full_bp_eps_device(_adj16) for ntrials trials
extern "C" int64_t scldpc_full_bp_eps_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16)
{
    uint64_t need = 0;
    const int rc = launch_full_bp_eps("scldpc_full_bp_eps_workspace_query", p, ntrials, nullptr, adj16 != 0, nullptr, 1, 1,
                                      nullptr, nullptr, scldpc::Scratch{nullptr, 0, &need}, nullptr);
    return rc ? (int64_t)rc : (int64_t)need;
}
