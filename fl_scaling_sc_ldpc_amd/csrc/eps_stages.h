// One sampled code at every point of a descending eps grid, in one launch: the walk over the stages that peel_sweep_eps.hip and
// full_bp_eps.hip share, on the device and on the host.  Both decoders end a point on the maximal stopping set inside the
// erased set E over the CNs below a limit; maximal stopping sets are monotone in E, and that of E' ⊆ E lies inside the residual R
// of E: residual(E') = residual(R ∩ E').  The erased sets of a descending grid are nested, so stage k peels
// U = R_{k-1} ∩ {lev > k} instead of {lev > k}: at the points below the threshold R_{k-1} is empty or small, and the stage
// costs its own rebuild and a scan.
//
// Per trial, one 1024-thread workgroup, built on flood_common.h (the same CN-word forms, rows and dv instances as
// peel_sweep_kernel and full_bp_kernel):
//   levels   one pass over the trial's level bytes: U = {lev >= 1}, and the K + 1 counts of the levels — lev == 0 and lev == K
//            (most VNs: known at every point or erased at every point) are counted in registers, the levels between by LDS
//            atomics — whose suffix sums are the #erased of every point.
//   stage k  k >= 1: U = R ∩ {lev > k}, reading the 32 level bytes of every word in which R has a bit (words without one, all
//            of them once a trial has decoded, cost nothing; chosen by measurement over one byte load per bit of R, the twin
//            under SCLDPC_EPS_WALK_BITS: equal on terminated chains, 1.5 % faster where every trial carries a large residual,
//            profiles/eps_stage_mask_ab.txt); zero the CN words and build them over U — stage 0 with build_cn_words'
//            streaming loop, later stages from U's set bits; peel to the fixpoint (a scan of every CN < cn_lim holding one VN,
//            then queue rounds, a re-scan after a queue overflow; no `frozen` bitmap: nothing is barred from firing — so a
//            re-scan finds exactly the CNs the lost queue held, the number of rounds does not depend on the queue length, and
//            the re-scans are counted on their own); R := U; the End policy's end of the stage and its row of point k.
//   Once R is empty every later point's row is zeros with its #erased, and the loop ends.
// R and the level counts live where FloodLayout has pos_b (the `frozen` region is sized by the CNs, not the VNs); pos_a holds
// the End policy's per-position arrays.
//
// What an End policy supplies (peel_sweep_eps.hip, full_bp_eps.hip):
//   Args         the kernel's argument struct: Geo, then dv, L, cns_pos, n, ncn, npoints, ntrials, lev_wide, lay, vn_adj,
//                levels, ws and the optional bitmap output bits_out [K][T][nw] under these names, and the entry's own fields
//   cn_lim(a)    CNs below it may fire
//   kPosArrays   how many arrays of L words in pos_a are cleared at stage set-up
//   kRebuilds    the end of the stage rebuilds the CN words: they are zeroed after R := U
//   finish<ST, DV, A16>(...)   the end of a stage with a residual, up to its row of results
//   zero_row(...)              the row of a point at which the residual is empty
//   pos_words(p) the size of pos_a
// The phases stay in the kernel's body: as functions of their own, over a context struct, they spill VGPRs in a kernel held at
// the 64-VGPR bound.  Two things of an end of stage live in the body as well, because where they stand decides the generated code
// (profiles/eps_walk_static.txt, profiles/eps_walk_ab.txt): the pointer to the second position array, taken at the top, and the
// two adjacency rows finish may use.  As locals of finish the rows reach the kernel in front of its other arrays, the compiler
// then keeps other arrays in registers, and the generic-dv instances of the sweep decoder took 62-63 VGPRs and ran 1.2 to 3 %
// slower.
#pragma once
#include "flood_common.h"
#include "../../include/scldpc_eps.h"
#include "../../include/scldpc_thresh.h"
#include <string>

namespace scldpc_dev {

constexpr int kBlock = 1024;
constexpr int kBins = SCLDPC_EPS_MAX_POINTS + 4;        // level counts [0, K], rounded to 16 bytes
enum { S_PUSH = 0, S_OVF = 3, S_LOST = 10, S_LOST_EXP = 11, S_RCNT = 12, S_NSCAL = 16 };

using Layout = scldpc::FloodLayout;      // pos_a = End's position arrays; pos_b = R (nw words) + the level counts (kBins words)

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

// bits (key < t) of the 32 VNs of word w, none at or past n; wide: the row is 16-byte aligned and n % 4 == 0.
// per(b, key): called with every key of the word and its bit number.
template <class Per>
__device__ __forceinline__ uint32_t key_word(const uint32_t *kr, int w, int n, bool wide, uint32_t t, Per &&per)
{
    uint32_t x = 0;
    const int j0 = w * 32;
    if (wide) {
#pragma unroll 2
        for (int q = 0; q < 8; q++) {
            if (j0 + 4 * q >= n) break;                             // n % 4 == 0: a whole group or none
            const uint4 v = *reinterpret_cast<const uint4 *>(kr + j0 + 4 * q);
            const uint32_t k4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                per(4 * q + u, k4[u]);
                x |= (uint32_t)(k4[u] < t) << (4 * q + u);
            }
        }
    } else {
        for (int b = 0; b < 32 && j0 + b < n; b++) {
            const uint32_t k = kr[j0 + b];
            per(b, k);
            x |= (uint32_t)(k < t) << b;
        }
    }
    return x;
}

__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// Two 1024-thread workgroups per CU (8 waves per SIMD: at most 64 VGPRs, and 72 SGPRs as in full_bp.hip) wherever the LDS
// admits them.  peel_sweep_kernel stays below 64 VGPRs unasked; with the stages in a loop the scheduler, left to the 128 VGPRs
// that one workgroup per CU allows, takes up to 118, so the bound is stated.  No spills: tests/test_walk_resources.py.
template <int DV, bool A16, class ST, class End>
__global__ __launch_bounds__(kBlock, 8) __attribute__((amdgpu_num_sgpr(72))) void eps_walk_kernel(const typename End::Args a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cn_state = ST::kGlobal ? a.ws + (size_t)blockIdx.x * a.ncn : lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *R = lds + a.lay.pos_b;
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *pos = reinterpret_cast<int *>(lds + a.lay.pos_a);
    int *pos_2nd = pos + a.L;                                       // kPosArrays == 2: the second array
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    int tid = threadIdx.x, lane = tid & 63;
    const int trial = blockIdx.x;
    const int n = a.n, ncn = a.ncn, dv = (DV ? DV : a.dv), cn_lim = End::cn_lim(a), nw = a.lay.nw, qcap = a.lay.qcap;
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

    int stage = 0, iter = 0, rescans = 0;
    for (; stage < K; stage++) {
        // (tid made opaque per stage: what the phases derive from it is computed again in every stage instead of being
        // hoisted out of this loop and kept in registers across it, which cost a workgroup per CU: see DESIGN.md)
        asm volatile("" : "+v"(tid));
        lane = tid & 63;
        // ---- U of this stage, the CN words over it
        if (stage > 0)
            for (int w = tid; w < nw; w += kBlock) {
                const uint32_t r = R[w];
#ifdef SCLDPC_EPS_WALK_BITS                                             // the A/B twin (profiles/eps_stage_mask_ab.txt): one byte load per bit of R
                uint32_t x = 0;
                for (uint32_t m = r; m; m &= m - 1) {
                    const int b = __ffs((int)m) - 1;
                    x |= (uint32_t)(lv[w * 32 + b] > (uint32_t)stage) << b;
                }
                U[w] = x;
#else
                U[w] = r ? r & level_word(lv, w, n, wide, (uint32_t)stage, [](uint32_t) {}) : 0u;
#endif
            }
        for (int c = tid; c < ST::words(ncn); c += kBlock) cn_state[c] = 0;
        if (tid < S_NSCAL) scal[tid] = 0;
        for (int i = tid; i < End::kPosArrays * a.L; i += kBlock) pos[i] = 0;
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

        // ---- peeling to the fixpoint (peel_sweep_kernel's rounds; the order is irrelevant for the residual) ----
        int ncur = 0;
        bool scan = true;
        iter = 0;
        rescans = 0;
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
                    if (o[i] == 2u && cc[i] < cn_lim) {             // transition to one VN: may fire (PD:305-308)
                        const int idx = atomicAdd(&scal[S_PUSH + g], 1);
                        if (idx < qcap) qn[idx] = (uint32_t)cc[i]; else scal[S_OVF + g] = 1;
                    }
                }
            };
            if (scan) {
                // every CN < cn_lim holding one VN: at the outset all of them may fire (the sweep starts at CN 0, PD:656,
                // 273-277), and after a queue overflow those found got there by a transition
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
            if (ovf) { scan = true; rescans++; continue; }
            scan = false;
            if (ncur == 0) break;                                   // nothing queued: fixpoint
        }
        __syncthreads();

        // ---- R := the residual; the policy's end of the stage ----
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
        if (End::kRebuilds)
            for (int c = tid; c < ST::words(ncn); c += kBlock) cn_state[c] = 0;
        __syncthreads();
        const int residual = scal[S_RCNT];
        if (residual == 0) break;                                   // the same answer in every thread; the tail below writes the rows
        int32_t ca[8], cb[8];                                       // finish's adjacency rows: see the head of this file
        End::template finish<ST, DV, A16>(a, adj, dv, cn_lim, cn_state, U, pos, pos_2nd, scal, bins, nw, tid, lane, trial, stage,
                                          residual, iter, rescans, ca, cb);
        __syncthreads();                                            // the next stage clears scal and the position arrays, and rewrites U
    }

    // ---- the residual is empty from `stage` on (stage == K: every point has its row): rows of zeros with the #erased; the
    //      stage that found it empty keeps its rounds
    for (int k = stage + tid; k < K; k += kBlock)
        End::zero_row(a, (size_t)k * a.ntrials + trial, k == stage ? iter : 0, k == stage ? rescans : 0, bins[k + 1]);
    if (a.bits_out)
        for (int k = stage; k < K; k++)
            for (int w = tid; w < nw; w += kBlock) a.bits_out[((size_t)k * a.ntrials + trial) * nw + w] = 0u;
}

}  // namespace scldpc_dev

namespace scldpc {

// The front of every launch on one sampled code per frame (the two eps walks here, frame_threshold.hip, vn_threshold.hip), and
// the launch.  Args is the kernel's argument struct: Geo, then dv, L, cns_pos, n, ncn, ntrials, lay, vn_adj and ws under these
// names.  own(a, ncn) refuses what the entry refuses about its own arguments and sets the entry's own fields; pos_a(p) and
// max(the words of R and the level counts, pos_b_floor) size the two position regions, which with the 2-byte adjacency decide the
// CN-word form a shape takes; pick names the kernel instance as flood_pick asks.
template <class Args, class Own, class Pick>
inline int walk_launch(const char *who, const scldpc_code_params *p, int32_t ntrials, bool any_null, const void *d_vn_adj, bool adj16,
                       const Scratch &scratch, void *stream, int (*pos_a)(const scldpc_code_params *), int pos_b_floor, Own &&own,
                       Pick &&pick)
{
    using namespace scldpc_dev;
    if (int rc = check_params(p)) return rc;
    if (int rc = flood_check_call(who, scratch, ntrials, any_null || !d_vn_adj)) return rc;
    const int n = n_of(p), ncn = nk_of(p);
    Args a{};
    if (int rc = own(a, ncn)) return rc;
    if (ntrials <= 0) return SCLDPC_OK;
    if (!flood_limits_ok(p))
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: needs dc <= 15, dv <= 8, dc*n < 2^24", who);
    int words;
    // packed 16-bit words for position-structured graphs only = the 2-byte adjacency
    auto carve = [&](int w) {
        const int pos_b = ((nw_of(p) + 3) & ~3) + kBins;
        return flood_carve_roomy(p, {flood_cn_lds_words(w, ncn), false, pos_a(p), pos_b > pos_b_floor ? pos_b : pos_b_floor, 256}, &a.lay);
    };
    const std::string nofit = std::string(who) + ": %d VN bits + %d scan bits do not fit 160 KiB of LDS";
    if (int rc = flood_choose_words(who, nofit.c_str(), p, ntrials, scratch, adj16 && (int64_t)p->dv * p->vns_pos <= 4096, carve,
                                    &words, &a.ws)) return rc;
    if (words == kWordsQueryDone) return SCLDPC_OK;
    if (const char *v = getenv("SCLDPC_DEBUG_EPS_QCAP")) {          // tests: forces the overflow re-scan at a small shape
        const int cap = atoi(v);
        if (cap > 0 && cap < a.lay.qcap) a.lay.qcap = cap;
    }
    a.dv = p->dv; a.L = p->L; a.cns_pos = p->cns_pos; a.n = n; a.ncn = ncn; a.ntrials = ntrials; a.vn_adj = d_vn_adj;
    const std::string inexact = std::string(who) + ": reciprocal division inexact";
    if (int rc = flood_geo(inexact.c_str(), p, n > 4096 ? n : 4096, &a)) return rc;
    void (*kern)(const Args) = flood_pick(words, p->dv == 4, adj16, pick);
    return flood_launch(kern, ntrials, kBlock, stream, a);
}

// The eps walks' launch.  d_rows: the entry's result rows, for the null test only.  fill(a, ncn) sets the End policy's own
// fields of Args and refuses what the entry refuses about them.  R and the level counts in pos_b.
template <class End, class Fill>
inline int eps_walk_launch(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                           const uint8_t *d_levels, int32_t npoints, const void *d_rows, uint32_t *d_bits, const Scratch &scratch,
                           void *stream, Fill &&fill)
{
    using Args = typename End::Args;
    return walk_launch<Args>(who, p, ntrials, !d_rows || !d_levels, d_vn_adj, adj16, scratch, stream, &End::pos_words, 0,
                             [&](Args &a, int ncn) {
        if (npoints < 1 || npoints > SCLDPC_EPS_MAX_POINTS)
            return set_error(SCLDPC_ERR_BAD_ARG, "%s: 1 <= npoints <= %d (got npoints = %d)", who, SCLDPC_EPS_MAX_POINTS, npoints);
        a.npoints = npoints; a.levels = d_levels; a.bits_out = d_bits;
        a.lev_wide = (n_of(p) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_levels) & 3) == 0;
        return fill(a, ncn);
    }, [](auto st, auto dv, auto a16) -> void (*)(const Args) {
        return scldpc_dev::eps_walk_kernel<decltype(dv)::value, decltype(a16)::value, decltype(st), End>;
    });
}

// The window and the keys of both threshold launches (frame_threshold.hip, vn_threshold.hip): the check and the fields.
template <class Args>
inline int thresh_window(const char *who, const scldpc_code_params *p, int ncn, const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi,
                         int32_t is_term, Args &a)
{
    if (!(t_lo < t_hi && t_hi <= SCLDPC_THRESH_MAX))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 0 <= t_lo < t_hi <= %u (got t_lo = %u, t_hi = %u)", who, SCLDPC_THRESH_MAX, t_lo,
                         t_hi);
    a.cn_lim = is_term ? ncn : p->L * p->cns_pos;
    a.t_lo = t_lo; a.t_hi = t_hi; a.keys = d_keys;
    a.key_wide = (n_of(p) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_keys) & 15) == 0;
    return SCLDPC_OK;
}

}  // namespace scldpc
