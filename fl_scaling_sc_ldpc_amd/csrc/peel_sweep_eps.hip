// Sweep peeling of one sampled code at every point of a descending eps grid, in one launch (include/scldpc_eps.h) — gfx950 kernel.
//
// peel_sweep.hip's trial with sweep_start = 0: every CN < total_size that holds one VN fires, at the outset or after a
// transition, so the residual is the maximal stopping set inside the erased set E (no CN of the residual's graph below
// total_size holds exactly one of its VNs, and peeling never removes a VN of a stopping set).  Maximal stopping sets are
// monotone in E, and that of E' ⊆ E lies inside the residual R of E: residual(E') = residual(R ∩ E').  The erased sets of a
// descending grid are nested, so stage k peels U = R_{k-1} ∩ {lev > k} instead of {lev > k}: at the points below the threshold
// R_{k-1} is empty or small, and the stage costs its own rebuild and a scan.  (With sweep_start > 0 a CN below it fires only on
// a TRANSITION to one VN, which depends on the outset: the identity is false there and the entry takes no sweep_start.)
//
// Per trial, one 1024-thread workgroup, built on flood_common.h the way peel_sweep_kernel is (the same CN-word forms, rows and
// dv instances):
//   levels   one pass over the trial's level bytes: U = {lev >= 1}, and the K + 1 counts of the levels — lev == 0 and lev == K
//            (most VNs: known at every point or erased at every point) are counted in registers, the levels between by LDS
//            atomics — whose suffix sums are the #erased of every point.
//   stage k  k >= 1: U = R ∩ {lev > k}, reading the 32 level bytes of every word in which R has a bit (words without one, all
//            of them once a trial has decoded, cost nothing; chosen by measurement over one byte load per bit of R, the twin
//            under SCLDPC_EPS_WALK_BITS: equal on terminated chains, 1.5 % faster where every trial carries a large residual,
//            profiles/eps_stage_mask_ab.txt); zero the CN words and build them over U — stage 0 with build_cn_words'
//            streaming loop, later stages from U's set bits; peel to the fixpoint with peel_sweep_kernel's rounds (a scan of
//            every CN < total_size holding one VN, then queue rounds, a re-scan after a queue overflow; no `frozen` bitmap:
//            nothing is barred from firing — so a re-scan finds exactly the CNs the lost queue held, the number of rounds
//            does not depend on the queue length, and the re-scans are counted on their own in out[6]); R := U; the lost / component / expurgation pass of peel_sweep_kernel unchanged
//            (it rebuilds the CN words over the lost VNs and overwrites U, hence R); out[k][trial].
//   Once R is empty every later point's row is zeros with its #erased, and the loop ends.
// R and the level counts live where FloodLayout has pos_b (the `frozen` region is sized by the CNs, not the VNs).
#include "flood_common.h"
#include "../../include/scldpc_eps.h"
#include <string>

namespace {

using namespace scldpc_dev;

constexpr int kBlock = 1024;
constexpr int kBins = SCLDPC_EPS_MAX_POINTS + 4;        // level counts [0, K], rounded to 16 bytes
enum { S_PUSH = 0, S_OVF = 3, S_LOST = 10, S_LOST_EXP = 11, S_RCNT = 12, S_NSCAL = 16 };

using Layout = scldpc::FloodLayout;      // pos_a = pos_flag; pos_b = R (nw words) + the level counts (kBins words)

struct Args : Geo {             // Geo: vns_pos, magic_v, magic_c
    int dv, L, cns_pos, n, ncn, total_size, lost_lo, lost_hi, npoints, ntrials, lev_wide;
    Layout lay;
    const void *vn_adj;
    const uint8_t *levels;      // [T][n]
    int32_t *out;               // [K][T][8]: lost, lost_exp, blocks_failed_exp, 0, 0, rounds and re-scans of the stage, #erased at the point
    uint32_t *lost_out;         // optional [K][T][nw]
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
// admits them.  peel_sweep_kernel stays below 64 VGPRs unasked; with the stages in a loop the scheduler, left to the 128 VGPRs
// that one workgroup per CU allows, takes up to 118, so the bound is stated.  No spills: `make resources`, DESIGN.md.
template <int DV, bool A16, class ST>
__global__ __launch_bounds__(kBlock, 8) __attribute__((amdgpu_num_sgpr(72))) void peel_sweep_eps_kernel(const Args a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cn_state = ST::kGlobal ? a.ws + (size_t)blockIdx.x * a.ncn : lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *R = lds + a.lay.pos_b;
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *pos_flag = reinterpret_cast<int *>(lds + a.lay.pos_a);
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    int tid = threadIdx.x, lane = tid & 63;
    const int trial = blockIdx.x;
    const int n = a.n, ncn = a.ncn, dv = (DV ? DV : a.dv), cn_lim = a.total_size, nw = a.lay.nw, qcap = a.lay.qcap;
    const int K = a.npoints;
    int *bins = reinterpret_cast<int *>(R + ((nw + 3) & ~3));       // [K + 1]; after the suffix sums bins[k + 1] = #erased at point k
    const char *adj = static_cast<const char *>(a.vn_adj) + (size_t)trial * n * dv * (A16 ? 2 : 4);
    const uint8_t *lv = a.levels + (size_t)trial * n;
    const bool wide = a.lev_wide != 0;
    auto pos_of = [&](int j) { return (int)__umulhi((uint32_t)j, a.magic_v); };

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

    auto is_lost = [&](int j, int32_t (&cc)[8]) {
        load_adj<DV, A16>(adj, dv, j, pos_of(j), a.cns_pos, cc);
        bool in_range = false, all_inside = true;
        for (int i = 0; i < dv; i++) {
            in_range |= cc[i] >= a.lost_lo && cc[i] < a.lost_hi;    // PD:661-664
            all_inside &= cc[i] < cn_lim;                           // PD:665
        }
        return in_range && all_inside;
    };
    // what VN v's CNs say: -2 = some CN holds >= 3 lost VNs or two different partners show up; -1 = no partner; else the partner
    auto neighbourhood = [&](const Vn &v, const int32_t (&cc)[8]) {
        int partner = -1;
        for (int i = 0; i < dv; i++) {
            const uint32_t k = ST::cnt(cn_state, cc[i]);
            if (k >= 3u) return -2;
            if (k == 2u) {
                const int b = ST::partner(cn_state, cc[i], v, i, a);
                if (partner >= 0 && b != partner) return -2;
                partner = b;
            }
        }
        return partner;
    };

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
        for (int i = tid; i < a.L; i += kBlock) pos_flag[i] = 0;
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
                // every CN < total_size holding one VN: at the outset all of them may fire (the sweep starts at CN 0, PD:656,
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

        // ---- R := the residual; lost set, components, expurgated statistics (peel_sweep_kernel's pass) ----
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
        for (int c = tid; c < ST::words(ncn); c += kBlock) cn_state[c] = 0;  // CN words over the lost VNs only, from here on
        __syncthreads();
        const int residual = scal[S_RCNT];
        if (residual == 0) break;                                   // the same answer in every thread; the tail below writes the rows
        for (int w = tid; w < nw; w += kBlock) {
            uint32_t x = U[w], keep = 0;
            while (x) {
                const int b = __ffs((int)x) - 1;
                x &= x - 1;
                int32_t cc[8];
                if (is_lost(w * 32 + b, cc)) {
                    keep |= 1u << b;
                    const Vn v = make_vn(a, w * 32 + b);
                    for (int i = 0; i < dv; i++) ST::add(cn_state, cc[i], v, i, a.vns_pos, true, false);
                }
            }
            U[w] = keep;                                            // U := lost
        }
        __syncthreads();
        int lost = 0, lost_exp = 0;
        for (int w = tid; w < nw; w += kBlock) {
            uint32_t x = U[w];
            while (x) {
                const int b = __ffs((int)x) - 1;
                x &= x - 1;
                const Vn va = make_vn(a, w * 32 + b);
                int32_t cc[8], cb[8];
                load_adj<DV, A16>(adj, dv, va.j, va.pos, a.cns_pos, cc);
                lost++;
                int pa = neighbourhood(va, cc);
                if (pa >= 0) {                                      // one partner: is {a, partner} closed?
                    const Vn vb = make_vn(a, pa);
                    load_adj<DV, A16>(adj, dv, vb.j, vb.pos, a.cns_pos, cb);
                    const int pb = neighbourhood(vb, cb);
                    if (pb != va.j) pa = -2;
                }
                if (pa == -2) {                                     // component of > 2 VNs
                    lost_exp++;
                    pos_flag[cc[0] / a.cns_pos] = 1;                // int(u.birthday / cns_per_pos), PD:160,687
                }
            }
        }
        {
            const uint32_t t1 = wave_inclusive_scan((uint32_t)lost), t2 = wave_inclusive_scan((uint32_t)lost_exp);
            if (lane == 63 && t1) atomicAdd(&scal[S_LOST], (int)t1);
            if (lane == 63 && t2) atomicAdd(&scal[S_LOST_EXP], (int)t2);
        }
        __syncthreads();
        const size_t row = (size_t)stage * a.ntrials + trial;
        if (a.lost_out)
            for (int w = tid; w < nw; w += kBlock) a.lost_out[row * nw + w] = U[w];
        if (tid == 0) {
            int blocks = 0;
            for (int pos = 0; pos < a.L; pos++) blocks += pos_flag[pos];
            int32_t *o = a.out + row * 8;
            o[0] = scal[S_LOST]; o[1] = scal[S_LOST_EXP]; o[2] = blocks; o[3] = 0; o[4] = 0; o[5] = iter; o[6] = rescans;
            o[7] = bins[stage + 1];
        }
        __syncthreads();                                            // the next stage clears scal and pos_flag, and rewrites U
    }

    // ---- the residual is empty from `stage` on (stage == K: every point has its row): rows of zeros with the #erased; the
    //      stage that found it empty keeps its rounds
    for (int k = stage + tid; k < K; k += kBlock) {
        int32_t *o = a.out + ((size_t)k * a.ntrials + trial) * 8;
        o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = k == stage ? iter : 0;
        o[6] = k == stage ? rescans : 0;
        o[7] = bins[k + 1];
    }
    if (a.lost_out)
        for (int k = stage; k < K; k++)
            for (int w = tid; w < nw; w += kBlock) a.lost_out[((size_t)k * a.ntrials + trial) * nw + w] = 0u;
}

}  // namespace

static int launch_peel_sweep_eps(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                                 const uint8_t *d_levels, int32_t npoints, int32_t total_size, int32_t lost_lo, int32_t lost_hi,
                                 int32_t *d_out, uint32_t *d_lost_bits, const scldpc::Scratch &scratch, void *stream)
{
    using namespace scldpc;
    if (int rc = check_params(p)) return rc;
    if (int rc = flood_check_call(who, scratch, ntrials, !d_out || !d_vn_adj || !d_levels)) return rc;
    const int n = n_of(p), ncn = nk_of(p);
    if (npoints < 1 || npoints > SCLDPC_EPS_MAX_POINTS)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 1 <= npoints <= %d (got npoints = %d)", who, SCLDPC_EPS_MAX_POINTS, npoints);
    if (total_size < 0 || total_size > ncn || lost_lo < 0 || lost_hi > ncn)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: CN ranges outside [0,%d]", who, ncn);
    if (ntrials <= 0) return SCLDPC_OK;
    if (!flood_limits_ok(p))
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: needs dc <= 15, dv <= 8, dc*n < 2^24", who);
    Args a{};
    int words;
    // packed 16-bit words for position-structured graphs only = the 2-byte adjacency; R and the level counts in pos_b
    auto carve = [&](int w) {
        return flood_carve_roomy(p, {flood_cn_lds_words(w, ncn), false, p->L + p->dv, ((nw_of(p) + 3) & ~3) + kBins, 256}, &a.lay);
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
    a.total_size = total_size; a.lost_lo = lost_lo; a.lost_hi = lost_hi; a.npoints = npoints; a.ntrials = ntrials;
    const std::string inexact = std::string(who) + ": reciprocal division inexact";
    if (int rc = flood_geo(inexact.c_str(), p, n > 4096 ? n : 4096, &a)) return rc;
    a.vn_adj = d_vn_adj; a.levels = d_levels; a.out = d_out; a.lost_out = d_lost_bits;
    a.lev_wide = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(d_levels) & 3) == 0;
    void (*kern)(const Args) = flood_pick(words, p->dv == 4, adj16, [](auto st, auto dv, auto a16) -> void (*)(const Args) {
        return peel_sweep_eps_kernel<decltype(dv)::value, decltype(a16)::value, decltype(st)>;
    });
    return flood_launch(kern, ntrials, kBlock, stream, a);
}

extern "C" int scldpc_peel_sweep_eps_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj,
                                            const uint8_t *d_levels, int32_t npoints, int32_t total_size, int32_t lost_lo,
                                            int32_t lost_hi, int32_t *d_out, uint32_t *d_lost_bits, void *d_workspace,
                                            uint64_t workspace_bytes, void *stream)
{
    return launch_peel_sweep_eps("scldpc_peel_sweep_eps_device", p, ntrials, d_vn_adj, false, d_levels, npoints, total_size,
                                 lost_lo, lost_hi, d_out, d_lost_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

extern "C" int scldpc_peel_sweep_eps_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                  const uint8_t *d_levels, int32_t npoints, int32_t total_size, int32_t lost_lo,
                                                  int32_t lost_hi, int32_t *d_out, uint32_t *d_lost_bits, void *d_workspace,
                                                  uint64_t workspace_bytes, void *stream)
{
    return launch_peel_sweep_eps("scldpc_peel_sweep_eps_device_adj16", p, ntrials, d_vn_adj16, true, d_levels, npoints,
                                 total_size, lost_lo, lost_hi, d_out, d_lost_bits,
                                 scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

// workspace of scldpc_peel_sweep_eps_device(_adj16) for ntrials trials
extern "C" int64_t scldpc_peel_sweep_eps_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16)
{
    uint64_t need = 0;
    const int rc = launch_peel_sweep_eps("scldpc_peel_sweep_eps_workspace_query", p, ntrials, nullptr, adj16 != 0, nullptr, 1, 0,
                                         0, 0, nullptr, nullptr, scldpc::Scratch{nullptr, 0, &need}, nullptr);
    return rc ? (int64_t)rc : (int64_t)need;
}
