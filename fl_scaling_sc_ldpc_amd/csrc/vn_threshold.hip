// The exact erasure threshold of every VN and of every position under unlimited full BP (include/scldpc_vn_thresh.h) — gfx950
// kernel.
//
// VN j of a frame is erased at threshold t iff key[j] < t; S(t) is the maximal stopping set inside E(t) = {key < t} over the CNs
// below cn_lim, monotone in t, and tau(j) = min {t : j in S(t)}.  After the decode at t_hi, R = S(t_hi) and the CN words hold
// exactly R.  With m the largest key of R, S(t) = R for every t in (m, top]; at t = m the VNs of R with key m leave E, all of
// them together, and peeling on from the CN words as they stand leaves S(m): everything removed on the way has tau = m + 1.
// So the walk needs no rebuild of the CN words: it reveals the keys of R in descending order and peels after each.
//
// Per frame, one 1024-thread workgroup on flood_common.h, with frame_threshold_kernel's CN-word forms, rows and dv instances.
// The kernel is ONE loop of rounds; a round is the work below, one barrier, and the read of its three counters:
//   scan    every CN < cn_lim holding one VN releases it (the first round of the decode at t_hi, and after a queue overflow)
//   queue   the CNs the round before pushed release their VN
//   list    the candidates list[gi, ge) — one key — are removed from R where they still are in it
//   tie     every VN of R with key == top - 1 is removed, found by a scan of the keys (no list)
// A round's releases push the CNs they leave with one VN for the next round.  When a round pushes nothing the stamp's cascade
// is over ("settled"), the step is accounted, and the next piece of work is chosen:
//   stage 0   stamp 0: U = {key < t_hi}, the CN words by build_cn_words, rounds to the fixpoint R (frame_threshold_kernel's
//             stage 0).  Then tau = NONE goes out for every VN outside R, in one coalesced pass.
//   chunk     with top `hi`, cut = hi - width: the VNs of R with key >= cut go to an LDS list of (key, VN), reading the 32 keys
//             of only the words in which R has a bit; the list is sorted descending (bitonic, one entry per thread).  width is
//             sized from |R| and hi for half a list of candidates (keys are uniform in practice) and never reaches below t_lo.
//             Overflow: width halves and the scan repeats.  width == 1: every candidate has the key hi - 1: a tie round, no
//             list — which is what makes any keys (all equal, heavy ties) terminate.  An exhausted list moves hi to the cut.
//   step      the next run of equal keys m of the list is a list round with stamp m + 1; a candidate an earlier cascade
//             released is skipped by the release itself (its bit in R is clear), and a round that releases nothing is no step.
//   end       R empty, or hi <= t_lo: what is left is S(t_lo) and gets tau = t_lo.
// Every released VN stores its stamp to d_tau (one 4-byte store; each word of the row is written exactly once, by the NONE pass,
// a release, or the last pass), lowers its position's LDS word by atomicMin, and counts in the round's counter; a step's count
// goes to an LDS difference array at the first grid index with grid[k] >= stamp, whose prefix sums are the counts.
//
// Progress.  Every loop below is bounded: a queue or scan round either releases a VN (|R| falls) or pushes nothing (the stamp
// settles); a list round advances the list index; an exhausted or empty list lowers hi to cut < hi; an overflow halves width
// down to 1, where the tie round needs no list and lowers hi by one.  hi never rises, and the walk ends at hi <= t_lo or R = ∅.
//
// Uniformity.  Every decision is taken by all threads from values read after a barrier that no thread overwrites before the
// next barrier: the round counters rotate over three slots (thread 0 clears the next round's at the top of a round: that slot
// was last read two barriers ago), the list's length over two (cleared in front of the scan's first barrier), and the list is
// written only between a scan's barriers and by the sort, which ends on one.  R's words are never read for a decision.
// Waves wait for each other at __syncthreads() only.  Where the CN words live in the workspace (ST::kGlobal) the rounds order a
// word's global atomics by those barriers, exactly as frame_threshold_kernel's do.
#include "eps_stages.h"
#include "../../include/scldpc_vn_thresh.h"
#include <climits>

namespace {

using namespace scldpc_dev;

constexpr int kListCap = 512;       // candidates per chunk, 8 bytes each
constexpr int kGridWords = SCLDPC_VNT_MAX_POINTS;

// scal[]: S_PUSH [0, 3) and S_OVF [3, 6) as in eps_stages.h, then
enum { V_REL = 6, V_LCNT = 9, V_NER = 11, V_RCNT = 12 };
enum { K_SCAN = 0, K_QUEUE = 1, K_LIST = 2, K_TIE = 3 };

struct VArgs : Geo {            // Geo: vns_pos, magic_v, magic_c
    int dv, L, cns_pos, n, ncn, cn_lim, ntrials, key_wide, npoints, ccap;
    uint32_t t_lo, t_hi;
    Layout lay;                 // pos_a: the L position words (of 2 L); pos_b: grid [256], differences [256], the list [2 kListCap]
    const void *vn_adj;
    const uint32_t *keys;       // [T][n]
    int32_t *rows;              // [T][SCLDPC_VNT_NCOLS]
    uint32_t *pos_thresh;       // [T][L]
    int32_t *counts;            // [T][npoints] (npoints > 0)
    uint32_t *tau;              // optional [T][n]
    uint32_t *ws;               // [T][ncn] CN words in global memory (ensembles beyond the LDS)
    uint32_t grid[SCLDPC_VNT_MAX_POINTS];
};

// Two 1024-thread workgroups per CU (8 waves per SIMD: at most 64 VGPRs) wherever the LDS admits them, as
// frame_threshold_kernel.  No spills: tests/test_walk_resources.py.
template <int DV, bool A16, class ST>
__global__ __launch_bounds__(kBlock, 8) void vn_threshold_kernel(const VArgs a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cn_state = ST::kGlobal ? a.ws + (size_t)blockIdx.x * a.ncn : lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;                                    // {key < t_hi}, then R
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *posw = lds + a.lay.pos_a;
    uint32_t *gridw = lds + a.lay.pos_b;
    int *diff = reinterpret_cast<int *>(gridw + kGridWords);
    unsigned long long *list = reinterpret_cast<unsigned long long *>(gridw + 2 * kGridWords);
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    const int tid = threadIdx.x, lane = tid & 63;
    const int trial = blockIdx.x;
    const int n = a.n, ncn = a.ncn, dv = (DV ? DV : a.dv), cn_lim = a.cn_lim, nw = a.lay.nw, qcap = a.lay.qcap, ccap = a.ccap;
    const int K = a.npoints;
    const char *adj = static_cast<const char *>(a.vn_adj) + (size_t)trial * n * dv * (A16 ? 2 : 4);
    const uint32_t *kr = a.keys + (size_t)trial * n;
    uint32_t *taur = a.tau ? a.tau + (size_t)trial * n : nullptr;
    const bool wide = a.key_wide != 0;
    const uint32_t t_lo = a.t_lo;

    if (tid < S_NSCAL) scal[tid] = 0;
    for (int i = tid; i < a.L; i += kBlock) posw[i] = SCLDPC_VNT_NONE;
    if (tid < kGridWords) {
        gridw[tid] = tid < K ? a.grid[tid] : 0u;
        diff[tid] = 0;
    }
    __syncthreads();                                                // (the zeroed scalars before any wave's atomics on them)
    // ---- stage 0 (frame_threshold_kernel's): U = {key < t_hi} and its size; the CN words cleared, then built over U
    {
        int uc = 0;
        for (int w = tid; w < nw; w += kBlock) {
            const uint32_t x = key_word(kr, w, n, wide, a.t_hi, [](int, uint32_t) {});
            U[w] = x;
            uc += __popc(x);
        }
        const uint32_t tot = wave_inclusive_scan((uint32_t)uc);
        if (lane == 63 && tot) atomicAdd(&scal[V_NER], (int)tot);
    }
    for (int c = tid; c < ST::words(ncn); c += kBlock) cn_state[c] = 0;
    __syncthreads();
    const int ner = uniform(scal[V_NER]);
    if (ner) {
        build_cn_words<ST, DV, A16, kBlock, false>(a, adj, dv, a.cns_pos, n, tid, U, cn_state,
                                                   [](const Vn &, const int32_t (&)[8], bool) {});
        __syncthreads();
    }

    // ---- the rounds.  All of the following are the same in every thread.
    int iter = 0, ncur = 0, rel = 0, scans = 0, rescans = 0, steps = 0;
    int r0 = 0, rsize = 0, last_rel = 0, lcnt = 0, li = 0, gi = 0, ge = 0, kptr = K;
    uint32_t stamp = 0, last_stamp = 0, hi = a.t_hi, cut = a.t_hi, width = 0;
    bool scan = ner != 0, stage0 = true;
    for (;;) {
        int kind = scan ? K_SCAN : K_QUEUE;
        if (!scan && ncur == 0) {
            // ---- settled: the cascade of `stamp` is over
            if (stage0) {
                stage0 = false;
                int rc = 0;
                for (int w = tid; w < nw; w += kBlock) rc += __popc(U[w]);
                const uint32_t tot = wave_inclusive_scan((uint32_t)rc);
                if (lane == 63 && tot) atomicAdd(&scal[V_RCNT], (int)tot);
                if (taur)                                           // the VNs the decode at t_hi recovers, or that it never lost
                    for (int j = tid; j < n; j += kBlock)
                        if (!((U[j >> 5] >> (j & 31)) & 1u)) taur[j] = SCLDPC_VNT_NONE;
                __syncthreads();
                r0 = rsize = uniform(scal[V_RCNT]);                 // (written once: nothing overwrites it)
            } else if (rel) {
                steps++;
                last_rel = rel;
                last_stamp = stamp;
                rsize -= rel;
                if (tid == 0) {                                     // the stamps descend: the first grid index at or above moves down
                    while (kptr > 0 && gridw[kptr - 1] >= stamp) kptr--;
                    if (kptr < K) diff[kptr] += rel;
                }
                rel = 0;
            }
            // ---- the next piece of work
            bool done = false;
            for (;;) {
                if (rsize == 0) { done = true; break; }
                if (li < lcnt) {                                    // the next run of one key in the sorted list
                    const uint32_t m = (uint32_t)(list[li] >> 32);
                    gi = li;
                    ge = li + 1;
                    while (ge < lcnt && (uint32_t)(list[ge] >> 32) == m) ge++;
                    li = ge;
                    stamp = m + 1u;
                    kind = K_LIST;
                    break;
                }
                hi = cut;                                           // every key of R is below the cut now (the first time: t_hi)
                if (hi <= t_lo) { done = true; break; }
                {
                    const uint32_t target = ccap > 1 ? (uint32_t)ccap / 2u : 1u;
                    const unsigned long long wd = (unsigned long long)hi * target / (uint32_t)rsize;
                    width = wd < 1ull ? 1u : wd > (unsigned long long)(hi - t_lo) ? hi - t_lo : (uint32_t)wd;
                }
                int cnt = 0;
                for (;;) {                                          // (ends: width halves down to 1, which needs no list)
                    cut = hi - width;
                    scans++;
                    if (width == 1u) break;
                    const int slot = V_LCNT + (scans & 1);
                    if (tid == 0) scal[slot] = 0;
                    __syncthreads();
                    for (int w = tid; w < nw; w += kBlock) {
                        const uint32_t x = U[w];
                        if (x)
                            key_word(kr, w, n, wide, 0u, [&](int b, uint32_t k) {
                                if (((x >> b) & 1u) && k >= cut) {
                                    const int idx = atomicAdd(&scal[slot], 1);
                                    if (idx < ccap) list[idx] = ((unsigned long long)k << 32) | (uint32_t)(w * 32 + b);
                                }
                            });
                    }
                    __syncthreads();
                    cnt = uniform(scal[slot]);
                    if (cnt <= ccap) break;
                    width = width / 2u;                             // (cnt > ccap >= 1 and width >= 2 here)
                    rescans++;
                }
                if (width == 1u) {                                  // one key, hi - 1: no list
                    lcnt = li = 0;
                    stamp = hi;
                    kind = K_TIE;
                    break;
                }
                lcnt = cnt;
                li = 0;
                if (cnt > 1) {                                      // bitonic sort, descending, over the next power of two
                    int P = 2;
                    while (P < cnt) P <<= 1;
                    if (tid >= cnt && tid < P) list[tid] = 0ull;
                    __syncthreads();
                    for (int k = 2; k <= P; k <<= 1)
                        for (int j = k >> 1; j > 0; j >>= 1) {
                            const int o = tid ^ j;
                            if (tid < P && o > tid) {
                                const unsigned long long x = list[tid], y = list[o];
                                if ((tid & k) == 0 ? x < y : x > y) { list[tid] = y; list[o] = x; }
                            }
                            __syncthreads();
                        }
                }
                // (an empty chunk: the loop lowers hi to the cut and scans the next one)
            }
            if (done) break;
        }

        // ---- one round
        const int g = iter % 3, gn = (iter + 1) % 3;
        uint32_t *qc = q[iter & 1], *qn = q[(iter + 1) & 1];
        if (tid == 0) { scal[S_PUSH + gn] = 0; scal[S_OVF + gn] = 0; scal[V_REL + gn] = 0; }
        auto drop = [&](int j) {                                    // VN j leaves R, if it still is in it
            const Vn v = make_vn(a, j);
            int32_t cc[8];
            load_adj<DV, A16>(adj, dv, j, v.pos, a.cns_pos, cc);
            const uint32_t bit = 1u << (j & 31);
            if (!(atomicAnd(&U[j >> 5], ~bit) & bit)) return;
            uint32_t o[8];
            for (int i = 0; i < dv; i++) o[i] = ST::remove_cnt(cn_state, cc[i], v, i, a.vns_pos);
            for (int i = 0; i < dv; i++) ST::remove_fold(cn_state, cc[i], v, i, a.vns_pos);
            for (int i = 0; i < dv; i++) {
                if (o[i] == 2u && cc[i] < cn_lim) {                 // transition to one VN: may fire
                    const int idx = atomicAdd(&scal[S_PUSH + g], 1);
                    if (idx < qcap) qn[idx] = (uint32_t)cc[i]; else scal[S_OVF + g] = 1;
                }
            }
            if (stamp) {
                atomicAdd(&scal[V_REL + g], 1);
                atomicMin(&posw[v.pos], stamp);
                if (taur) taur[j] = stamp;
            }
        };
        auto release = [&](int c) {
            const int j = ST::lone_vn(cn_state, c, a);
            if (j >= 0) drop(j);
        };
        if (kind == K_SCAN) {
            snapshot_frontier<kBlock>(fbits, 0, cn_lim, tid, [&](int c) { return c < cn_lim && ST::cnt(cn_state, c) == 1u; });
            __syncthreads();
            sweep_frontier<kBlock>(fbits, 0, cn_lim, tid, release);
        } else if (kind == K_QUEUE) {
            for (int k = tid; k < ncur; k += kBlock) release((int)qc[k]);
        } else if (kind == K_LIST) {
            if (gi + tid < ge) drop((int)(uint32_t)list[gi + tid]);
        } else {
            for (int w = tid; w < nw; w += kBlock) {
                const uint32_t x = U[w];                            // (only this thread clears bits of word w in a tie round)
                if (!x) continue;
                uint32_t m = x & ~key_word(kr, w, n, wide, cut, [](int, uint32_t) {});
                while (m) {
                    const int b = __ffs((int)m) - 1;
                    m &= m - 1;
                    drop(w * 32 + b);
                }
            }
        }
        __syncthreads();
        const bool ovf = uniform(scal[S_OVF + g]) != 0;
        ncur = ovf ? 0 : uniform(scal[S_PUSH + g]);
        rel += uniform(scal[V_REL + g]);
        iter++;
        scan = ovf;
        if (ovf) rescans++;
    }

    // ---- what is left is S(t_lo): tau = t_lo
    if (rsize) {
        for (int j = tid; j < n; j += kBlock)
            if ((U[j >> 5] >> (j & 31)) & 1u) {
                if (taur) taur[j] = t_lo;
                atomicMin(&posw[make_vn(a, j).pos], t_lo);
            }
        if (tid == 0 && K > 0) diff[0] += rsize;
    }
    __syncthreads();
    for (int i = tid; i < a.L; i += kBlock) a.pos_thresh[(size_t)trial * a.L + i] = posw[i];
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < K; k++) {
            acc += diff[k];
            a.counts[(size_t)trial * K + k] = acc;
        }
        const int status = r0 == 0 ? 1 : rsize ? 2 : 0;
        int32_t *o = a.rows + (size_t)trial * SCLDPC_VNT_NCOLS;
        o[0] = status == 0 ? (int32_t)last_stamp : status == 2 ? (int32_t)t_lo : -1;
        o[1] = status;
        o[2] = r0;
        o[3] = status == 0 ? last_rel : rsize;
        o[4] = steps;
        o[5] = scans;
        o[6] = rescans;
        o[7] = ner;
    }
}

}  // namespace

// The launch on walk_launch's front, with launch_frame_threshold's window check, form ladder and workspace rule; the LDS carve is
// this kernel's own (pos_a: the position words; pos_b: the grid, the count differences and the candidate list).  pos_a and pos_b
// are never smaller than launch_frame_threshold's, of which pos_a's second L words stay unused: from n = 47 000 on the shape rule
// is that kernel's and full_bp_eps's, so that a shape takes the same CN-word form in all three.
static int launch_vn_threshold(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                               const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t npoints,
                               const uint32_t *grid, int32_t *d_rows, uint32_t *d_pos_thresh, int32_t *d_counts, uint32_t *d_tau,
                               const scldpc::Scratch &scratch, void *stream)
{
    using scldpc::set_error;
    return scldpc::walk_launch<VArgs>(who, p, ntrials, !d_rows || !d_keys || !d_pos_thresh, d_vn_adj, adj16, scratch, stream,
                                      [](const scldpc_code_params *p) { return 2 * p->L; }, 2 * kGridWords + 2 * kListCap,
                                      [&](VArgs &a, int ncn) {
        if (int rc = scldpc::thresh_window(who, p, ncn, d_keys, t_lo, t_hi, is_term, a)) return rc;
        if (npoints < 0 || npoints > SCLDPC_VNT_MAX_POINTS)
            return set_error(SCLDPC_ERR_BAD_ARG, "%s: 0 <= npoints <= %d (got npoints = %d)", who, SCLDPC_VNT_MAX_POINTS, npoints);
        if (npoints > 0 && (!grid || (ntrials > 0 && !d_counts)))
            return set_error(SCLDPC_ERR_BAD_ARG, "%s: npoints = %d needs a grid and d_counts", who, npoints);
        for (int k = 0; k < npoints; k++) {
            if (grid[k] < t_lo || grid[k] > t_hi || (k > 0 && grid[k] <= grid[k - 1]))
                return set_error(SCLDPC_ERR_BAD_ARG, "%s: the grid must ascend strictly inside [t_lo, t_hi] (grid[%d] = %u)", who, k,
                                 grid[k]);
            a.grid[k] = grid[k];
        }
        a.npoints = npoints; a.rows = d_rows; a.pos_thresh = d_pos_thresh; a.counts = d_counts; a.tau = d_tau;
        a.ccap = kListCap;
        if (const char *v = getenv("SCLDPC_DEBUG_VNT_CCAP")) {      // tests: forces list overflows and tie rounds
            const int cap = atoi(v);
            if (cap > 0 && cap < a.ccap) a.ccap = cap;
        }
        return (int)SCLDPC_OK;
    }, [](auto st, auto dv, auto a16) -> void (*)(const VArgs) {
        return vn_threshold_kernel<decltype(dv)::value, decltype(a16)::value, decltype(st)>;
    });
}

extern "C" int scldpc_vn_threshold_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj,
                                          const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t npoints,
                                          const uint32_t *grid, int32_t *d_rows, uint32_t *d_pos_thresh, int32_t *d_counts,
                                          uint32_t *d_tau, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_vn_threshold("scldpc_vn_threshold_device", p, ntrials, d_vn_adj, false, d_keys, t_lo, t_hi, is_term, npoints, grid,
                               d_rows, d_pos_thresh, d_counts, d_tau, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

extern "C" int scldpc_vn_threshold_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term,
                                                int32_t npoints, const uint32_t *grid, int32_t *d_rows, uint32_t *d_pos_thresh,
                                                int32_t *d_counts, uint32_t *d_tau, void *d_workspace, uint64_t workspace_bytes,
                                                void *stream)
{
    return launch_vn_threshold("scldpc_vn_threshold_device_adj16", p, ntrials, d_vn_adj16, true, d_keys, t_lo, t_hi, is_term, npoints,
                               grid, d_rows, d_pos_thresh, d_counts, d_tau, scldpc::Scratch{d_workspace, workspace_bytes, nullptr},
                               stream);
}

// workspace of scldpc_vn_threshold_device(_adj16) for ntrials frames
extern "C" int64_t scldpc_vn_threshold_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16)
{
    uint64_t need = 0;
    const int rc = launch_vn_threshold("scldpc_vn_threshold_workspace_query", p, ntrials, nullptr, adj16 != 0, nullptr, 0u, 1u, 1, 0,
                                       nullptr, nullptr, nullptr, nullptr, nullptr, scldpc::Scratch{nullptr, 0, &need}, nullptr);
    return rc ? (int64_t)rc : (int64_t)need;
}
