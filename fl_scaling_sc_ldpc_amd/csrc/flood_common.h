// What the first-generation flooding decoders share around the CN-word policies of cn_words.h (full_bp.hip, sw_bp.hip,
// peel_sweep.hip, peel_fixpoint.h): on the device the channel load, the build of the CN words, the frontier snapshot and its
// sweep, the size-2 stopping-set test and full BP's result block; on the host the LDS carve and the front of a launch (argument
// and limit checks, the ladder Packed -> Wide -> WideG with its workspace, the prebuild switch, the launch itself).
// Every device function is inlined into its kernel.  The release lambdas and the round loops are NOT here: they differ in what
// they count and when they stop, and stay in their kernels (profiles/flood_common_static.txt has the generated code's figures).
// The two eps-grid decoders (peel_sweep_eps.hip, full_bp_eps.hip) do share theirs, which count the same things: eps_stages.h, on
// top of this header, has their walk over the stages as one kernel template and their launch front.
#pragma once
#include "common.h"
#include "kernel_util.h"
#include "cn_words.h"
#include <cstdlib>
#include <type_traits>

namespace scldpc_dev {

__device__ __forceinline__ Vn make_vn(const Geo &a, int j)
{
    Vn v;
    v.j = j; v.pos = (int)__umulhi((uint32_t)j, a.magic_v); v.t = j - v.pos * a.vns_pos;
    return v;
}

// U := this trial's channel words; returns the erasures in the words this thread loaded
template <int BLOCK>
__device__ __forceinline__ int load_channel(const uint32_t *ch, uint32_t *U, int nw, int n, int tid)
{
    int ne = 0;
    for (int w = tid; w < nw; w += BLOCK) {
        const uint32_t x = chan_tail(ch[w], w, nw, n);
        U[w] = x;
        ne += __popc(x);
    }
    return ne;
}

template <int BLOCK>
__device__ __forceinline__ void store_bits(uint32_t *out, int trial, const uint32_t *U, int nw, int tid)
{
    if (out)
        for (int w = tid; w < nw; w += BLOCK) out[(size_t)trial * nw + w] = U[w];
}

// ---- build: every erased VN (ALL: every VN, the unerased ones for the degree alone) adds itself to its dv CNs.  Four rows per
//      thread are loaded before the first is used, and loaded unconditionally, so that each wave instruction reads 1 KiB
//      contiguous (dv = 4) and four of them are in flight.  j_first = tid, or n to skip the build (words prebuilt).
//      per_vn(v, c, erased): what the caller counts besides, once per VN that takes part.
template <class ST, int DV, bool A16, int BLOCK, bool ALL, class PerVn>
__device__ __forceinline__ void build_cn_words(const Geo &a, const char *adj, int dv, int cns_pos, int n, int j_first,
                                               const uint32_t *U, uint32_t *cn_state, PerVn &&per_vn)
{
    for (int j0 = j_first; j0 < n; j0 += 4 * BLOCK) {
        int32_t c[4][8];
        bool er[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u * BLOCK;
            er[u] = false;
            if (j < n) {
                load_adj<DV, A16>(adj, dv, j, (int)__umulhi((uint32_t)j, a.magic_v), cns_pos, c[u]);
                er[u] = (U[j >> 5] >> (j & 31)) & 1u;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u * BLOCK;
            if (j < n && (ALL || er[u])) {
                const Vn v = make_vn(a, j);
                per_vn(v, c[u], er[u]);
                for (int i = 0; i < dv; i++) ST::add(cn_state, c[u][i], v, i, a.vns_pos, er[u], ALL);
            }
        }
    }
}

// ---- frontier: a scan round first takes a snapshot of the CNs that fire into fbits, so that its own releases cannot promote
//      CNs into it, and after the caller's barrier sweeps the snapshot.
// fires(c): does CN c fire?  Called by every thread of every 64-CN slice that meets [c0, c1), also for c outside the range (the
// answer must be false there), in wave-uniform control flow; it may count.  (sw_bp_kernel and peel_sweep_kernel, which writes a
// second bitmap, keep this loop as their own copy: with the helper they ran 0.6 % and 0.3 % slower, profiles/flood_common_ab.txt.)
template <int BLOCK, class Fires>
__device__ __forceinline__ void snapshot_frontier(uint32_t *fbits, int c0, int c1, int tid, Fires &&fires)
{
    const int lane = tid & 63;
    for (int base = c0 & ~63; base < c1; base += BLOCK) {
        const int c = base + tid;
        const unsigned long long m = __ballot(fires(c));
        if (c - lane < c1) {                                        // this wave's 64-CN slice starts inside the range
            if (lane == 0) fbits[c >> 5] = (uint32_t)m;
            if (lane == 32) fbits[c >> 5] = (uint32_t)(m >> 32);
        }
    }
}

template <int BLOCK, class Release>
__device__ __forceinline__ void sweep_frontier(const uint32_t *fbits, int c0, int c1, int tid, Release &&release)
{
    for (int base = c0 & ~63; base < c1; base += BLOCK) {
        const int c = base + tid;
        if (c < c1 && ((fbits[c >> 5] >> (c & 31)) & 1u)) release(c);
    }
}

// ---- size-2 stopping sets (BPF:1067-1133, BPW:850-908): an erased VN belongs to one iff every one of its CNs has cnt == 2 and
//      names the same partner, in the VN's own position
template <class ST>
__device__ __forceinline__ bool in_size2_set(const Geo &a, const uint32_t *cn_state, const Vn &v, const int32_t (&cc)[8], int dv)
{
    int partner = -1;
    for (int i = 0; i < dv; i++) {
        const int b = ST::partner(cn_state, cc[i], v, i, a);
        if (b < 0 || (i > 0 && b != partner)) return false;
        partner = b;
    }
    return (int)__umulhi((uint32_t)partner, a.magic_v) == v.pos;
}

// every VN still erased in U: per_vn(v), and pos_ss[its position]++ if it belongs to a size-2 stopping set
template <class ST, int DV, bool A16, int BLOCK, class PerVn>
__device__ __forceinline__ void count_size2_sets(const Geo &a, const char *adj, int dv, int cns_pos, const uint32_t *cn_state,
                                                 const uint32_t *U, int nw, int tid, int *pos_ss, PerVn &&per_vn)
{
    for (int w = tid; w < nw; w += BLOCK) {
        uint32_t x = U[w];
        while (x) {
            const int b = __ffs((int)x) - 1;
            x &= x - 1;
            const Vn v = make_vn(a, w * 32 + b);
            per_vn(v);
            int32_t cc[8];
            load_adj<DV, A16>(adj, dv, v.j, v.pos, cns_pos, cc);
            if (in_size2_set<ST>(a, cn_state, v, cc, dv)) atomicAdd(&pos_ss[v.pos], 1);
        }
    }
}

// ---- full BP's result (one thread): blocks in error, the expurgated counts, the eight counters
__device__ __forceinline__ void write_full_bp_counters(int32_t *o, const int *pos_cnt, const int *pos_ss, int L, int ne,
                                                       int iterations, int status, int nch)
{
    int be = 0, ee = 0, bee = 0;
    for (int pos = 0; pos < L; pos++) {
        if (pos_cnt[pos] > 0) be++;
        const int e = pos_cnt[pos] - pos_ss[pos];
        if (e > 0 && bee == 0) { ee = e; bee = 1; }                 // only the FIRST such position (BPF:1126-1132)
    }
    o[SCLDPC_C_NUM_ERASURES] = ne;
    o[SCLDPC_C_NUM_BLOCKS_ERR] = be;
    o[SCLDPC_C_NUM_ERASURES_EXP] = ee;
    o[SCLDPC_C_NUM_BLOCKS_ERR_EXP] = bee;
    o[SCLDPC_C_NUM_ERASURES_P1] = 0;
    o[SCLDPC_C_ITERATIONS] = iterations;
    o[SCLDPC_C_STATUS] = status;
    o[SCLDPC_C_CHANNEL_ERASURES] = nch;
}

}  // namespace scldpc_dev

namespace scldpc {

constexpr int kFloodScalars = 16;                                   // the S_* counters of each kernel
constexpr int kHalfLdsBytes = kMaxLdsBytes / 2 - 1024;              // what a workgroup may take when two share the CU

enum FloodWords { kWordsPacked = 0, kWordsWide = 1, kWordsGlobal = 2, kWordsQueryDone = -1 };

struct FloodLayout {            // offsets in 32-bit words into dynamic LDS
    int cn_state, U, fbits, frozen, pos_a, pos_b, scal, q0, q1, total;
    int qcap, nw;
};

struct FloodRegions {           // what a kernel keeps in LDS besides U, fbits, the scalars and the two queues
    int cn_words;               // CN words (0: they live in the workspace)
    bool frozen;                // a second bitmap the size of fbits
    int pos_a, pos_b;           // two per-position arrays, in words
    int min_qcap;               // fewer queue entries than this: does not fit
};

inline int flood_cn_lds_words(int words, int nk)
{
    return words == kWordsPacked ? scldpc_dev::Packed::lds_words(nk) : words == kWordsWide ? scldpc_dev::Wide::lds_words(nk)
                                                                                           : scldpc_dev::WideG::lds_words(nk);
}

// LDS carve, every region rounded to 16 bytes; the queues take what budget_bytes leaves, 8192 entries each at the most.
// 0, or -1 if the queues would be shorter than r.min_qcap.
inline int flood_carve(const scldpc_code_params *p, const FloodRegions &r, int budget_bytes, FloodLayout *lay)
{
    const int nk = nk_of(p);
    int off = 0;
    auto take = [&](int words) { int o = off; off += (words + 3) & ~3; return o; };   // keep 16-B alignment
    lay->nw = nw_of(p);
    lay->cn_state = take(r.cn_words);
    lay->U = take(lay->nw);
    lay->fbits = take(((nk + 63) / 64) * 2);
    lay->frozen = take(r.frozen ? ((nk + 63) / 64) * 2 : 0);
    lay->pos_a = take(r.pos_a);
    lay->pos_b = take(r.pos_b);
    lay->scal = take(kFloodScalars);
    int qcap = ((budget_bytes / 4 - off) / 2) & ~3;
    if (qcap > 8192) qcap = 8192;
    if (qcap < r.min_qcap) return -1;
    lay->qcap = qcap;
    lay->q0 = take(qcap);
    lay->q1 = take(qcap);
    lay->total = off;
    return 0;
}

// Two workgroups per CU (half the LDS each) whenever queues of at least 1024 entries still fit: the kernels wait on LDS / L2
// round trips most of the time and a second trial on the CU hides them.  Otherwise the whole LDS.
inline bool flood_carve_roomy(const scldpc_code_params *p, const FloodRegions &r, FloodLayout *lay)
{
    if (flood_carve(p, r, kHalfLdsBytes, lay) == 0 && lay->qcap >= 1024) return true;
    return flood_carve(p, r, kMaxLdsBytes, lay) == 0;
}

// ---- the front of a launch.  `who` is the entry point's name as the messages give it.
// after check_params: clears the query's answer; a negative ntrials or a null buffer of a real launch is an error
inline int flood_check_call(const char *who, const Scratch &scratch, int32_t ntrials, bool null_buffer)
{
    if (scratch.query) *scratch.query = 0;
    if (!scratch.query && (ntrials < 0 || (ntrials > 0 && null_buffer)))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer or negative ntrials", who);
    return SCLDPC_OK;
}

// what the CN words can hold: cnt and deg in four bits each, Σ ids in 24
inline bool flood_limits_ok(const scldpc_code_params *p)
{
    return p->dc <= 15 && p->dv <= 8 && (int64_t)p->dc * n_of(p) < (1ll << scldpc_dev::kDegShift);
}

// The ladder: 16-bit words (can_pack), else 32-bit words in LDS, else 32-bit words in the caller's workspace.  carve(words) lays
// out the LDS for a rung and says whether it fits.  Sets *words; kWordsQueryDone: scratch.query has its answer and the caller
// returns.  nofit_fmt takes (n, nk).
template <class Carve>
inline int flood_choose_words(const char *who, const char *nofit_fmt, const scldpc_code_params *p, int32_t ntrials,
                              const Scratch &scratch, bool can_pack, Carve &&carve, int *words, uint32_t **ws)
{
    const int nk = nk_of(p);
    *words = kWordsQueryDone;
    int w = can_pack && carve(kWordsPacked) ? kWordsPacked : kWordsWide;
    if (w == kWordsWide && !carve(kWordsWide)) {
        // CN words to a global workspace; the VN bitmap, scan bitmap and queues must still fit the LDS
        if (!carve(kWordsGlobal)) return set_error(SCLDPC_ERR_TOO_LARGE, nofit_fmt, n_of(p), nk);
        w = kWordsGlobal;
        const size_t need = (size_t)ntrials * nk * sizeof(uint32_t);
        if (scratch.query) { *scratch.query = need; return SCLDPC_OK; }
        void *buf = nullptr;
        if (int rc = take_scratch(who, scratch, need, &buf)) return rc;
        *ws = static_cast<uint32_t *>(buf);
    }
    if (!scratch.query) *words = w;
    return SCLDPC_OK;
}

// x / vns_pos for x < v_limit and c / cns_pos for c < nk by one multiply each
inline int flood_geo(const char *inexact_msg, const scldpc_code_params *p, int64_t v_limit, scldpc_dev::Geo *g)
{
    g->vns_pos = p->vns_pos;
    if (!magic_of(p->vns_pos, v_limit, &g->magic_v) || !magic_of(p->cns_pos, nk_of(p), &g->magic_c))
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s", inexact_msg);
    return SCLDPC_OK;
}

// the kernel instance of a rung × (dv == 4 or generic) × adjacency width: inst(ST{}, DV, A16) names it, with DV an
// std::integral_constant<int, 4 or 0> and A16 an std::bool_constant
template <class Inst>
inline auto flood_pick(int words, bool dv4, bool adj16, Inst &&inst)
{
    auto form = [&](auto st) {
        using I4 = std::integral_constant<int, 4>;
        using I0 = std::integral_constant<int, 0>;
        return dv4 ? (adj16 ? inst(st, I4{}, std::true_type{}) : inst(st, I4{}, std::false_type{}))
                   : (adj16 ? inst(st, I0{}, std::true_type{}) : inst(st, I0{}, std::false_type{}));
    };
    return words == kWordsPacked ? form(scldpc_dev::Packed{}) : words == kWordsWide ? form(scldpc_dev::Wide{}) : form(scldpc_dev::WideG{});
}

// the workspace's CN words through an LDS ring (cn_build.hip) instead of one global atomic per edge; `env` (A/B, tests) = 0
// leaves the build to the kernel.  1 = built.
inline int flood_prebuild(const char *env, const scldpc_code_params *p, int ntrials, const void *d_vn_adj16,
                          const uint32_t *d_chan_bits, uint32_t *ws, bool deg, void *stream)
{
    bool pre = true;
    if (const char *v = getenv(env)) pre = atoi(v) != 0;
    return pre && cn_build_launch(p, ntrials, static_cast<const uint16_t *>(d_vn_adj16), d_chan_bits, ws, deg, stream) ? 1 : 0;
}

template <class Args>
inline int flood_launch(void (*kern)(const Args), int ntrials, int block, void *stream, const Args &a)
{
    if (int rc = allow_max_lds(reinterpret_cast<const void *>(kern))) return rc;
    hipLaunchKernelGGL(kern, dim3(ntrials), dim3(block), 4u * (size_t)a.lay.total, static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

}  // namespace scldpc
