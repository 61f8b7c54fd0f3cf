// Size spectrum of the connected components of a set of VNs, per trial (include/scldpc_ss.h): extract_stopping_sets
// (PD:1077-1095) on the device.  Members are joined through every CN they share; the kernel labels the components with a
// lock-free union-find in the style of ECL-CC (Jaiganesh & Burtscher, HPDC 2018) and adds their sizes to a histogram.
//
// One 1024-thread workgroup per trial; no word passes between workgroups except the final 64-bit integer atomics.  Phases,
// with a barrier between two of them and none inside data-dependent control flow:
//   load    member words -> LDS, popcount.  A trial with no member adds 1 to hist[0] and ends (at low eps: almost all).
//   init    parent[j] = j for the members, cn_rep[c] = none for every CN.
//   union   every member claims cn_rep[c] of its dv CNs with a CAS; where another member holds it, the two are united.
//   slots   the count of a component lives in the dead cn_rep room, at the first in-range CN of its root's row: that CN
//           belongs to this component alone (every member that touches it was united with its claimant).  Roots zero it.
//   count   every member adds 1 at its root's slot, one atomic per wave and root.
//   emit    roots add to 32-bit LDS bins, to an LDS [L][8] table (straight to global where the table does not fit) and to
//           the trial's scalars; after the last barrier the non-zero bins go out with one 64-bit atomic each.
//
// Union-find.  INVARIANT: parent[x] <= x at all times, with equality exactly at a root.  unite() hooks the LARGER root under
// the smaller with atomicCAS(&parent[a], a, b), b < a, and a root that has been hooked never becomes a root again; find()
// halves the path by pointing x at its grandparent g <= parent[x] < x, a store to a non-root that no CAS can be waiting on.
// So every path strictly decreases and every find() terminates; a failed CAS means another thread hooked that root, i.e.
// made progress.  The root of a component is its lowest-index member (d_pos_hist relies on this).  The loads of the find loop
// are relaxed atomic loads: they are not hoisted, and for state in the workspace they are served by the L2, where the atomics
// act, not by a line the CU's vector cache may still hold.
//
// State = parent[n] + cn_rep[ncn] int32: in LDS beside the member words and bins where that fits (form 1), else in the trial's
// slice of the caller's workspace (form 2; the (4,8), L = 50, M = 1000 benchmark shape: 4 * (50 000 + 26 500) B > 160 KiB).
#include "flood_common.h"
#include "../../include/scldpc_ss.h"

namespace {
using scldpc_dev::load_adj;

constexpr int kBlock = 1024;
constexpr int kStatusBytes = 256;       // the status word's slot in front of the slices (keeps them 256-byte aligned)
constexpr int kNone = -1;               // cn_rep: no member has claimed this CN
constexpr int kPosLdsWords = 8192;      // the [L][8] table stays in LDS up to this many words (L <= 1024)
enum { S_MEMBERS, S_COMPS, S_LARGEST, S_BIG, S_BAD, kScalars = 8 };

struct Layout {                         // offsets in 32-bit words into dynamic LDS
    int M, bins, pos, scal, parent, cn, total;
    int form, pos_lds;
    long long slice_words;              // form 2: words of one trial's slice of the workspace
};

struct Args {
    scldpc_dev::Geo geo;
    int dv, L, cns_pos, n, ncn, nw, nbins;
    Layout lay;
    const char *adj;
    const uint32_t *members;
    unsigned long long *hist, *pos_hist;
    int32_t *trial, *status, *state;
};

__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// path halving; parent[x] <= x keeps the walk strictly decreasing
__device__ __forceinline__ int find_root(int *parent, int x)
{
    int p = ld(&parent[x]);
    while (p != x) {
        const int g = ld(&parent[p]);
        if (g == p) return p;
        st(&parent[x], g);              // x is not a root and never will be: no CAS expects parent[x] == x any more
        x = g;
        p = ld(&parent[x]);
    }
    return x;
}

__device__ __forceinline__ void unite(int *parent, int a, int b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(&parent[a], a, b) == a) return;          // failed: somebody else hooked a, look again
    }
}

template <int DV, bool A16, bool LDS_STATE>
__global__ __launch_bounds__(kBlock) void ss_spectrum_kernel(const Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ss_lds[];
    uint32_t *M = ss_lds + a.lay.M, *bins = ss_lds + a.lay.bins, *pos_tab = ss_lds + a.lay.pos;
    int *scal = reinterpret_cast<int *>(ss_lds + a.lay.scal);
    int *parent, *cn;
    if constexpr (LDS_STATE) {
        parent = reinterpret_cast<int *>(ss_lds + a.lay.parent);
        cn = reinterpret_cast<int *>(ss_lds + a.lay.cn);
    } else {
        parent = a.state + (size_t)blockIdx.x * (size_t)a.lay.slice_words;
        cn = parent + a.n;
    }
    const int tid = threadIdx.x, lane = tid & 63, trial = blockIdx.x;
    const int dv = DV ? DV : a.dv, n = a.n, ncn = a.ncn, nw = a.nw;
    const bool pos_lds = a.pos_hist && a.lay.pos_lds;
    const char *adj = a.adj + (size_t)trial * n * dv * (A16 ? 2 : 4);

    // ---- load
    for (int b = tid; b < a.nbins; b += kBlock) bins[b] = 0;
    if (pos_lds)
        for (int i = tid; i < a.L * SCLDPC_SS_POS_SIZES; i += kBlock) pos_tab[i] = 0;
    if (tid < kScalars) scal[tid] = 0;
    __syncthreads();
    {
        const uint32_t *mw = a.members + (size_t)trial * nw;
        int mine = 0;
        for (int w = tid; w < nw; w += kBlock) {
            const uint32_t x = scldpc_dev::chan_tail(mw[w], w, nw, n);
            M[w] = x;
            mine += __popc(x);
        }
        mine = scldpc_dev::wave_sum(mine);
        if (lane == 0 && mine) atomicAdd(&scal[S_MEMBERS], mine);
    }
    __syncthreads();
    const int members = scal[S_MEMBERS];
    if (members == 0) {                                         // the same answer in every thread: no barrier is skipped by some
        if (tid == 0) {
            atomicAdd(&a.hist[0], 1ull);
            if (a.trial)
                *reinterpret_cast<int4 *>(a.trial + (size_t)trial * 4) = make_int4(0, 0, 0, 0);
        }
        return;
    }
    auto member = [&](int j) { return j < n && ((M[j >> 5] >> (j & 31)) & 1u); };
    auto row = [&](int j, int32_t (&c)[8]) {
        load_adj<DV, A16>(adj, dv, j, A16 ? (int)__umulhi((uint32_t)j, a.geo.magic_v) : 0, a.cns_pos, c);
    };
    auto in_range = [&](int c) { return (uint32_t)c < (uint32_t)ncn; };
    // the first in-range CN of VN j's row, or -1 (a member without one is a component of its own, of size 1)
    auto slot_of = [&](int j) {
        int32_t c[8];
        row(j, c);
        int s = -1;
        for (int i = dv - 1; i >= 0; i--)
            if (in_range(c[i])) s = c[i];
        return s;
    };

    // ---- init
    for (int j = tid; j < n; j += kBlock)
        if (member(j)) st(&parent[j], j);
    for (int c = tid; c < ncn; c += kBlock) st(&cn[c], kNone);
    __syncthreads();

    // ---- union
    bool bad = false;
    for (int j = tid; j < n; j += kBlock) {
        if (!member(j)) continue;
        int32_t c[8];
        row(j, c);
        for (int i = 0; i < dv; i++) {
            if (!in_range(c[i])) { bad = true; continue; }      // never an index
            const int old = atomicCAS(&cn[c[i]], kNone, j);
            if (old != kNone && old != j) unite(parent, j, old);
        }
    }
    if (bad) atomicOr(&scal[S_BAD], SCLDPC_SS_BAD_CN);
    __syncthreads();

    // ---- slots
    for (int j = tid; j < n; j += kBlock)
        if (member(j) && ld(&parent[j]) == j) {
            const int s = slot_of(j);
            if (s >= 0) st(&cn[s], 0);
        }
    __syncthreads();

    // ---- count: the lanes of a wave that found the same root add once
    for (int j0 = 0; j0 < n; j0 += kBlock) {
        const int j = j0 + tid;
        const bool act = member(j);
        const int r = act ? find_root(parent, j) : -1;
        unsigned long long todo = __ballot(act);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int r0 = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(r == r0);
            if (lane == leader) {
                const int s = slot_of(r0);
                if (s >= 0) atomicAdd(&cn[s], __popcll(same));
            }
            todo &= ~same;
        }
    }
    __syncthreads();

    // ---- emit
    for (int j = tid; j < n; j += kBlock)
        if (member(j) && ld(&parent[j]) == j) {
            const int slot = slot_of(j);
            const int s = slot >= 0 ? ld(&cn[slot]) : 1;
            atomicAdd(&bins[min(s, a.nbins - 1)], 1u);
            if (a.pos_hist) {
                const int at = (j / a.geo.vns_pos) * SCLDPC_SS_POS_SIZES + min(s, SCLDPC_SS_POS_SIZES) - 1;
                if (pos_lds) atomicAdd(&pos_tab[at], 1u);
                else atomicAdd(&a.pos_hist[at], 1ull);
            }
            atomicAdd(&scal[S_COMPS], 1);
            atomicMax(&scal[S_LARGEST], s);
            if (s > 2) atomicAdd(&scal[S_BIG], s);
        }
    __syncthreads();
    for (int b = tid; b < a.nbins; b += kBlock)
        if (const uint32_t v = bins[b]) atomicAdd(&a.hist[b], (unsigned long long)v);
    if (pos_lds)
        for (int i = tid; i < a.L * SCLDPC_SS_POS_SIZES; i += kBlock)
            if (const uint32_t v = pos_tab[i]) atomicAdd(&a.pos_hist[i], (unsigned long long)v);
    if (tid == 0) {
        if (a.trial)
            *reinterpret_cast<int4 *>(a.trial + (size_t)trial * 4) = make_int4(scal[S_COMPS], scal[S_LARGEST], members, scal[S_BIG]);
        if (scal[S_BAD]) atomicOr(a.status, scal[S_BAD]);
    }
}

bool force_workspace()
{
    const char *v = getenv("SCLDPC_DEBUG_SS_FORCE_WORKSPACE");
    return v && atoi(v) != 0;
}

// The LDS carve, every region rounded to 16 bytes: 0, or the error set.  The position table is laid out whether or not the
// call passes d_pos_hist, so that form and workspace size depend on the ensemble alone.
int carve(const char *who, const scldpc_code_params *p, Layout *lay)
{
    using namespace scldpc;
    if (int rc = check_params(p)) return rc;
    if (p->dv > 8) return set_error(SCLDPC_ERR_TOO_LARGE, "%s: dv <= 8 (got dv = %d)", who, p->dv);
    const int64_t n = n_of(p), ncn = nk_of(p);
    int64_t off = 0;
    auto take = [&](int64_t words) { const int64_t o = off; off += (words + 3) & ~(int64_t)3; return (int)o; };
    const int64_t pos_words = (int64_t)p->L * SCLDPC_SS_POS_SIZES;
    lay->pos_lds = pos_words <= kPosLdsWords;
    const int64_t fixed = nw_of(p) + SCLDPC_SS_MAX_BINS + (lay->pos_lds ? pos_words : 0) + kScalars + 16;
    if (4 * fixed > kMaxLdsBytes)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: the member words of %lld VNs per trial do not fit one CU's LDS beside the bins",
                         who, (long long)n);
    lay->M = take(nw_of(p));
    lay->bins = take(SCLDPC_SS_MAX_BINS);
    lay->pos = take(lay->pos_lds ? pos_words : 0);
    lay->scal = take(kScalars);
    lay->form = !force_workspace() && 4 * (off + n + ncn + 8) <= kMaxLdsBytes ? 1 : 2;
    lay->parent = lay->cn = 0;
    lay->slice_words = 0;
    if (lay->form == 1) {
        lay->parent = take(n);
        lay->cn = take(ncn);
    } else {
        lay->slice_words = (n + ncn + 63) & ~(int64_t)63;
    }
    lay->total = (int)off;
    return SCLDPC_OK;
}

template <bool LDS_STATE>
auto pick(bool dv4, bool adj16) -> void (*)(const Args)
{
    return dv4 ? (adj16 ? ss_spectrum_kernel<4, true, LDS_STATE> : ss_spectrum_kernel<4, false, LDS_STATE>)
               : (adj16 ? ss_spectrum_kernel<0, true, LDS_STATE> : ss_spectrum_kernel<0, false, LDS_STATE>);
}
}  // namespace

extern "C" int scldpc_ss_spectrum_form(const scldpc_code_params *p)
{
    Layout lay;
    if (int rc = carve("scldpc_ss_spectrum_form", p, &lay)) return rc;
    return lay.form;
}

extern "C" int64_t scldpc_ss_spectrum_workspace_bytes(const scldpc_code_params *p, int32_t ntrials)
{
    static const char *who = "scldpc_ss_spectrum_workspace_bytes";
    Layout lay;
    if (carve(who, p, &lay)) return -1;
    if (ntrials < 0) { scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: negative ntrials", who); return -1; }
    return kStatusBytes + 4 * (int64_t)ntrials * lay.slice_words;
}

extern "C" int scldpc_ss_spectrum_device(const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, int32_t adj_kind,
                                         const uint32_t *d_member_bits, int32_t nbins, int64_t *d_hist, int64_t *d_pos_hist,
                                         int32_t *d_trial, void *d_ws, int64_t ws_bytes, void *stream)
{
    using namespace scldpc;
    static const char *who = "scldpc_ss_spectrum_device";
    Args a;
    if (int rc = carve(who, p, &a.lay)) return rc;
    if (ntrials < 0) return set_error(SCLDPC_ERR_BAD_ARG, "%s: negative ntrials", who);
    if (nbins < 2 || nbins > SCLDPC_SS_MAX_BINS)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 2 <= nbins <= %d (got nbins = %d)", who, SCLDPC_SS_MAX_BINS, nbins);
    if (adj_kind != 0 && adj_kind != 1)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: adj_kind is 0 (int32 global CN ids) or 1 (uint16 position-local ids), got %d",
                         who, adj_kind);
    a.geo.vns_pos = p->vns_pos;
    a.geo.magic_v = a.geo.magic_c = 0;
    if (adj_kind == 1) {
        if ((int64_t)p->vns_pos * p->dv > 65535)
            return set_error(SCLDPC_ERR_TOO_LARGE, "%s: adj_kind 1 needs vns_pos * dv <= 65535 (got %lld)", who,
                             (long long)p->vns_pos * p->dv);
        if (int rc = flood_geo("scldpc_ss_spectrum_device: reciprocal division inexact", p, n_of(p), &a.geo)) return rc;
    }
    if (ntrials == 0) return SCLDPC_OK;
    if (!d_vn_adj || !d_member_bits || !d_hist || !d_ws) return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer", who);
    if (reinterpret_cast<uintptr_t>(d_ws) & 15) return set_error(SCLDPC_ERR_BAD_ARG, "%s: workspace not 16-byte aligned", who);
    const int64_t need = kStatusBytes + 4 * (int64_t)ntrials * a.lay.slice_words;
    if (ws_bytes < need)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)need);
    a.dv = p->dv; a.L = p->L; a.cns_pos = p->cns_pos; a.n = n_of(p); a.ncn = nk_of(p); a.nw = nw_of(p); a.nbins = nbins;
    a.adj = static_cast<const char *>(d_vn_adj);
    a.members = d_member_bits;
    a.hist = reinterpret_cast<unsigned long long *>(d_hist);
    a.pos_hist = reinterpret_cast<unsigned long long *>(d_pos_hist);
    a.trial = d_trial;
    a.status = static_cast<int32_t *>(d_ws);
    a.state = reinterpret_cast<int32_t *>(static_cast<char *>(d_ws) + kStatusBytes);
    void (*kern)(const Args) = a.lay.form == 1 ? pick<true>(p->dv == 4, adj_kind == 1) : pick<false>(p->dv == 4, adj_kind == 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = allow_max_lds(reinterpret_cast<const void *>(kern))) return rc;
    SCLDPC_HIP_CHECK(hipMemsetAsync(a.status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(kern, dim3(ntrials), dim3(kBlock), 4u * (size_t)a.lay.total, st, a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}
