// The exact erasure threshold of every frame under unlimited full BP (include/scldpc_thresh.h) — gfx950 kernel.
//
// VN j of a frame is erased at threshold t iff key[j] < t, so the erased sets E(t) are nested, and what unlimited flooding BP
// leaves of E(t) is S(t), the maximal stopping set inside E(t) over the CNs below cn_lim, monotone in t.  The
// frame's critical threshold T* = min {t : S(t) != ∅} is found by bisection on the integer t, every stage peeling inside the
// residual of the last non-empty one: S(t) = S(S(t') ∩ E(t)) for t <= t' (the identity eps_stages.h walks a grid with).
//
// Per frame, one 1024-thread workgroup on flood_common.h; the CN-word forms, rows, dv instances, the build, the peel rounds with
// two queues and the re-scan on overflow have eps_walk_kernel's structure (eps_stages.h), whose stage is a grid point where this
// one's is a threshold:
//   stage 0   U = {key < t_hi} from the frame's keys (16-byte loads), the CN words by build_cn_words' streaming loop, peel to the
//             fixpoint: R.  R empty: status 1.
//   stage 1   U = R ∩ {key < t_lo}: non-empty after peeling: status 2, and that is the critical residual.
//   bisection invariant S(hi) = R != ∅, S(lo) = ∅: mid = lo + (hi - lo) / 2, U = R ∩ {key < mid}, reading the 32 keys of only
//             the words in which R has a bit; the CN words are zeroed and rebuilt from U's set bits; peel.  Non-empty: R := U and
//             hi := max(key over U) + 1 (<= mid: S(t) = U for every t above U's largest key, so nothing lies between); empty:
//             lo := mid.  hi - lo == 1: T* = hi.
//   A stage whose U is empty before any peeling (every key of R is >= t) builds and peels nothing.
//   end       the bitmap R, its size, and its first and last position by LDS min / max atomics over R's words.
// R lives where FloodLayout has pos_b.  The per-stage scalars (|U|, |residual|, its largest key) alternate between two slots by
// the parity of the stage: thread 0 clears the other parity's slots after the stage's first barrier, and the barriers of the build
// and the peel order that store before the next stage's atomics; a skipped stage (U empty) has none of those and ends on a
// barrier of its own.
// The phases stay in the kernel's body for the reason eps_stages.h gives.
#include "eps_stages.h"
#include "../../include/scldpc_thresh.h"
#include <climits>

namespace {

using namespace scldpc_dev;

// scal[]: the peel rounds' S_PUSH [0, 3) and S_OVF [3, 6) as in eps_stages.h, then
enum { T_UCNT = 6, T_RCNT = 8, T_MAXK = 10, T_NER = 12, T_PMIN = 13, T_PMAX = 14, T_FCNT = 15 };

struct TArgs : Geo {            // Geo: vns_pos, magic_v, magic_c
    int dv, L, cns_pos, n, ncn, cn_lim, ntrials, key_wide;
    uint32_t t_lo, t_hi;
    Layout lay;
    const void *vn_adj;
    const uint32_t *keys;       // [T][n]
    int32_t *rows;              // [T][SCLDPC_THRESH_NCOLS]
    uint32_t *bits_out;         // optional [T][nw]: the critical residual
    uint32_t *ws;               // [T][ncn] CN words in global memory (ensembles beyond the LDS)
};

// Two 1024-thread workgroups per CU (8 waves per SIMD: at most 64 VGPRs, and 72 SGPRs) wherever the LDS admits them, as
// eps_walk_kernel.  No spills: tests/test_walk_resources.py.
template <int DV, bool A16, class ST>
__global__ __launch_bounds__(kBlock, 8) __attribute__((amdgpu_num_sgpr(72))) void frame_threshold_kernel(const TArgs a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cn_state = ST::kGlobal ? a.ws + (size_t)blockIdx.x * a.ncn : lds + a.lay.cn_state;
    uint32_t *U = lds + a.lay.U;
    uint32_t *fbits = lds + a.lay.fbits;
    uint32_t *R = lds + a.lay.pos_b;
    uint32_t *q[2] = {lds + a.lay.q0, lds + a.lay.q1};
    int *scal = reinterpret_cast<int *>(lds + a.lay.scal);

    int tid = threadIdx.x, lane = tid & 63;
    const int trial = blockIdx.x;
    const int n = a.n, ncn = a.ncn, dv = (DV ? DV : a.dv), cn_lim = a.cn_lim, nw = a.lay.nw, qcap = a.lay.qcap;
    const char *adj = static_cast<const char *>(a.vn_adj) + (size_t)trial * n * dv * (A16 ? 2 : 4);
    const uint32_t *kr = a.keys + (size_t)trial * n;
    const bool wide = a.key_wide != 0;

    if (tid < S_NSCAL) scal[tid] = tid == T_PMIN ? INT_MAX : tid == T_PMAX ? -1 : 0;
    __syncthreads();

    uint32_t lo = a.t_lo, hi = a.t_hi;
    int phase = 0, stage = 0, rescans = 0, status;                 // phase 0: the decode at t_hi; 1: the test at t_lo; 2: the bisection
    for (;;) {
        // (tid made opaque per stage: what the phases derive from it is computed again in every stage instead of being
        // hoisted out of this loop and kept in registers across it: see eps_stages.h)
        asm volatile("" : "+v"(tid));
        lane = tid & 63;
        const uint32_t t = phase == 0 ? hi : phase == 1 ? lo : lo + (hi - lo) / 2;
        const int par = stage & 1;
        // ---- U of this stage and its size; the CN words cleared
        {
            int uc = 0;
            for (int w = tid; w < nw; w += kBlock) {
                const uint32_t r = stage ? R[w] : 0xFFFFFFFFu;
                const uint32_t x = r ? r & key_word(kr, w, n, wide, t, [](int, uint32_t) {}) : 0u;
                U[w] = x;
                uc += __popc(x);
            }
            const uint32_t tot = wave_inclusive_scan((uint32_t)uc);
            if (lane == 63 && tot) atomicAdd(&scal[T_UCNT + par], (int)tot);
        }
        for (int c = tid; c < ST::words(ncn); c += kBlock) cn_state[c] = 0;
        __syncthreads();
        const int ucnt = uniform(scal[T_UCNT + par]);
        if (tid == 0) {                                             // the other parity's slots for the next stage; the first round's
            scal[T_UCNT + (par ^ 1)] = 0; scal[T_RCNT + (par ^ 1)] = 0; scal[T_MAXK + (par ^ 1)] = 0;
            scal[S_PUSH] = 0; scal[S_OVF] = 0;
            if (stage == 0) scal[T_NER] = ucnt;
        }
        int residual = 0;
        uint32_t mk = 0;
        if (ucnt) {                                                 // (the same answer in every thread)
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

            // ---- peeling to the fixpoint (eps_walk_kernel's rounds; the order is irrelevant for the residual) ----
            int ncur = 0, iter = 0;
            bool scan = true;
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
                        if (o[i] == 2u && cc[i] < cn_lim) {         // transition to one VN: may fire
                            const int idx = atomicAdd(&scal[S_PUSH + g], 1);
                            if (idx < qcap) qn[idx] = (uint32_t)cc[i]; else scal[S_OVF + g] = 1;
                        }
                    }
                };
                if (scan) {
                    // every CN < cn_lim holding one VN: at the outset all of them may fire, and after a queue overflow those
                    // found got there by a transition
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
                if (ncur == 0) break;                               // nothing queued: fixpoint
            }
            __syncthreads();

            // ---- what is left, and its largest key ----
            {
                int rc = 0;
                uint32_t mx = 0;
                for (int w = tid; w < nw; w += kBlock) {
                    const uint32_t x = U[w];
                    if (x) {
                        rc += __popc(x);
                        key_word(kr, w, n, wide, 0u, [&](int b, uint32_t k) { if ((x >> b) & 1u) mx = k > mx ? k : mx; });
                    }
                }
                const uint32_t tot = wave_inclusive_scan((uint32_t)rc);
                if (lane == 63 && tot) atomicAdd(&scal[T_RCNT + par], (int)tot);
                if (mx) atomicMax(reinterpret_cast<uint32_t *>(&scal[T_MAXK + par]), mx);
            }
            __syncthreads();
            residual = uniform(scal[T_RCNT + par]);
            mk = (uint32_t)uniform(scal[T_MAXK + par]);
        } else {
            // a skipped stage has no barrier of the build or the peel behind thread 0's clearing of the other parity's slots:
            // without this one another wave could add its |U| of the next stage before that store lands
            __syncthreads();
        }
        stage++;
        if (residual)                                               // R := U, every word by the thread that reads it next
            for (int w = tid; w < nw; w += kBlock) R[w] = U[w];
        if (phase == 0) {
            if (!residual) { status = 1; break; }
            hi = mk + 1;                                            // (below t_lo: the next stage keeps all of R, status 2)
            phase = 1;
        } else if (phase == 1) {
            if (residual) { status = 2; break; }
            phase = 2;                                              // S(lo) = ∅ and S(hi) = R: some key of R is >= lo, hi > lo
        } else {
            if (residual) hi = mk + 1; else lo = t;
        }
        if (phase == 2 && hi - lo <= 1u) { status = 0; break; }
    }

    // ---- the critical residual: its bitmap, its size, its first and last position
    {
        int fc = 0;
        for (int w = tid; w < nw; w += kBlock) {
            const uint32_t x = status == 1 ? 0u : R[w];
            if (a.bits_out) a.bits_out[(size_t)trial * nw + w] = x;
            if (x) {
                fc += __popc(x);
                atomicMin(&scal[T_PMIN], make_vn(a, w * 32 + __ffs((int)x) - 1).pos);
                atomicMax(&scal[T_PMAX], make_vn(a, w * 32 + 31 - __clz((int)x)).pos);
            }
        }
        const uint32_t tot = wave_inclusive_scan((uint32_t)fc);
        if (lane == 63 && tot) atomicAdd(&scal[T_FCNT], (int)tot);
    }
    __syncthreads();
    if (tid == 0) {
        int32_t *o = a.rows + (size_t)trial * SCLDPC_THRESH_NCOLS;
        o[0] = status == 0 ? (int32_t)hi : status == 2 ? (int32_t)a.t_lo : -1;
        o[1] = status;
        o[2] = scal[T_FCNT];
        o[3] = status == 1 ? -1 : scal[T_PMIN];
        o[4] = scal[T_PMAX];
        o[5] = stage;
        o[6] = rescans;
        o[7] = scal[T_NER];
    }
}

}  // namespace

// The launch on walk_launch's front: the shape rule and LDS carve of the eps walks, region for region (full_bp_eps.hip's sizes, so
// that a shape takes the same CN-word form in both kernels; R is the one region of pos_a / pos_b this kernel uses: the 2 L
// position words and the kBins words beside R are deliberately unused).
static int launch_frame_threshold(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                                  const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t *d_rows,
                                  uint32_t *d_bits, const scldpc::Scratch &scratch, void *stream)
{
    return scldpc::walk_launch<TArgs>(who, p, ntrials, !d_rows || !d_keys, d_vn_adj, adj16, scratch, stream,
                                      [](const scldpc_code_params *p) { return 2 * p->L; }, 0, [&](TArgs &a, int ncn) {
        a.rows = d_rows; a.bits_out = d_bits;
        return scldpc::thresh_window(who, p, ncn, d_keys, t_lo, t_hi, is_term, a);
    }, [](auto st, auto dv, auto a16) -> void (*)(const TArgs) {
        return frame_threshold_kernel<decltype(dv)::value, decltype(a16)::value, decltype(st)>;
    });
}

extern "C" int scldpc_frame_threshold_device(const scldpc_code_params *p, int32_t ntrials, const int32_t *d_vn_adj,
                                             const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term, int32_t *d_rows,
                                             uint32_t *d_bits, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_frame_threshold("scldpc_frame_threshold_device", p, ntrials, d_vn_adj, false, d_keys, t_lo, t_hi, is_term, d_rows,
                                  d_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

extern "C" int scldpc_frame_threshold_device_adj16(const scldpc_code_params *p, int32_t ntrials, const uint16_t *d_vn_adj16,
                                                   const uint32_t *d_keys, uint32_t t_lo, uint32_t t_hi, int32_t is_term,
                                                   int32_t *d_rows, uint32_t *d_bits, void *d_workspace, uint64_t workspace_bytes,
                                                   void *stream)
{
    return launch_frame_threshold("scldpc_frame_threshold_device_adj16", p, ntrials, d_vn_adj16, true, d_keys, t_lo, t_hi, is_term,
                                  d_rows, d_bits, scldpc::Scratch{d_workspace, workspace_bytes, nullptr}, stream);
}

// workspace of scldpc_frame_threshold_device(_adj16) for ntrials frames
extern "C" int64_t scldpc_frame_threshold_workspace_query(const scldpc_code_params *p, int32_t ntrials, int32_t adj16)
{
    uint64_t need = 0;
    const int rc = launch_frame_threshold("scldpc_frame_threshold_workspace_query", p, ntrials, nullptr, adj16 != 0, nullptr, 0u, 1u, 1,
                                          nullptr, nullptr, scldpc::Scratch{nullptr, 0, &need}, nullptr);
    return rc ? (int64_t)rc : (int64_t)need;
}
