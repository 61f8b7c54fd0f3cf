// Unlimited full BP of one sampled code at every point of a descending eps grid, in one launch (include/scldpc_bp_eps.h) —
// gfx950 kernel: full BP's end of a stage of eps_stages.h's walk.
//
// On the BEC the set flooding BP converges to is the maximal stopping set inside the erased set E over the CNs below cn_lim
// (full_bp_fixpoint_kernel rests on it): the order in which CNs fire does not matter, only the iteration
// count does, and nobody asks for it here.  That is what the walk rests on; full BP has no sweep start, so there is no
// exception to the identity.  (With an iteration cap the result depends on the schedule: the entry takes none.)
//   end of stage k  the CN words hold the counts over the residual R_k as the peeling left them, which is the state
//            full_bp_fixpoint_kernel ends on: count_size2_sets with the per-position counts, the erased bits,
//            write_full_bp_counters(ne = |R_k|, the stage's rounds, status 0, #erased at point k).
// pos_a holds pos_cnt [L] and pos_ss [L].
#include "eps_stages.h"
#include "../../include/scldpc_bp_eps.h"

namespace {

using namespace scldpc_dev;

struct BpEnd {
    struct Args : Geo {         // Geo: vns_pos, magic_v, magic_c
        int dv, L, cns_pos, n, ncn, cn_lim, npoints, ntrials, lev_wide;
        Layout lay;
        const void *vn_adj;
        const uint8_t *levels;  // [T][n]
        int32_t *counters;      // [K][T][SCLDPC_NCOUNTERS]
        uint32_t *bits_out;     // optional [K][T][nw]: the VNs still erased
        uint32_t *ws;           // [T][ncn] CN words in global memory (ensembles beyond the LDS)
    };
    static constexpr int kPosArrays = 2;
    static constexpr bool kRebuilds = false;
    static __device__ __forceinline__ int cn_lim(const Args &a) { return a.cn_lim; }
    static int pos_words(const scldpc_code_params *p) { return 2 * p->L; }

    // decodeBP's end on the CN words as the peeling left them (BPF:1067-1133)
    template <class ST, int DV, bool A16>
    static __device__ __forceinline__ void finish(const Args &a, const char *adj, int dv, int, uint32_t *cn_state, uint32_t *U,
                                  int *pos_cnt, int *pos_ss, int *, const int *bins, int nw, int tid, int, int trial, int stage,
                                  int residual, int iter, int, int32_t (&)[8], int32_t (&)[8])
    {
        count_size2_sets<ST, DV, A16, kBlock>(a, adj, dv, a.cns_pos, cn_state, U, nw, tid, pos_ss,
                                              [&](const Vn &v) { atomicAdd(&pos_cnt[v.pos], 1); });
        __syncthreads();
        const size_t row = (size_t)stage * a.ntrials + trial;
        if (a.bits_out)
            for (int w = tid; w < nw; w += kBlock) a.bits_out[row * nw + w] = U[w];
        if (tid == 0)                                               // ITERATIONS = the peeling rounds of this stage
            write_full_bp_counters(a.counters + row * SCLDPC_NCOUNTERS, pos_cnt, pos_ss, a.L, residual, iter, 0, bins[stage + 1]);
    }

    static __device__ __forceinline__ void zero_row(const Args &a, size_t row, int iter, int, int nerased)
    {
        int32_t *o = a.counters + row * SCLDPC_NCOUNTERS;
        o[SCLDPC_C_NUM_ERASURES] = 0; o[SCLDPC_C_NUM_BLOCKS_ERR] = 0; o[SCLDPC_C_NUM_ERASURES_EXP] = 0;
        o[SCLDPC_C_NUM_BLOCKS_ERR_EXP] = 0; o[SCLDPC_C_NUM_ERASURES_P1] = 0;
        o[SCLDPC_C_ITERATIONS] = iter;
        o[SCLDPC_C_STATUS] = 0;
        o[SCLDPC_C_CHANNEL_ERASURES] = nerased;
    }
};

}  // namespace

static int launch_full_bp_eps(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                              const uint8_t *d_levels, int32_t npoints, int32_t is_term, int32_t *d_counters,
                              uint32_t *d_erased_bits, const scldpc::Scratch &scratch, void *stream)
{
    return scldpc::eps_walk_launch<BpEnd>(who, p, ntrials, d_vn_adj, adj16, d_levels, npoints, d_counters, d_erased_bits, scratch,
                                          stream, [&](BpEnd::Args &a, int ncn) {
        a.cn_lim = is_term ? ncn : p->L * p->cns_pos;               // BPT:944-948
        a.counters = d_counters;
        return (int)SCLDPC_OK;
    });
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
