// Sweep peeling of one sampled code at every point of a descending eps grid, in one launch (include/scldpc_eps.h) — gfx950 kernel:
// the sweep decoder's end of a stage of eps_stages.h's walk.
//
// peel_sweep.hip's trial with sweep_start = 0: every CN < total_size that holds one VN fires, at the outset or after a
// transition, so the residual is the maximal stopping set inside the erased set E (no CN of the residual's graph below
// total_size holds exactly one of its VNs, and peeling never removes a VN of a stopping set), which is what the walk rests on.
// (With sweep_start > 0 a CN below it fires only on a TRANSITION to one VN, which depends on the outset: the identity is false
// there and the entry takes no sweep_start.)
//   end of stage k  the lost / component / expurgation pass of peel_sweep_kernel unchanged: it rebuilds the CN words, which the
//            walk has zeroed, over the lost VNs and overwrites U (R is kept); the lost bits; out[k][trial], with the stage's
//            re-scans on their own in out[6].
// pos_a holds pos_flag [L].
#include "eps_stages.h"

namespace {

using namespace scldpc_dev;

struct PeelEnd {
    struct Args : Geo {         // Geo: vns_pos, magic_v, magic_c
        int dv, L, cns_pos, n, ncn, total_size, lost_lo, lost_hi, npoints, ntrials, lev_wide;
        Layout lay;
        const void *vn_adj;
        const uint8_t *levels;  // [T][n]
        int32_t *out;           // [K][T][8]: lost, lost_exp, blocks_failed_exp, 0, 0, rounds and re-scans of the stage, #erased at the point
        uint32_t *bits_out;     // optional [K][T][nw]: the lost VNs
        uint32_t *ws;           // [T][ncn] CN words in global memory (ensembles beyond the LDS)
    };
    static constexpr int kPosArrays = 1;
    static constexpr bool kRebuilds = true;
    static __device__ __forceinline__ int cn_lim(const Args &a) { return a.total_size; }
    static int pos_words(const scldpc_code_params *p) { return p->L + p->dv; }

    template <class ST, int DV, bool A16>
    static __device__ __forceinline__ void finish(const Args &a, const char *adj, int dv, int cn_lim, uint32_t *cn_state, uint32_t *U,
                                  int *pos_flag, int *, int *scal, const int *bins, int nw, int tid, int lane, int trial, int stage,
                                  int residual, int iter, int rescans, int32_t (&cc)[8], int32_t (&cb)[8])
    {
        auto is_lost = [&](int j, int32_t (&cc)[8]) {
            load_adj<DV, A16>(adj, dv, j, (int)__umulhi((uint32_t)j, a.magic_v), a.cns_pos, cc);
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
        for (int w = tid; w < nw; w += kBlock) {
            uint32_t x = U[w], keep = 0;
            while (x) {
                const int b = __ffs((int)x) - 1;
                x &= x - 1;
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
        if (a.bits_out)
            for (int w = tid; w < nw; w += kBlock) a.bits_out[row * nw + w] = U[w];
        if (tid == 0) {
            int blocks = 0;
            for (int pos = 0; pos < a.L; pos++) blocks += pos_flag[pos];
            int32_t *o = a.out + row * 8;
            o[0] = scal[S_LOST]; o[1] = scal[S_LOST_EXP]; o[2] = blocks; o[3] = 0; o[4] = 0; o[5] = iter; o[6] = rescans;
            o[7] = bins[stage + 1];
        }
    }

    static __device__ __forceinline__ void zero_row(const Args &a, size_t row, int iter, int rescans, int nerased)
    {
        int32_t *o = a.out + row * 8;
        o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = iter; o[6] = rescans; o[7] = nerased;
    }
};

}  // namespace

static int launch_peel_sweep_eps(const char *who, const scldpc_code_params *p, int32_t ntrials, const void *d_vn_adj, bool adj16,
                                 const uint8_t *d_levels, int32_t npoints, int32_t total_size, int32_t lost_lo, int32_t lost_hi,
                                 int32_t *d_out, uint32_t *d_lost_bits, const scldpc::Scratch &scratch, void *stream)
{
    return scldpc::eps_walk_launch<PeelEnd>(who, p, ntrials, d_vn_adj, adj16, d_levels, npoints, d_out, d_lost_bits, scratch, stream,
                                            [&](PeelEnd::Args &a, int ncn) {
        if (total_size < 0 || total_size > ncn || lost_lo < 0 || lost_hi > ncn)
            return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: CN ranges outside [0,%d]", who, ncn);
        a.total_size = total_size; a.lost_lo = lost_lo; a.lost_hi = lost_hi; a.out = d_out;
        return (int)SCLDPC_OK;
    });
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
