// Throughput-mode sampling of the UNCOUPLED (dv, dc) ensemble on the device (gfx950): ldpc.gen_slots with its repeat
// rejection (ldpc.py:45-84, PD:134-135) — one uniformly random permutation of the S = dv * M sockets, socket dv*t+i wired to
// edge i of VN t, CN = rank / dc, redrawn until no VN meets a CN twice — and the channel of the accepted draw.
// The law and the keys (include/scldpc_uncoupled.h): trial t tries attempts a = 0, 1, 2, ..; candidate a is the one position
// of the tail-biting sampler at L = 1 (sampler.hip, stream 0) under trial' = t + (a << 40), i.e. with a << 8 added to the
// high counter word; the first candidate without a repeated CN in a VN row is the trial's graph, the channel words are those
// of the same trial' (stream 2^31, independent of the graph keys, so acceptance does not bias them).
// One 1024-thread workgroup per trial and no word between workgroups.  An attempt is the ranking of sampler.hip's first
// generation, restated here (its twenty shipped instances keep their instruction text): byte-wide bucket counters four to a
// word, the atomic's return value as arrival slot, a DPP scan, the keys grouped by bucket, rank = bucket base + smaller
// bucket-mates (ties by socket).  Then the CN ids go, 2 bytes each, into the room of the dead counters, every VN tests its dv
// entries pairwise, and the workgroup reads ONE LDS word behind a barrier: every thread sees the same verdict and all leave
// the loop together.  Nothing reaches global memory before that: only the accepted attempt (or the cap) writes.
// No trap: sixteen keys in one bucket (never, for Philox keys: the mean is 0.25) end the trial with attempts = -1 and zero
// outputs, which the caller reports.
#include "sampler_common.h"
#include "philox.h"
#include "../../include/scldpc_uncoupled.h"

namespace {

constexpr int kThreads = scldpc::kSamplerThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSockets = 8192;
constexpr int kMaxAttempts = 1 << 24;
constexpr unsigned long long kMaxTrials = 1ull << 40;

struct UArgs {
    int dv, dc, vns_pos, S, nb, shift, dc_shift, nw;
    int max_attempts;
    uint32_t crowd_limit;       // an arrival slot at or past it ends the trial with -1 (15: the count would leave its nibble)
    uint32_t seed_lo, seed_hi;
    unsigned long long trial0;
    uint32_t thresh;            // erased iff (draw >> 1) < thresh
    int off_gkey, off_gidx, off_wsum;            // LDS offsets in 32-bit words
    int32_t *vn_adj;            // int32 [T][M][dv]
    uint32_t *chan;             // [T][nw]
    int32_t *attempts;          // [T]
};

using scldpc_dev::channel_erased;
using scldpc_dev::channel_tail;
using scldpc_dev::philox4x32_10;
using scldpc_dev::wave_inclusive_scan;

// KMAX = Philox calls per thread per attempt (4 sockets each); ROWS = 64-counter rows each wave scans (nb = 1024 * ROWS words).
// LDS: hist [nb] | gkey [S] | gidx [S] 2 B | wsum [16], verdict, crowded.  The S 2-byte CN ids of an attempt take the room of
// hist, which is dead once the keys are grouped.  80 SGPRs at most, as sampler.hip explains: two workgroups share a CU.
template <int KMAX, int ROWS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_num_sgpr(72))) void sample_uncoupled_kernel(const UArgs a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *hist = lds;                                           // nb words of four byte-wide counters -> scanned words
    uint16_t *cn = reinterpret_cast<uint16_t *>(lds);               // S CN ids (after the grouping)
    uint32_t *gkey = lds + a.off_gkey;                              // S keys grouped by bucket
    uint16_t *gidx = reinterpret_cast<uint16_t *>(lds + a.off_gidx);   // S socket ids, same order
    uint32_t *wsum = lds + a.off_wsum;                              // per-wave totals; [kWaves] verdict, [kWaves + 1] crowded

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long trial = a.trial0 + blockIdx.x;
    const uint32_t t_lo = (uint32_t)trial, t_hi0 = (uint32_t)(trial >> 32);      // trial < 2^40: t_hi0 < 256
    const int S = a.S, nb = a.nb, dv = a.dv;
    const int ncalls = (S + 3) >> 2;
    const int kshift = a.shift - 2;                                 // key >> kshift = bucket (4 * nb of them)

    if (tid == 0) { wsum[kWaves] = 0; wsum[kWaves + 1] = 0; }
    int status = 0;             // attempts of the accepted draw; 0: none within max_attempts; -1: a crowded bucket
    uint32_t t_hi = t_hi0;
    for (int att = 0; att < a.max_attempts; att++) {
        t_hi = t_hi0 + ((uint32_t)att << 8);                        // trial' = trial + (att << 40)
        for (int b = tid; b < nb; b += kThreads) hist[b] = 0;       // (the CN ids of the attempt before: all read, barrier 7)
        __syncthreads();                                            // 1

        // ---- keys + bucket histogram; the atomic's return value is the arrival slot in the bucket
        uint32_t key[KMAX * 4], slot[KMAX * 4], crowded = 0;
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            const int q = tid + k * kThreads;
            if (q < ncalls) {
                uint32_t r[4];
                philox4x32_10((uint32_t)q, 0u, t_lo, t_hi, a.seed_lo, a.seed_hi, r);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    key[k * 4 + u] = r[u];
                    slot[k * 4 + u] = 0;
                    if (q * 4 + u < S) {
                        const uint32_t b = r[u] >> kshift, sh = (b & 3u) * 8u;
                        slot[k * 4 + u] = (atomicAdd(&hist[b >> 2], 1u << sh) >> sh) & 0xFFu;
                        crowded = max(crowded, slot[k * 4 + u]);
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) { key[k * 4 + u] = 0; slot[k * 4 + u] = 0; }
            }
        }
        if (crowded >= a.crowd_limit) wsum[kWaves + 1] = 1u;        // a bucket count must fit its nibble
        __syncthreads();                                            // 2
        if (wsum[kWaves + 1] != 0u) { status = -1; break; }         // one word, written before the barrier only: uniform

        // ---- exclusive scan of the bucket counts.  Each wave owns nb/16 contiguous words = ROWS rows of 64; the rows are
        //      scanned independently (DPP) and chained by their totals; after the barrier every wave scans the 16 slice
        //      totals itself and folds its own slice base into its words, so a reader needs ONE word per key:
        //      word = [global exclusive prefix:14 | c0:4 | c1:4 | c2:4 | c3:4]  (base of bucket k = prefix + c0..c(k-1)).
        uint32_t mine[ROWS];
        {
            const int base = wave * (ROWS * 64) + lane;
            uint32_t v[ROWS], inc[ROWS], raw[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                raw[r] = hist[base + r * 64];
                v[r] = (raw[r] * 0x01010101u) >> 24;                // keys in the word's four buckets
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++) inc[r] = wave_inclusive_scan(v[r]);
            uint32_t carry = 0;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const uint32_t excl = carry + inc[r] - v[r], x = raw[r];        // byte counts (each < 16, checked above) -> nibbles
                mine[r] = excl | ((x & 0xFu) << 14) | (((x >> 8) & 0xFu) << 18) | (((x >> 16) & 0xFu) << 22) | ((x >> 24) << 26);
                carry += (uint32_t)__builtin_amdgcn_readlane((int)inc[r], 63);
            }
            if (lane == 0) wsum[wave] = carry;
        }
        __syncthreads();                                            // 3
        {
            const uint32_t t = lane < kWaves ? wsum[lane] : 0u;
            const uint32_t inc = wave_inclusive_scan(t);
            const uint32_t slice = (uint32_t)__builtin_amdgcn_readlane((int)(inc - t), wave);
            const int base = wave * (ROWS * 64) + lane;
#pragma unroll
            for (int r = 0; r < ROWS; r++) hist[base + r * 64] = mine[r] + slice;
        }
        __syncthreads();                                            // 4

        // ---- group (key, socket) by bucket: the bucket words of the thread's keys are read together, one wait, then the stores
        constexpr int E = KMAX * 4;
        uint32_t g0s[E], g1s[E];
        {
            uint32_t b0[E], h0[E];
            bool ok[E];
#pragma unroll
            for (int e = 0; e < E; e++) {
                const int q = tid + (e >> 2) * kThreads, sck = q * 4 + (e & 3);
                ok[e] = q < ncalls && sck < S;
                b0[e] = ok[e] ? key[e] >> kshift : 0u;
                h0[e] = hist[b0[e] >> 2];
            }
#pragma unroll
            for (int e = 0; e < E; e++) {
                const uint32_t k = b0[e] & 3u, h = h0[e];
                const uint32_t c0 = (h >> 14) & 15u, c1 = (h >> 18) & 15u, c2 = (h >> 22) & 15u;
                g0s[e] = (h & 0x3FFFu) + (k > 0 ? c0 : 0u) + (k > 1 ? c1 : 0u) + (k > 2 ? c2 : 0u);
                g1s[e] = g0s[e] + ((h >> (14u + 4u * k)) & 15u);
                if (!ok[e]) g0s[e] = g1s[e] = 0;
            }
#pragma unroll
            for (int e = 0; e < E; e++) {
                if (ok[e] && g1s[e] - g0s[e] > 1u) {                // a key alone in its bucket has rank g0: nothing to compare
                    const uint32_t g = g0s[e] + slot[e];
                    gkey[g] = key[e];
                    gidx[g] = (uint16_t)((tid + (e >> 2) * kThreads) * 4 + (e & 3));
                }
            }
        }
        __syncthreads();                                            // 5: the scanned words are dead, their room takes the CN ids

        // ---- rank = bucket base + #(smaller (key, socket) pairs in the bucket); CN = rank / dc.  Step k reads bucket-mate k
        //      of each of the thread's keys, the socket id only on a key tie.
        {
            uint32_t rank[E], span = 0;
#pragma unroll
            for (int e = 0; e < E; e++) { rank[e] = g0s[e]; span = max(span, g1s[e] - g0s[e]); }
            for (uint32_t step = 0; step < span; step++) {
                uint32_t k2[E];
                bool on[E], tie = false;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const uint32_t g = g0s[e] + step;
                    on[e] = g < g1s[e] && step != slot[e];          // slot[e] is this key's own place in the bucket
                    k2[e] = gkey[on[e] ? g : 0u];
                }
#pragma unroll
                for (int e = 0; e < E; e++) {
                    rank[e] += on[e] && k2[e] < key[e];
                    tie |= on[e] && k2[e] == key[e];
                }
                if (tie) {
#pragma unroll
                    for (int e = 0; e < E; e++)
                        if (on[e] && k2[e] == key[e])
                            rank[e] += gidx[g0s[e] + step] < (uint16_t)((tid + (e >> 2) * kThreads) * 4 + (e & 3));
                }
            }
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                const int q = tid + k * kThreads, s0 = q * 4;
                uint32_t id[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t r = rank[k * 4 + u];
                    id[u] = a.dc_shift >= 0 ? r >> a.dc_shift : r / (uint32_t)a.dc;
                }
                if (q < ncalls && s0 + 3 < S) {                     // (the ids start at an 8-byte boundary: one store for 4 sockets)
                    uint2 v; v.x = id[0] | (id[1] << 16); v.y = id[2] | (id[3] << 16);
                    *reinterpret_cast<uint2 *>(cn + s0) = v;
                } else if (q < ncalls) {
#pragma unroll
                    for (int u = 0; u < 4; u++) if (s0 + u < S) cn[s0 + u] = (uint16_t)id[u];
                }
            }
        }
        __syncthreads();                                            // 6

        // ---- no VN may hold a CN twice (ldpc.py:67-84): VN t owns entries dv*t .. dv*t + dv - 1
        bool twice = false;
        for (int t = tid; t < a.vns_pos; t += kThreads) {
            const uint16_t *row = cn + t * dv;
            for (int i = 1; i < dv; i++) {
                const uint16_t ci = row[i];
                for (int j = 0; j < i; j++) twice |= row[j] == ci;
            }
        }
        if (twice) wsum[kWaves] = (uint32_t)att + 1u;               // every writer of this attempt stores the same value
        __syncthreads();                                            // 7
        if (wsum[kWaves] != (uint32_t)att + 1u) { status = att + 1; break; }    // uniform; next written behind six barriers
    }

    // ---- the accepted draw goes out: rows (socket order IS row order: full-line stores), channel words, attempts.
    //      Without one every element is zero.
    const bool got = status > 0;
    int32_t *rows = a.vn_adj + (size_t)blockIdx.x * S;
    for (int e = tid; e < S; e += kThreads) rows[e] = got ? (int32_t)cn[e] : 0;
    uint32_t *chan = a.chan + (size_t)blockIdx.x * a.nw;
    for (int w = tid; w < a.nw; w += kThreads) {
        uint32_t word = 0;
        if (got) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                uint32_t r[4];
                philox4x32_10((uint32_t)(w * 8 + c), 0x80000000u, t_lo, t_hi, a.seed_lo, a.seed_hi, r);
#pragma unroll
                for (int u = 0; u < 4; u++) word |= channel_erased(r[u], a.thresh) << (c * 4 + u);
            }
            word = channel_tail(word, w * 32, a.vns_pos);
        }
        chan[w] = word;
    }
    if (tid == 0) a.attempts[blockIdx.x] = status;
}

// the shape rule, in the header's order; pure
int shape(const char *who, const scldpc_code_params *p)
{
    if (int rc = scldpc::check_params(p)) return rc;
    if (p->L != 1)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: the uncoupled ensemble is one position: L must be 1 (got L = %d)", who, p->L);
    if (p->dv > 8)
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: dv <= 8 (got dv = %d)", who, p->dv);
    if ((int64_t)p->cns_pos * p->dc > kMaxSockets)
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: at most %d sockets, cns_pos * dc (got %lld)", who, kMaxSockets,
                                 (long long)p->cns_pos * p->dc);
    if (p->dv > p->cns_pos)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: no simple graph with dv > cns_pos (got dv = %d, cns_pos = %d)", who,
                                 p->dv, p->cns_pos);
    return SCLDPC_OK;
}

}  // namespace

extern "C" int scldpc_sample_philox_uncoupled_supported(const scldpc_code_params *p)
{
    return shape("scldpc_sample_philox_uncoupled_supported", p) == SCLDPC_OK;
}

extern "C" int scldpc_sample_philox_uncoupled_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
                                                     double eps, int32_t max_attempts, int32_t *d_vn_adj, uint32_t *d_chan_bits,
                                                     int32_t *d_attempts, void *stream)
{
    const char *who = "scldpc_sample_philox_uncoupled_device";
    if (int rc = shape(who, p)) return rc;
    if (!(eps >= 0.0 && eps <= 1.0))
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: eps=%g outside [0,1]", who, eps);
    if (max_attempts < 1 || max_attempts > kMaxAttempts)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: 1 <= max_attempts <= %d (got %d)", who, kMaxAttempts, max_attempts);
    if (trial0 > kMaxTrials || (ntrials > 0 && trial0 + (uint64_t)ntrials > kMaxTrials))
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: trial0 + ntrials <= 2^40 (attempt a of trial t is keyed t + (a << 40))", who);
    if (ntrials < 0)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: negative ntrials", who);
    if (ntrials == 0) return SCLDPC_OK;
    if (!d_vn_adj || !d_chan_bits || !d_attempts)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer", who);

    UArgs a{};
    a.dv = p->dv; a.dc = p->dc; a.vns_pos = p->vns_pos; a.S = p->cns_pos * p->dc; a.nw = scldpc::nw_of(p);
    int lg = 10;                                    // nb = power of two >= max(S, kThreads), at most 8192
    while ((1 << lg) < a.S) lg++;
    a.nb = 1 << lg; a.shift = 32 - lg;
    a.dc_shift = -1;
    for (int k = 0; k < 8; k++) if ((1 << k) == p->dc) a.dc_shift = k;
    a.max_attempts = max_attempts;
    a.crowd_limit = 15;
    if (const char *v = getenv("SCLDPC_DEBUG_UNCOUPLED_CROWD_LIMIT"))        // diagnostics / tests only
        a.crowd_limit = (uint32_t)std::min(15, std::max(1, atoi(v)));
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.thresh = scldpc::erasure_threshold(eps);
    int off = a.nb;
    a.off_gkey = off; off += (a.S + 3) & ~3;
    a.off_gidx = off; off += ((a.S + 1) / 2 + 3) & ~3;
    a.off_wsum = off; off += 32;
    const size_t lds_bytes = 4u * (size_t)off;     // 80 KiB + 128 B at 8192 sockets
    a.vn_adj = d_vn_adj; a.chan = d_chan_bits; a.attempts = d_attempts;

    const int kmax = ((a.S + 3) / 4 + kThreads - 1) / kThreads;     // 1 or 2
    const int rows = a.nb / kThreads;                               // 1, 2, 4 or 8 rows of 64 per wave
    void (*kern)(const UArgs) = kmax == 1 && rows <= 4 ? (rows == 1 ? sample_uncoupled_kernel<1, 1> : rows == 2 ? sample_uncoupled_kernel<1, 2>
                                                                                                    : sample_uncoupled_kernel<1, 4>)
                                                       : sample_uncoupled_kernel<2, 8>;
    if (int rc = scldpc::allow_max_lds(reinterpret_cast<const void *>(kern))) return rc;
    hipLaunchKernelGGL(kern, dim3(ntrials), dim3(kThreads), lds_bytes, static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}
