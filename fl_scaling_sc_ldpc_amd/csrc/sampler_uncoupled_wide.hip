// The rejection sampler of the UNCOUPLED (dv, dc) ensemble up to 32 768 sockets (gfx950): the law of sampler_uncoupled.hip and
// include/scldpc_uncoupled.h, bit for bit — candidate a of trial t is the one position of the tail-biting sampler at L = 1 under
// trial' = t + (a << 40), sockets ranked by (key, socket), CN = rank / dc, the first candidate without a repeated CN in a VN row
// is the graph, the channel words are those of the same trial' — in a kernel whose LDS does not grow with the keys.
// One 1024-thread workgroup per trial, no word between workgroups, the attempt loop inside the kernel.  What differs from the
// first kernel is the ranking.  The keys stay in REGISTERS (Philox call q = tid + 1024 k, up to eight calls per thread); LDS
// holds, per attempt,
//   * 2-byte counters, one per bucket of the top key bits, which the scan turns into 2-byte first ranks and the grouping,
//     which uses them as cursors, into end ranks: a bucket's ranks are [end[b - 1], end[b]).  A 2-byte count cannot wrap (at
//     most 32 768 keys), so there is no crowded-bucket limit here;
//   * the packed words (key << lg | socket) of the part's keys, grouped by bucket.  lg = log2(buckets) >= log2(S): the word
//     drops exactly the bucket's own bits, so comparing two words of one bucket compares (key, socket): key ties are ordered;
//   * the S 2-byte CN ids, in socket order, for the repeat test and the accepted rows.
// Up to 16 384 sockets the whole key range is ranked at once (P = 1; 128 KiB at 16 384).  Beyond, P = 4 PARTS by the two top
// key bits are ranked one after the other through the same counters and packed words (8192 buckets, kPartCap words), each part
// on top of the parts before it.  The one capacity random keys could reach is a part's size: Binomial(S, 1/4) against
// kPartCap = 12 288, mean at most 8192 — a Chernoff bound of exp(-819) per part.  A part beyond the cap ends the
// trial with attempts = -1 and zero outputs; no trap.  SCLDPC_DEBUG_UNCOUPLED_WIDE_PART_CAP lowers the cap (tests of that path).
// Barriers per attempt: 6 P + 1, the same in every attempt; the verdict and the part total are read by all threads from LDS
// words behind a barrier, so every thread leaves the loop in the same attempt.  Nothing reaches global memory before that.
#include "sampler_common.h"
#include "philox.h"
#include "../../include/scldpc_uncoupled_wide.h"

namespace {

constexpr int kThreads = scldpc::kSamplerThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSockets = 32768;
constexpr int kOnePartSockets = 16384;          // up to here P = 1
constexpr int kPartCap = 12288;                 // P = 4: packed words of one part
constexpr int kMaxAttempts = 1 << 24;
constexpr unsigned long long kMaxTrials = 1ull << 40;

struct WArgs {
    int dv, dc, vns_pos, S, nbp, lg, dc_shift, nw;      // nbp buckets per part; lg = log2(all buckets) = socket bits of a packed word
    int max_attempts;
    uint32_t part_cap;          // a part of more keys ends the trial with -1
    uint32_t seed_lo, seed_hi;
    unsigned long long trial0;
    uint32_t thresh;            // erased iff (draw >> 1) < thresh
    int off_gpk, off_cn, off_wsum;               // LDS offsets in 32-bit words
    int32_t *vn_adj;            // int32 [T][M][dv]
    uint32_t *chan;             // [T][nw]
    int32_t *attempts;          // [T]
};

using scldpc_dev::channel_erased;
using scldpc_dev::channel_tail;
using scldpc_dev::philox4x32_10;
using scldpc_dev::wave_inclusive_scan;

// The keys are all a thread keeps from phase to phase.  Left alone the compiler also keeps every key's bucket, shift and packed
// word (they do not change from part to part, so it hoists them out of the part loop): four registers per key where one is
// meant.  An empty asm statement makes the key opaque at the head of a phase, so what a phase derives from it dies with the phase.
// The same for the thread id: the 4 KMAX socket numbers and their "below S" masks are cheap to make and dear to keep.
__device__ __forceinline__ void forget_derived(uint32_t &key) { asm volatile("" : "+v"(key)); }
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }

// KMAX = Philox calls per thread per attempt (4 sockets each); 1 << LGP parts; WPT = counter words a thread scans
// (nbp = 2048 * WPT buckets per part).
// LDS: cnt [nbp / 2 words: two 2-byte counters / first ranks / end ranks each] | gpk [S or kPartCap] |
// cn [S] 2 B | wsum [16], verdict.
template <int KMAX, int LGP, int WPT>
__global__ __launch_bounds__(kThreads) void sample_uncoupled_wide_kernel(const WArgs a)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cnt = lds;
    const uint16_t *ends = reinterpret_cast<const uint16_t *>(lds);    // after the grouping: the end rank of every bucket
    uint32_t *gpk = lds + a.off_gpk;
    uint16_t *cn = reinterpret_cast<uint16_t *>(lds + a.off_cn);
    uint32_t *wsum = lds + a.off_wsum;                                  // per-wave totals; [kWaves] verdict

    constexpr int E = KMAX * 4, P = 1 << LGP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long trial = a.trial0 + blockIdx.x;
    const uint32_t t_lo = (uint32_t)trial, t_hi0 = (uint32_t)(trial >> 32);      // trial < 2^40: t_hi0 < 256
    const int S = a.S, dv = a.dv, lg = a.lg;
    const int ncalls = (S + 3) >> 2;
    const int kshift = 32 - lg;                                         // key >> kshift = bucket, its top LGP bits the part
    const uint32_t bmask = (uint32_t)a.nbp - 1u;
    const int nwords = a.nbp >> 1;                                      // counter words = WPT * kThreads

    if (tid == 0) wsum[kWaves] = 0;
    int status = 0;             // attempts of the accepted draw; 0: none within max_attempts; -1: a part beyond its room
    uint32_t t_hi = t_hi0;
    for (int att = 0; att < a.max_attempts; att++) {
        t_hi = t_hi0 + ((uint32_t)att << 8);                            // trial' = trial + (att << 40)
        uint32_t key[E];
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            const int q = tid + k * kThreads;
            uint32_t r[4] = {0u, 0u, 0u, 0u};
            if (q < ncalls) philox4x32_10((uint32_t)q, 0u, t_lo, t_hi, a.seed_lo, a.seed_hi, r);
#pragma unroll
            for (int u = 0; u < 4; u++) key[k * 4 + u] = r[u];
            __builtin_amdgcn_sched_barrier(0);                          // one call's rounds at a time: the keys fill the registers
        }

        uint32_t base = 0;                                              // keys of the parts before this one
#pragma unroll 1
        for (int part = 0; part < P; part++) {
            for (int w = tid; w < nwords; w += kThreads) cnt[w] = 0;
            __syncthreads();                                            // A

            // ---- bucket counts
            const int tid1 = opaque(tid);
#pragma unroll
            for (int e = 0; e < E; e++) {
                const int sck = (tid1 + (e >> 2) * kThreads) * 4 + (e & 3);
                if ((e & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                forget_derived(key[e]);
                if (sck < S && (LGP == 0 || (int)(key[e] >> (32 - (LGP ? LGP : 1))) == part)) {
                    const uint32_t b = (key[e] >> kshift) & bmask;
                    atomicAdd(&cnt[b >> 1], 1u << ((b & 1u) * 16u));
                }
            }
            __syncthreads();                                            // B

            // ---- exclusive scan: a thread owns WPT consecutive words, the wave scans the thread totals (DPP), the 16 wave
            //      totals meet in wsum; every wave scans them itself.  word = [first rank of b + 1:16 | first rank of b:16].
            uint32_t x[WPT], tot = 0;
            scldpc_dev::load_hist_words<WPT>(cnt, tid, x);
#pragma unroll
            for (int r = 0; r < WPT; r++) tot += (x[r] & 0xFFFFu) + (x[r] >> 16);
            const uint32_t inc = wave_inclusive_scan(tot);
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();                                            // C
            const uint32_t wt = lane < kWaves ? wsum[lane] : 0u;
            const uint32_t winc = wave_inclusive_scan(wt);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)winc, kWaves - 1);
            uint32_t p0 = inc - tot + (uint32_t)__builtin_amdgcn_readlane((int)(winc - wt), wave);
#pragma unroll
            for (int r = 0; r < WPT; r++) {
                const uint32_t lo = x[r] & 0xFFFFu, hi = x[r] >> 16;
                x[r] = p0 | ((p0 + lo) << 16);                          // at most 32 768: 16 bits hold it
                p0 += lo + hi;
            }
            scldpc_dev::store_hist_words<WPT>(cnt, tid, x);
            __syncthreads();                                            // D
            if (total > a.part_cap) { status = -1; break; }             // the same 16 words for every thread: uniform

            // ---- the packed words grouped by bucket: the bucket's first rank is a cursor, the atomic's return value the
            //      key's place.  (The order within a bucket is that of arrival; the ranking below does not read it.)
            //      Afterwards entry b holds the END of bucket b, which is the first rank of bucket b + 1.
            const int tid2 = opaque(tid);
#pragma unroll
            for (int e = 0; e < E; e++) {
                const int sck = (tid2 + (e >> 2) * kThreads) * 4 + (e & 3);
                if ((e & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                forget_derived(key[e]);
                if (sck < S && (LGP == 0 || (int)(key[e] >> (32 - (LGP ? LGP : 1))) == part)) {
                    const uint32_t b = (key[e] >> kshift) & bmask, sh = (b & 1u) * 16u;
                    const uint32_t g = (atomicAdd(&cnt[b >> 1], 1u << sh) >> sh) & 0xFFFFu;
                    gpk[g] = (key[e] << lg) | (uint32_t)sck;
                }
            }
            __syncthreads();                                            // E

            // ---- rank = keys of the parts before + bucket base + smaller bucket-mates; CN = rank / dc
            const int tid3 = opaque(tid);
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                uint32_t g0[4], g1[4];
                bool live[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int sck = (tid3 + k * kThreads) * 4 + u;
                    forget_derived(key[k * 4 + u]);
                    const uint32_t kk = key[k * 4 + u];
                    live[u] = sck < S && (LGP == 0 || (int)(kk >> (32 - (LGP ? LGP : 1))) == part);
                    const uint32_t b = live[u] ? (kk >> kshift) & bmask : 0u;
                    g1[u] = ends[b];
                    g0[u] = ends[b > 0u ? b - 1u : 0u];
                    if (b == 0u) g0[u] = 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!live[u]) continue;
                    const int sck = (tid3 + k * kThreads) * 4 + u;
                    uint32_t r = g0[u];
                    if (g1[u] - g0[u] > 1u) {                           // a key alone in its bucket has rank g0
                        const uint32_t pk = (key[k * 4 + u] << lg) | (uint32_t)sck;
#pragma unroll 1
                        for (uint32_t m = g0[u]; m < g1[u]; m++) r += gpk[m] < pk;      // (itself included: not below)
                    }
                    r += base;
                    cn[sck] = (uint16_t)(a.dc_shift >= 0 ? r >> a.dc_shift : r / (uint32_t)a.dc);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            base += total;
            __syncthreads();                                            // F: the counters may be cleared; behind the last part, the CN ids stand
        }
        if (status < 0) break;

        // ---- no VN may hold a CN twice (ldpc.py:67-84): VN t owns entries dv*t .. dv*t + dv - 1
        bool twice = false;
        for (int t = tid; t < a.vns_pos; t += kThreads) {
            const uint16_t *row = cn + t * dv;
            for (int i = 1; i < dv; i++) {
                const uint16_t ci = row[i];
                for (int j = 0; j < i; j++) twice |= row[j] == ci;
            }
        }
        if (twice) wsum[kWaves] = (uint32_t)att + 1u;                   // every writer of this attempt stores the same value
        __syncthreads();                                                // G
        if (wsum[kWaves] != (uint32_t)att + 1u) { status = att + 1; break; }    // uniform; next written behind 6 P barriers
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

extern "C" int scldpc_sample_philox_uncoupled_wide_supported(const scldpc_code_params *p)
{
    return shape("scldpc_sample_philox_uncoupled_wide_supported", p) == SCLDPC_OK;
}

extern "C" int scldpc_sample_philox_uncoupled_wide_device(const scldpc_code_params *p, uint64_t seed, uint64_t trial0, int32_t ntrials,
                                                          double eps, int32_t max_attempts, int32_t *d_vn_adj, uint32_t *d_chan_bits,
                                                          int32_t *d_attempts, void *stream)
{
    const char *who = "scldpc_sample_philox_uncoupled_wide_device";
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

    WArgs a{};
    a.dv = p->dv; a.dc = p->dc; a.vns_pos = p->vns_pos; a.S = p->cns_pos * p->dc; a.nw = scldpc::nw_of(p);
    const bool parts = a.S > kOnePartSockets;
    a.lg = 12;                                      // buckets = power of two >= max(S, 4096): an instance's thread scans WPT words
    while ((1 << a.lg) < a.S) a.lg++;
    a.nbp = (1 << a.lg) >> (parts ? 2 : 0);
    a.dc_shift = -1;
    for (int k = 0; k < 16; k++) if ((1 << k) == p->dc) a.dc_shift = k;
    a.max_attempts = max_attempts;
    const int cap = parts ? kPartCap : (a.S + 3) & ~3;          // P = 1: the one part holds every key
    a.part_cap = (uint32_t)cap;
    if (const char *v = getenv("SCLDPC_DEBUG_UNCOUPLED_WIDE_PART_CAP"))      // diagnostics / tests only
        a.part_cap = (uint32_t)std::min(cap, std::max(0, atoi(v)));
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.trial0 = trial0;
    a.thresh = scldpc::erasure_threshold(eps);
    int off = a.nbp / 2;
    a.off_gpk = off; off += cap;
    a.off_cn = off; off += ((a.S + 1) / 2 + 3) & ~3;
    a.off_wsum = off; off += 32;
    const size_t lds_bytes = 4u * (size_t)off;     // 128 KiB + 128 B at 16 384 and at 32 768 sockets
    if (lds_bytes > (size_t)scldpc::kMaxLdsBytes)
        return scldpc::set_error(SCLDPC_ERR_TOO_LARGE, "%s: %zu bytes of LDS per trial", who, lds_bytes);
    a.vn_adj = d_vn_adj; a.chan = d_chan_bits; a.attempts = d_attempts;

    const int kmax = ((a.S + 3) / 4 + kThreads - 1) / kThreads;     // 1 .. 8
    void (*kern)(const WArgs) = parts ? sample_uncoupled_wide_kernel<8, 2, 4>            // 8192 buckets per part
                              : kmax == 1 ? sample_uncoupled_wide_kernel<1, 0, 2>        // 4096 buckets
                              : kmax == 2 ? sample_uncoupled_wide_kernel<2, 0, 4>        // 8192
                                          : sample_uncoupled_wide_kernel<4, 0, 8>;       // 16 384
    if (int rc = scldpc::allow_max_lds(reinterpret_cast<const void *>(kern))) return rc;
    hipLaunchKernelGGL(kern, dim3(ntrials), dim3(kThreads), lds_bytes, static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}
