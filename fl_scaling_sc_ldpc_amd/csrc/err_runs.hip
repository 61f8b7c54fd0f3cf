// Error-propagation statistics of the window decoders (include/scldpc_runs.h): where a chain's failed positions sit and how
// long their runs are, from the decoders' erased bits; runs, events, gaps and the time to first failure of the streaming
// decoder, from its trace rows.  Integer sums only; every bin is collected in LDS and leaves a workgroup once, as a 64-bit
// integer atomic, and only where it is not zero.
//
// chain_runs_kernel — persistent 256-thread workgroups, each striding over trials.  Per trial, three phases with a barrier
// after each:
//   count   a wave takes a position u: its lanes load the words covering bits [uV, (u+1)V) (consecutive words, one per lane),
//           mask the first and the last word, popcount, and the wave's sum goes to e[u] in LDS.  A wave issues the loads of
//           eight positions before it reduces the first, and those of the NEXT trial's first 32 positions before the
//           barrier, so that they are in flight under the two phases below.  No atomics.
//   flags   f[u] = e[u] > 0 by __ballot, one 64-bit mask per 64 positions, into LDS.
//   runs    thread c owns position c (+ 256 k): it adds f and e to its own bins (no atomics), and where a run starts at c it
//           measures the run over the masks and adds to the run histogram (LDS atomics: several runs may share a length).
//           Thread 0 adds what belongs to the trial as a whole.
// stream_runs_kernel — one wave per stream, four to a workgroup.  64 rows per step; x, doped and "decides a position" become
// three ballots and the state machine of the header walks the masks.  A step without a failing position and with nothing
// open is two additions.
#include "common.h"
#include "kernel_util.h"
#include "../../include/scldpc_runs.h"

namespace {
using scldpc_dev::wave_sum;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kMaxGrid = 4096;                  // persistent workgroups: as many as are resident at once, at most this (the sums do not depend on it)
constexpr int kFlushTrials = 1 << 22;           // a workgroup flushes its 32-bit bins after this many trials (<= 513 runs each)
constexpr int kInFlight = 8;                    // positions a wave has loads in flight for (more cost registers, and with them resident waves)
enum { S_RUNS, S_LONGEST, kScalars = 4 };

struct ChainArgs {
    int L, V, nw, ntrials, fw;                  // fw = words of d_fail_bits per trial
    const uint32_t *bits;
    unsigned long long *pos, *run_hist, *fail_hist;
    int32_t *trial;
    uint32_t *fail_bits;
};

struct ChainLds {                               // carved from dynamic LDS, the 64-bit arrays first
    unsigned long long *esum, *masks;
    int *e, *scal;
    uint32_t *fails, *first, *starts, *rh, *fh;
};

__device__ __forceinline__ ChainLds chain_carve(unsigned long long *base, int L)
{
    ChainLds s;
    s.esum = base;
    s.masks = s.esum + L;
    s.e = reinterpret_cast<int *>(s.masks + (SCLDPC_RUNS_MAX_L / 64));
    s.scal = s.e + L;
    s.fails = reinterpret_cast<uint32_t *>(s.scal + kScalars);
    s.first = s.fails + L;
    s.starts = s.first + L;
    s.rh = s.starts + L;
    s.fh = s.rh + 2 * (L + 1);
    return s;
}

size_t chain_lds_bytes(int L)
{
    return 8u * ((size_t)L + SCLDPC_RUNS_MAX_L / 64) + 4u * ((size_t)L + kScalars + 3u * L + 3u * ((size_t)L + 1));
}

// Position u covers bits [uV, (u+1)V): words w0 .. w1 of the trial's row (w1 <= nw - 1, as (u+1)V <= n <= 2^30).  A lane
// takes word w0 + lane (and the words 64, 128, … further on where a position has more than 64 words: tails()).
struct Span { int b0, b1, w0, w1; };
__device__ __forceinline__ Span span_of(int u, int V)
{
    Span s;
    s.b0 = u * V; s.b1 = s.b0 + V;
    s.w0 = s.b0 >> 5; s.w1 = (s.b1 - 1) >> 5;
    return s;
}
__device__ __forceinline__ uint32_t span_mask(const Span &s, int w, uint32_t x)
{
    if (w == s.w0) x &= ~0u << (s.b0 & 31);
    if (w == s.w1 && (s.b1 & 31)) x &= (1u << (s.b1 & 31)) - 1u;
    return x;
}

__device__ void chain_flush(const ChainArgs &a, const ChainLds &s)
{
    const int tid = threadIdx.x, L = a.L;
    __syncthreads();
    for (int u = tid; u < L; u += kBlock) {
        if (const uint32_t v = s.fails[u]) { atomicAdd(&a.pos[4 * u + 0], (unsigned long long)v); s.fails[u] = 0; }
        if (const unsigned long long v = s.esum[u]) { atomicAdd(&a.pos[4 * u + 1], v); s.esum[u] = 0; }
        if (const uint32_t v = s.first[u]) { atomicAdd(&a.pos[4 * u + 2], (unsigned long long)v); s.first[u] = 0; }
        if (const uint32_t v = s.starts[u]) { atomicAdd(&a.pos[4 * u + 3], (unsigned long long)v); s.starts[u] = 0; }
    }
    for (int i = tid; i < 2 * (L + 1); i += kBlock)
        if (const uint32_t v = s.rh[i]) { atomicAdd(&a.run_hist[i], (unsigned long long)v); s.rh[i] = 0; }
    for (int i = tid; i <= L; i += kBlock)
        if (const uint32_t v = s.fh[i]) { atomicAdd(&a.fail_hist[i], (unsigned long long)v); s.fh[i] = 0; }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void chain_runs_kernel(const ChainArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long runs_lds[];
    const ChainLds s = chain_carve(runs_lds, a.L);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: a position's bounds cost no vector registers
    const int L = a.L, V = a.V, nmasks = (L + 63) >> 6;

    for (int u = tid; u < L; u += kBlock) { s.esum[u] = 0; s.fails[u] = 0; s.first[u] = 0; s.starts[u] = 0; }
    for (int i = tid; i < 2 * (L + 1); i += kBlock) s.rh[i] = 0;
    for (int i = tid; i <= L; i += kBlock) s.fh[i] = 0;
    if (tid < kScalars) s.scal[tid] = 0;
    __syncthreads();

    // the loads of kInFlight positions u0, u0 + kWaves, …, back to back
    auto issue = [&](const uint32_t *row, int u0, uint32_t (&x)[kInFlight]) {
#pragma unroll
        for (int k = 0; k < kInFlight; k++) {
            const int u = u0 + k * kWaves;
            const Span sp = span_of(u < L ? u : 0, V);
            x[k] = row[(uint32_t)min(sp.w0 + lane, sp.w1)];             // always a word of the row; reduce() drops what lies beyond
        }
    };
    auto reduce = [&](int u0, const uint32_t (&x)[kInFlight]) {
#pragma unroll
        for (int k = 0; k < kInFlight; k++) {
            const int u = u0 + k * kWaves;
            const Span sp = span_of(u < L ? u : 0, V);
            const int w = sp.w0 + lane;
            const int e = wave_sum(w <= sp.w1 ? __popc(span_mask(sp, w, x[k])) : 0);
            if (lane == 0 && u < L) s.e[u] = e;
        }
    };
    // positions of more than 64 words (V > 2017 at the earliest): the words beyond a lane's first, added by the wave that owns u
    const bool long_positions = ((V + 30) >> 5) + 1 > 64;
    auto tails = [&](const uint32_t *row) {
        for (int u = wave; u < L; u += kWaves) {
            const Span sp = span_of(u, V);
            int c = 0;
            for (int w = sp.w0 + lane + 64; w <= sp.w1; w += 64) c += __popc(span_mask(sp, w, row[w]));
            c = wave_sum(c);
            if (lane == 0) s.e[u] += c;
        }
    };

    int done = 0;
    uint32_t x[kInFlight];                      // the first kWaves * kInFlight = 32 positions of the trial at hand, loaded a trial ahead
    if ((int)blockIdx.x < a.ntrials) issue(a.bits + (size_t)blockIdx.x * a.nw, wave, x);
    for (int t = blockIdx.x; t < a.ntrials; t += gridDim.x) {
        const uint32_t *row = a.bits + (size_t)t * a.nw;
        // ---- count
        reduce(wave, x);
        for (int u0 = wave + kWaves * kInFlight; u0 < L; u0 += kWaves * kInFlight) {
            uint32_t y[kInFlight];
            issue(row, u0, y);
            reduce(u0, y);
        }
        if (long_positions) tails(row);
        if (t + (int)gridDim.x < a.ntrials)     // the next trial's loads fly while this one's flags and runs are formed
            issue(a.bits + (size_t)(t + (int)gridDim.x) * a.nw, wave, x);
        __syncthreads();
        // ---- flags
        for (int k = wave; k < nmasks; k += kWaves) {
            const int u = 64 * k + lane;
            const unsigned long long m = __ballot(u < L && s.e[u] > 0);
            if (lane == 0) s.masks[k] = m;
        }
        __syncthreads();
        // ---- runs
        auto flag = [&](int u) { return (int)((s.masks[u >> 6] >> (u & 63)) & 1ull); };
        for (int u = tid; u < L; u += kBlock) {
            if (!flag(u)) continue;
            s.fails[u] += 1;
            s.esum[u] += (unsigned long long)s.e[u];
            if (u > 0 && flag(u - 1)) continue;
            s.starts[u] += 1;
            int len = 0;                        // ones from u on: the rest of u's mask, then whole masks
            for (int v = u; v < L;) {
                const unsigned long long rest = ~(s.masks[v >> 6] >> (v & 63));      // its zeros; bits shifted in count as zeros of the mask
                const int room = 64 - (v & 63);
                const int ones = rest ? __ffsll((long long)rest) - 1 : 64;
                if (ones < room) { len += ones; break; }
                len += room;
                v += room;
            }
            atomicAdd(&s.rh[2 * len], 1u);
            if (u + len == L) atomicAdd(&s.rh[2 * len + 1], 1u);
            atomicAdd(&s.scal[S_RUNS], 1);
            atomicMax(&s.scal[S_LONGEST], len);
        }
        if (a.fail_bits && tid < a.fw)
            a.fail_bits[(size_t)t * a.fw + tid] = (uint32_t)(s.masks[tid >> 1] >> (32 * (tid & 1)));
        int nfail = 0, first = L;
        if (tid == 0) {
            for (int k = nmasks - 1; k >= 0; k--) {
                const unsigned long long m = s.masks[k];
                nfail += __popcll(m);
                if (m) first = 64 * k + __ffsll((long long)m) - 1;
            }
            if (nfail == 0) s.rh[0] += 1;       // bin [0][0] is thread 0's alone: no run has length 0
            else s.first[first] += 1;           // and so is this table
            s.fh[nfail] += 1;
        }
        __syncthreads();
        if (tid == 0) {
            if (a.trial)
                *reinterpret_cast<int4 *>(a.trial + (size_t)t * 4) = make_int4(nfail, first, s.scal[S_RUNS], s.scal[S_LONGEST]);
            s.scal[S_RUNS] = 0;                 // the next trial's atomics come two barriers later
            s.scal[S_LONGEST] = 0;
        }
        if (++done == kFlushTrials) { chain_flush(a, s); done = 0; }
    }
    chain_flush(a, s);
}

// ================================================== stream ==================================================================
struct StreamArgs {
    int ms, nstreams, npos, nbins, ndoped, doped[SCLDPC_RUNS_MAX_DOPED];
    long long period;                           // without d_phase it may pass 2^31 - 1
    const int32_t *trace;
    const long long *counters;
    long long *carry;
    unsigned long long *hist, *sums, *phase;
};

size_t stream_lds_bytes(int nbins, int phase_rows)
{
    return 8u * (8u + (size_t)phase_rows) + 4u * (4u * (size_t)nbins + 2u * (size_t)phase_rows);
}

__device__ __forceinline__ bool phase_is_doped(const StreamArgs &a, int m)          // position_is_doped on m = d % period
{
    for (int i = 0; i < a.ndoped; i++) if (a.doped[i] == m) return true;
    return false;
}

__device__ __forceinline__ long long wave_sum64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kBlock) void stream_runs_kernel(const StreamArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long runs_lds[];
    const int P = a.phase ? (int)a.period : 0, nbins = a.nbins;
    unsigned long long *sums = runs_lds, *ph_nep = runs_lds + 8;
    uint32_t *hist = reinterpret_cast<uint32_t *>(ph_nep + P), *ph_cnt = hist + 4 * nbins;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    if (tid < 8) sums[tid] = 0;
    for (int i = tid; i < P; i += kBlock) { ph_nep[i] = 0; ph_cnt[2 * i] = 0; ph_cnt[2 * i + 1] = 0; }
    for (int i = tid; i < 4 * nbins; i += kBlock) hist[i] = 0;
    __syncthreads();

    const int s = blockIdx.x * kWaves + wave;   // the same in every lane of a wave, and so is all that follows from it
    bool live = s < a.nstreams;
    if (live && a.counters) live = a.counters[(size_t)s * 10 + 9] >= 0;
    if (live) {
        long long *cy = a.carry + (size_t)s * SCLDPC_RUNS_CARRY;
        long long decided = cy[0], run = cy[1], event = cy[2], since = cy[3], failed = cy[4];
        const int32_t *tr = a.trace + (size_t)s * (size_t)a.npos * 10;
        auto bin = [&](int h, long long v) {
            if (lane == 0) atomicAdd(&hist[h * nbins + (int)(v < nbins - 1 ? (v < 0 ? 0 : v) : nbins - 1)], 1u);   // a carry is the caller's
        };
        auto add = [&](int i, long long v) {
            if (lane == 0) atomicAdd(&sums[i], (unsigned long long)v);
        };
        for (int k0 = 0; k0 < a.npos; k0 += 64) {
            const int k = k0 + lane;
            const bool in = k < a.npos;
            const int pos = in ? tr[(size_t)k * 10] : 0, nep = in ? tr[(size_t)k * 10 + 1] : 0;
            const bool valid = in && pos >= a.ms;
            const long long d = (long long)pos - a.ms;
            const bool x = valid && nep > 0;
            const int m = valid ? (int)(d % a.period) : 0;                  // 0 <= m < period
            const bool dop = valid && phase_is_doped(a, m);
            const unsigned long long V = __ballot(valid), X = __ballot(x), D = __ballot(dop);
            if (valid && P) {
                atomicAdd(&ph_cnt[2 * m], 1u);
                if (x) { atomicAdd(&ph_cnt[2 * m + 1], 1u); atomicAdd(&ph_nep[m], (unsigned long long)nep); }
            }
            const int first_bin = (int)(d < nbins - 1 ? (d < 0 ? 0 : d) : nbins - 1);       // clamped before any lane reads it
            const int nv = __popcll(V);
            if (nv == 0) continue;
            add(0, nv);
            if (X) {
                const long long nepsum = wave_sum64(x ? (long long)nep : 0);
                add(1, __popcll(X));
                add(2, nepsum);
            }
            if (X == 0 && run == 0 && event == 0) {                         // nothing fails, nothing is open
                decided += nv;
                since += nv;
                continue;
            }
            for (unsigned long long rem = V; rem; rem &= rem - 1) {
                const int i = __ffsll((long long)rem) - 1;
                decided += 1;
                if ((X >> i) & 1ull) {
                    if (event == 0) {
                        if (failed == 0) {
                            bin(3, __shfl(first_bin, i, 64));
                        } else {
                            bin(2, since);
                            add(7, since);
                        }
                    }
                    run += 1; event += 1; failed += 1; since = 0;
                } else {
                    if (run) { bin(0, run); add(3, 1); add(4, run); run = 0; }
                    if (event && !((D >> i) & 1ull)) { bin(1, event); add(5, 1); add(6, event); event = 0; }
                    since += 1;
                }
            }
        }
        if (lane == 0) { cy[0] = decided; cy[1] = run; cy[2] = event; cy[3] = since; cy[4] = failed; }
    }
    __syncthreads();
    if (tid < 8)
        if (const unsigned long long v = sums[tid]) atomicAdd(&a.sums[tid], v);
    for (int i = tid; i < 4 * nbins; i += kBlock)
        if (const uint32_t v = hist[i]) atomicAdd(&a.hist[i], (unsigned long long)v);
    for (int i = tid; i < P; i += kBlock) {
        if (const uint32_t v = ph_cnt[2 * i]) atomicAdd(&a.phase[3 * i + 0], (unsigned long long)v);
        if (const uint32_t v = ph_cnt[2 * i + 1]) atomicAdd(&a.phase[3 * i + 1], (unsigned long long)v);
        if (const unsigned long long v = ph_nep[i]) atomicAdd(&a.phase[3 * i + 2], v);
    }
}
}  // namespace

extern "C" int scldpc_chain_runs_device(const scldpc_code_params *p, int32_t ntrials, const uint32_t *d_bits,
                                        int64_t *d_pos, int64_t *d_run_hist, int64_t *d_fail_hist,
                                        int32_t *d_trial, uint32_t *d_fail_bits, void *stream)
{
    using namespace scldpc;
    static const char *who = "scldpc_chain_runs_device";
    if (int rc = check_params(p)) return rc;
    if (p->L > SCLDPC_RUNS_MAX_L)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: L <= %d (got L = %d)", who, SCLDPC_RUNS_MAX_L, p->L);
    if (ntrials < 0) return set_error(SCLDPC_ERR_BAD_ARG, "%s: negative ntrials", who);
    if (ntrials == 0) return SCLDPC_OK;
    if (!d_bits || !d_pos || !d_run_hist || !d_fail_hist) return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer", who);
    ChainArgs a;
    a.L = p->L; a.V = p->vns_pos; a.nw = nw_of(p); a.ntrials = ntrials; a.fw = (p->L + 31) / 32;
    a.bits = d_bits;
    a.pos = reinterpret_cast<unsigned long long *>(d_pos);
    a.run_hist = reinterpret_cast<unsigned long long *>(d_run_hist);
    a.fail_hist = reinterpret_cast<unsigned long long *>(d_fail_hist);
    a.trial = d_trial;
    a.fail_bits = d_fail_bits;
    // one round of resident workgroups: a second, partial round would leave most CUs idle while it runs
    int dev = 0, cus = 0, per_cu = 0;
    SCLDPC_HIP_CHECK(hipGetDevice(&dev));
    SCLDPC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    SCLDPC_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, chain_runs_kernel, kBlock, chain_lds_bytes(p->L)));
    int grid = cus * per_cu;
    grid = grid < 1 ? 1 : (grid > kMaxGrid ? kMaxGrid : grid);
    if (ntrials < grid) grid = ntrials;
    hipLaunchKernelGGL(chain_runs_kernel, dim3(grid), dim3(kBlock), chain_lds_bytes(p->L), static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}

extern "C" int scldpc_stream_runs_device(const scldpc_code_params *p, int32_t nstreams, int32_t npos, const int32_t *d_trace,
                                         const int64_t *d_counters, int32_t ndoped, const int32_t *doped_positions,
                                         int32_t nbins, int64_t *d_carry, int64_t *d_hist, int64_t *d_sums,
                                         int64_t *d_phase, void *stream)
{
    using namespace scldpc;
    static const char *who = "scldpc_stream_runs_device";
    if (int rc = check_params(p)) return rc;
    if (nstreams < 0 || npos < 0) return set_error(SCLDPC_ERR_BAD_ARG, "%s: negative nstreams or npos", who);
    if (npos > SCLDPC_RUNS_MAX_NPOS)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: npos <= %d rows per stream and call (got %d): split the call, the sums do not "
                         "depend on the split", who, SCLDPC_RUNS_MAX_NPOS, npos);
    if (ndoped < 0 || ndoped > SCLDPC_RUNS_MAX_DOPED || (ndoped > 0 && !doped_positions))
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 0 <= ndoped <= %d, with its positions", who, SCLDPC_RUNS_MAX_DOPED);
    StreamArgs a;
    a.ndoped = ndoped;
    for (int d = 0; d < ndoped; d++) {
        if (doped_positions[d] < 0 || (d > 0 && doped_positions[d] <= doped_positions[d - 1]))
            return set_error(SCLDPC_ERR_BAD_ARG, "%s: doped positions must be non-negative and ascending (BPF:1585-1587)", who);
        a.doped[d] = doped_positions[d];
    }
    if (nbins < 2 || nbins > SCLDPC_RUNS_MAX_BINS)
        return set_error(SCLDPC_ERR_BAD_ARG, "%s: 2 <= nbins <= %d (got nbins = %d)", who, SCLDPC_RUNS_MAX_BINS, nbins);
    const int64_t period = ndoped ? (int64_t)doped_positions[ndoped - 1] + 1 : 1;
    if (d_phase && period > SCLDPC_RUNS_MAX_PERIOD)
        return set_error(SCLDPC_ERR_TOO_LARGE, "%s: d_phase takes a doping period <= %d (got %lld)", who, SCLDPC_RUNS_MAX_PERIOD,
                         (long long)period);
    if (nstreams == 0 || npos == 0) return SCLDPC_OK;
    if (!d_trace || !d_carry || !d_hist || !d_sums) return set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer", who);
    a.ms = p->dv - 1; a.nstreams = nstreams; a.npos = npos; a.nbins = nbins; a.period = period;
    a.trace = d_trace;
    a.counters = reinterpret_cast<const long long *>(d_counters);
    a.carry = reinterpret_cast<long long *>(d_carry);
    a.hist = reinterpret_cast<unsigned long long *>(d_hist);
    a.sums = reinterpret_cast<unsigned long long *>(d_sums);
    a.phase = reinterpret_cast<unsigned long long *>(d_phase);
    if (int rc = allow_max_lds(reinterpret_cast<const void *>(stream_runs_kernel))) return rc;
    hipLaunchKernelGGL(stream_runs_kernel, dim3((nstreams + kWaves - 1) / kWaves), dim3(kBlock),
                       stream_lds_bytes(nbins, d_phase ? (int)period : 0), static_cast<hipStream_t>(stream), a);
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}
