// Integer Gram matrices of a batch of degree-1 trajectories at K chosen steps — the device half of the covariance workflow
// (include/scldpc_cov.h).  With x[t][i] = r1[t][steps[i]] and m[t][i] = (x[t][i] != 0), over the trials of the batch,
//     gram[0][i][j] += Σ_t m[t][i]·m[t][j],   gram[1][i][j] += Σ_t x[t][i]·m[t][j],   gram[2][i][j] += Σ_t x[t][i]·x[t][j]
// in 64-bit integers, accumulated in place.  No floating point and no MFMA: the sums are exact at any size.
//
// Two kernels.  r1_gather_kernel copies the K columns into a dense int32 [Tpad][Kpad] panel in the caller's workspace, zero
// beyond trial T and column K (a zero adds nothing to any of the three sums), so that the Gram kernel loads whole 16-byte
// pieces without a bounds test; a step outside [0, ncols) is clamped and flagged in the workspace's status word.
// r1_gram_kernel: one workgroup of 256 threads per 64 x 64 tile of the output and per share of the trials (grid.z); it walks
// its trials in chunks of 32 staged in LDS (two panels of 8 KiB, the next chunk's global loads in flight under the current
// chunk's arithmetic); a thread keeps a 4 x 4 register tile of the three sums and adds it to gram with 64-bit integer atomics —
// integer addition, so the order does not matter.  Per trial and pair: one 32 x 32 + 64-bit multiply-add (gram[2]) and one
// select + 64-bit add (gram[1]); the rows hold counts and are read as unsigned 32-bit values.  The pair counts (gram[0]) cost
// nothing per pair and trial: a thread shifts the "non-zero" bit of each of its eight columns into a 32-bit mask per chunk,
// and a pair's count is the popcount of two masks, once per chunk.
// The column panel is stored permuted, LDS slot 4 * (c % 16) + c / 16 for column c, so that a thread's four columns are
// tx, tx + 16, tx + 32, tx + 48: one 16-byte LDS read per step, and sixteen neighbouring lanes of an atomic touch 128
// contiguous bytes of a row of gram.
#include "common.h"
#include "../../include/scldpc_cov.h"

namespace {
constexpr int kTile = 64;           // edge of an output tile; Kpad is a multiple of it
constexpr int kChunk = 32;          // trials per LDS stage; Tpad is a multiple of it
constexpr int kStatusBytes = 256;   // the status word's slot in front of the panel (keeps the panel 256-byte aligned)
constexpr int kTargetGroups = 1024; // workgroups wanted in flight: 256 CUs x 4 resident

struct Geometry {
    int64_t tpad; int kpad, tiles, nchunks, chunks_per_split, splits;
};

Geometry geometry(int32_t ntrials, int32_t k)
{
    Geometry g;
    g.tpad = ((int64_t)ntrials + kChunk - 1) / kChunk * kChunk;
    g.kpad = (k + kTile - 1) / kTile * kTile;
    g.tiles = g.kpad / kTile;
    g.nchunks = (int)(g.tpad / kChunk);
    const int ntile = g.tiles * g.tiles;
    int want = (kTargetGroups + ntile - 1) / ntile;
    if (want > g.nchunks) want = g.nchunks;
    if (want < 1) want = 1;
    g.chunks_per_split = g.nchunks ? (g.nchunks + want - 1) / want : 1;
    g.splits = g.nchunks ? (g.nchunks + g.chunks_per_split - 1) / g.chunks_per_split : 0;
    return g;
}

// block (64, 4): x = column of the panel, y = trial; rows beyond gridDim.y * 4 by a stride loop
__global__ void r1_gather_kernel(int ntrials, long long tpad, int ncols, const int32_t *r1, int k, int kpad, const int32_t *steps,
                                 int32_t *panel, int32_t *status)
{
    const int c = blockIdx.x * kTile + threadIdx.x;             // < kpad
    int s = 0;
    if (c < k) {
        s = steps[c];
        if (s < 0 || s >= ncols) {
            s = s < 0 ? 0 : ncols - 1;
            if (blockIdx.y == 0 && threadIdx.y == 0) atomicOr(status, SCLDPC_COV_STEP_CLAMPED);
        }
    }
    for (long long t = (long long)blockIdx.y * 4 + threadIdx.y; t < tpad; t += (long long)gridDim.y * 4)
        panel[(size_t)t * kpad + c] = (c < k && t < ntrials) ? r1[(size_t)t * ncols + s] : 0;
}

__global__ __launch_bounds__(256) void r1_gram_kernel(int k, int kpad, int nchunks, int chunks_per_split, const int32_t *panel,
                                                      unsigned long long *gram)
{
    __shared__ __attribute__((aligned(16))) int32_t sA[kChunk][kTile];      // rows i of the tile, in order
    __shared__ __attribute__((aligned(16))) int32_t sB[kChunk][kTile];      // columns j of the tile, permuted (see above)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int j0 = blockIdx.x * kTile, i0 = blockIdx.y * kTile;
    const int c0 = blockIdx.z * chunks_per_split;
    const int c1 = min(nchunks, c0 + chunks_per_split);

    unsigned long long g1[4][4], g2[4][4];      // the rows hold counts: read as unsigned 32-bit, products in 64 bits
    uint32_t g0[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) { g0[a][b] = 0; g1[a][b] = 0; g2[a][b] = 0; }

    // staging: thread (ty, tx) moves columns 4 tx .. 4 tx + 3 of trials ty and ty + 16 of the chunk, for both panels
    int4 ra0, ra1, rb0, rb1;
    const int32_t *src = panel + ((size_t)c0 * kChunk + ty) * kpad + 4 * tx;    // trial ty of chunk c0; trial ty + 16 below it
    const size_t half = (size_t)16 * kpad, step = (size_t)kChunk * kpad;
#define R1_GRAM_FETCH()                                                   \
    do {                                                                  \
        ra0 = *reinterpret_cast<const int4 *>(src + i0);                  \
        rb0 = *reinterpret_cast<const int4 *>(src + j0);                  \
        ra1 = *reinterpret_cast<const int4 *>(src + half + i0);           \
        rb1 = *reinterpret_cast<const int4 *>(src + half + j0);           \
        src += step;                                                      \
    } while (0)
    const int slot = 16 * (tx & 3) + (tx >> 2);                 // of column 4 tx; columns 4 tx + q sit 4 q further
    if (c0 < c1) R1_GRAM_FETCH();
    for (int c = c0; c < c1; c++) {
        __syncthreads();                                        // the previous chunk has been read
        *reinterpret_cast<int4 *>(&sA[ty][4 * tx]) = ra0;
        *reinterpret_cast<int4 *>(&sA[ty + 16][4 * tx]) = ra1;
        sB[ty][slot] = rb0.x; sB[ty][slot + 4] = rb0.y; sB[ty][slot + 8] = rb0.z; sB[ty][slot + 12] = rb0.w;
        sB[ty + 16][slot] = rb1.x; sB[ty + 16][slot + 4] = rb1.y; sB[ty + 16][slot + 8] = rb1.z; sB[ty + 16][slot + 12] = rb1.w;
        __syncthreads();
        if (c + 1 < c1) R1_GRAM_FETCH();
        // the chunk's 32 trials: per column a bitmask of its non-zero trials (the pair counts are popcounts, once per chunk)
        uint32_t bits_a[4] = {0, 0, 0, 0}, bits_b[4] = {0, 0, 0, 0};
#pragma unroll 2
        for (int t = 0; t < kChunk; t++) {
            const uint4 av = *reinterpret_cast<const uint4 *>(&sA[t][4 * ty]);
            const uint4 bv = *reinterpret_cast<const uint4 *>(&sB[t][4 * tx]);
            const uint32_t xa[4] = {av.x, av.y, av.z, av.w}, xb[4] = {bv.x, bv.y, bv.z, bv.w};
            uint32_t keep[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                bits_a[q] = (bits_a[q] << 1) | (xa[q] != 0);
                bits_b[q] = (bits_b[q] << 1) | (xb[q] != 0);
                keep[q] = xb[q] != 0 ? ~0u : 0u;
            }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    g1[a][b] += (unsigned long long)(xa[a] & keep[b]);
                    g2[a][b] += (unsigned long long)xa[a] * xb[b];
                }
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) g0[a][b] += __popc(bits_a[a] & bits_b[b]);
    }

#undef R1_GRAM_FETCH
    const size_t kk = (size_t)k * k;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + 4 * ty + a;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + tx + 16 * b;
            if (i < k && j < k) {
                unsigned long long *o = gram + (size_t)i * k + j;
                if (g0[a][b]) atomicAdd(o, (unsigned long long)g0[a][b]);
                if (g1[a][b]) atomicAdd(o + kk, g1[a][b]);
                if (g2[a][b]) atomicAdd(o + 2 * kk, g2[a][b]);
            }
        }
    }
}

// 0, or the error set: sizes the two queries and the entry share
int check_sizes(const char *who, int32_t ntrials, int32_t k)
{
    if (ntrials < 0) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: negative ntrials", who);
    if (k < 1 || k > SCLDPC_COV_MAX_STEPS)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: 1 <= k <= %d (got k = %d)", who, SCLDPC_COV_MAX_STEPS, k);
    return SCLDPC_OK;
}
}  // namespace

extern "C" int64_t scldpc_r1_gram_workspace_bytes(int32_t ntrials, int32_t k)
{
    if (check_sizes("scldpc_r1_gram_workspace_bytes", ntrials, k)) return -1;
    const Geometry g = geometry(ntrials, k);
    return kStatusBytes + 4 * g.tpad * g.kpad;
}

extern "C" int32_t scldpc_r1_gram_trial_splits(int32_t ntrials, int32_t k)
{
    if (check_sizes("scldpc_r1_gram_trial_splits", ntrials, k)) return -1;
    return geometry(ntrials, k).splits;
}

extern "C" int scldpc_r1_gram_device(int32_t ntrials, int32_t ncols, const int32_t *d_r1, int32_t k, const int32_t *d_steps,
                                     int64_t *d_gram, void *d_ws, int64_t ws_bytes, void *stream)
{
    static const char *who = "scldpc_r1_gram_device";
    if (const int rc = check_sizes(who, ntrials, k)) return rc;
    if (ncols < 0) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: negative ncols", who);
    if (ntrials == 0) return SCLDPC_OK;
    if (ncols == 0) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: ncols = 0 holds no step", who);
    if (!d_r1 || !d_steps || !d_gram || !d_ws) return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: null buffer", who);
    if (reinterpret_cast<uintptr_t>(d_ws) & 15)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: workspace not 16-byte aligned", who);
    const Geometry g = geometry(ntrials, k);
    const int64_t need = kStatusBytes + 4 * g.tpad * g.kpad;
    if (ws_bytes < need)
        return scldpc::set_error(SCLDPC_ERR_BAD_ARG, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                                 (long long)need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *status = static_cast<int32_t *>(d_ws);
    int32_t *panel = reinterpret_cast<int32_t *>(static_cast<char *>(d_ws) + kStatusBytes);
    SCLDPC_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    const int64_t row_groups = g.tpad / 4;
    hipLaunchKernelGGL(r1_gather_kernel, dim3(g.tiles, (unsigned)(row_groups < 16384 ? row_groups : 16384)), dim3(kTile, 4), 0, st,
                       ntrials, (long long)g.tpad, ncols, d_r1, k, g.kpad, d_steps, panel, status);
    SCLDPC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r1_gram_kernel, dim3(g.tiles, g.tiles, g.splits), dim3(256), 0, st, k, g.kpad, g.nchunks,
                       g.chunks_per_split, panel, reinterpret_cast<unsigned long long *>(d_gram));
    SCLDPC_HIP_CHECK(hipGetLastError());
    return SCLDPC_OK;
}
