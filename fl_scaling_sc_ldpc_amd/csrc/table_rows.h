// Rows of the 2-byte tables (VN -> CN, CN -> VN / CN -> socket) as the 4-bit decoders keep them in registers: shared by
// full_bp_small.hip and sw_ring.hip (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace scldpc_dev {

// A table row as it is kept in registers: its 16-bit entries two to a word.
template <int D>
struct Row {
    uint32_t w[(D + 1) / 2];
    __device__ __forceinline__ uint32_t operator[](int i) const { return (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; }
};
// Loads no wider than the alignment the layout guarantees: the unit in which a trial's table is addressed (one load each) and
// how many of them make a row — a whole row where its size is a power of two, else uint16 (VN rows) or uint32 (CN rows).
template <int D> struct VnUnit { using type = uint16_t; static constexpr int per_row = D; };
template <> struct VnUnit<4> { using type = uint2; static constexpr int per_row = 1; };
template <int D> struct CnUnit { using type = uint32_t; static constexpr int per_row = D / 2; };
template <> struct CnUnit<8> { using type = uint4; static constexpr int per_row = 1; };

__device__ __forceinline__ Row<4> load_row(const uint2 *rows, int j)
{
    const uint2 v = rows[j];
    return {{v.x, v.y}};
}
__device__ __forceinline__ Row<8> load_row(const uint4 *rows, int c)
{
    const uint4 v = rows[c];
    return {{v.x, v.y, v.z, v.w}};
}
template <int DV>
__device__ __forceinline__ Row<DV> load_row(const uint16_t *rows, int j)
{
    Row<DV> r;
    const uint16_t *h = rows + (size_t)j * DV;
#pragma unroll
    for (int i = 0; i < DV; i += 2) r.w[i >> 1] = (uint32_t)h[i] | (i + 1 < DV ? (uint32_t)h[i + 1] << 16 : 0u);
    return r;
}
template <int DC>
__device__ __forceinline__ Row<DC> load_row(const uint32_t *rows, int c)
{
    Row<DC> r;
    const uint32_t *h = rows + (size_t)c * (DC / 2);
#pragma unroll
    for (int i = 0; i < DC / 2; i++) r.w[i] = h[i];
    return r;
}

}  // namespace scldpc_dev
