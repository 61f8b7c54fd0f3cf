// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) — the one
// counter-based generator of the throughput-mode samplers (sampler*.hip, stream_bp.hip, peel_pick.hip).  Not reference
// arithmetic: the reference draws from one sequential glibc / MT19937 stream (glibc_sampler.cpp replays that exactly);
// its known-answer vectors are tested (tests/test_abi.py) and every device sampler has a CPU twin in oracle/.
// The header also compiles for the host (plain C++, no HIP): tests/test_philox_split_host.py builds it into a program.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCLDPC_PHILOX_HD __host__ __device__ __forceinline__
#else
#define SCLDPC_PHILOX_HD inline
#endif

namespace scldpc_dev {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;    // the round's two multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;    // what a round adds to the two key words

// a ^ b ^ c: gfx950's v_bitop3_b32 (truth table 0x96) on the device, one instruction instead of two
SCLDPC_PHILOX_HD uint32_t philox_xor3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// The round's two 32x32 -> 64 products are written as 64-bit multiplies: hipcc then emits ONE v_mad_u64_u32 per
// product instead of a v_mul_hi_u32 + v_mul_lo_u32 pair (18 instead of 36 quarter-rate multiplies per call), and the
// three-way XORs are gfx950's v_bitop3_b32 (truth table 0x96), one instruction instead of two.
SCLDPC_PHILOX_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                    uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        c0 = philox_xor3((uint32_t)(p1 >> 32), c1, k0); c1 = (uint32_t)p1;
        c2 = philox_xor3((uint32_t)(p0 >> 32), c3, k1); c3 = (uint32_t)p0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- The same function split by what its first rounds depend on, for a caller that draws philox4x32_10(c0, c1, c2,
// c3, k) for many c1 with c0, c2, c3 and the key fixed (the C2 sampler: c0 = thread, c1 = CN position, c2 | c3 = trial).
// Rounds 1 and 2 mix c1 into two words only, and through products of values that do not depend on c0:
//   round 1:  c0' = hi(M1 c2) ^ c1 ^ k0      — c1 and uniform values      c1' = lo(M1 c2)     — uniform, no c1
//             c2' = hi(M0 c0) ^ c3 ^ k1      — no c1                      c3' = lo(M0 c0)     — no c1
//   round 2:  c0" = hi(M1 c2') ^ c1' ^ k0'   — no c1                      c1" = lo(M1 c2')    — no c1
//             c2" = hi(M0 c0') ^ c3' ^ k1'   = U ^ c3'                    c3" = lo(M0 c0')    — c1 and uniform values
//   round 3:  M0 c0" has no c1; M1 c2" is the first product that depends on both c0 and c1.
// philox_prefix holds the four c1-free words a thread needs (three products, once per c0 / c2 / c3 / key),
// philox_uniform the two words made of c1, c2 and the key alone (uniform across the threads of a workgroup: its three
// products run on the scalar unit), and philox_tail finishes round 3 and runs rounds 4 - 10: 15 products instead of 20.
struct PhiloxPrefix {
    uint32_t c3r1;                      // round 1's c3' = lo(M0 c0)
    uint32_t a;                         // round 2's c1" ^ round 3's k0
    uint32_t b, c;                      // hi, lo of round 3's M0 c0"
};
struct PhiloxUniform {
    uint32_t u;                         // hi(M0 c0') ^ round 2's k1:   c2" = u ^ c3'
    uint32_t v;                         // lo(M0 c0') ^ round 3's k1:   round 3's c2 = b ^ v
};

SCLDPC_PHILOX_HD PhiloxPrefix philox_prefix(uint32_t c0, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0;
    const uint32_t c1r1 = (uint32_t)((uint64_t)kPhiloxM1 * c2);
    const uint32_t c2r1 = philox_xor3((uint32_t)(p0 >> 32), c3, k1);
    const uint64_t p1 = (uint64_t)kPhiloxM1 * c2r1;
    const uint32_t c0r2 = philox_xor3((uint32_t)(p1 >> 32), c1r1, k0 + kPhiloxW0);
    const uint64_t q0 = (uint64_t)kPhiloxM0 * c0r2;
    PhiloxPrefix f;
    f.c3r1 = (uint32_t)p0;
    f.a = (uint32_t)p1 ^ (k0 + 2u * kPhiloxW0);
    f.b = (uint32_t)(q0 >> 32);
    f.c = (uint32_t)q0;
    return f;
}

SCLDPC_PHILOX_HD PhiloxUniform philox_uniform(uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1)
{
    const uint32_t c0r1 = (uint32_t)(((uint64_t)kPhiloxM1 * c2) >> 32) ^ c1 ^ k0;
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0r1;
    PhiloxUniform g;
    g.u = (uint32_t)(p0 >> 32) ^ (k1 + kPhiloxW1);
    g.v = (uint32_t)p0 ^ (k1 + 2u * kPhiloxW1);
    return g;
}

SCLDPC_PHILOX_HD void philox_tail(const PhiloxPrefix &f, const PhiloxUniform &g, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
    const uint64_t q1 = (uint64_t)kPhiloxM1 * (g.u ^ f.c3r1);            // round 3's M1 c2"
    uint32_t c0 = (uint32_t)(q1 >> 32) ^ f.a, c1 = (uint32_t)q1, c2 = f.b ^ g.v, c3 = f.c;
    k0 += 3u * kPhiloxW0; k1 += 3u * kPhiloxW1;
#pragma unroll
    for (int r = 3; r < 10; r++) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        c0 = philox_xor3((uint32_t)(p1 >> 32), c1, k0); c1 = (uint32_t)p1;
        c2 = philox_xor3((uint32_t)(p0 >> 32), c3, k1); c3 = (uint32_t)p0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace scldpc_dev
