// Host check of csrc/philox.h's split form (built and run by tests/test_philox_split_host.py): philox_prefix +
// philox_uniform + philox_tail must equal philox4x32_10 on the Random123 known-answer vectors and on random
// (counter, key) pairs, with the counter values the C2 sampler uses mixed in.  Prints "ok <pairs>" or the first mismatch.
#include "philox.h"

#include <cstdio>
#include <cstdlib>

using namespace scldpc_dev;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t splitmix64()
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bool same(const uint32_t (&c)[4], const uint32_t (&k)[2], const uint32_t *want)
{
    uint32_t full[4], split[4];
    philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1], full);
    const PhiloxPrefix f = philox_prefix(c[0], c[2], c[3], k[0], k[1]);
    const PhiloxUniform g = philox_uniform(c[1], c[2], k[0], k[1]);
    philox_tail(f, g, k[0], k[1], split);
    bool ok = true;
    for (int i = 0; i < 4; i++) ok = ok && full[i] == split[i] && (!want || full[i] == want[i]);
    if (!ok) {
        printf("mismatch: ctr %08x %08x %08x %08x key %08x %08x\n  full  %08x %08x %08x %08x\n  split %08x %08x %08x %08x\n",
               c[0], c[1], c[2], c[3], k[0], k[1], full[0], full[1], full[2], full[3], split[0], split[1], split[2], split[3]);
        if (want) printf("  want  %08x %08x %08x %08x\n", want[0], want[1], want[2], want[3]);
    }
    return ok;
}

int main(int argc, char **argv)
{
    const long pairs = argc > 1 ? atol(argv[1]) : 100000;
    static const struct { uint32_t c[4], k[2], out[4]; } kat[] = {      // Random123 kat_vectors, philox4x32-10
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
         {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
         {0xd16cfe09u, 0x94fdcceb, 0x5001e420u, 0x24126ea1u}},
    };
    for (const auto &v : kat)
        if (!same(v.c, v.k, v.out)) return 1;
    for (long i = 0; i < pairs; i++) {
        const uint64_t a = splitmix64(), b = splitmix64(), k = splitmix64();
        uint32_t c[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
        uint32_t key[2] = {(uint32_t)k, (uint32_t)(k >> 32)};
        // the sampler's counters: c0 = thread (below and from 1024 on), c1 = 0 (first position), a small position, or
        // 0x80000000 (channel), c2 | c3 = trial index around the 32-bit boundary, a seed with a zero high half
        switch (i & 7) {
        case 1: c[0] &= 1023u; c[1] = 0u; break;
        case 2: c[0] = 1024u + (c[0] & 1023u); c[1] &= 63u; c[3] = 0u; break;
        case 3: c[1] = 0x80000000u; c[3] &= 0xFFu; break;
        case 4: c[2] = 0xFFFFFFFFu; c[0] &= 2047u; c[1] &= 63u; break;
        case 5: c[2] = 0u; c[3] = (c[3] & 0xFFu) + 1u; key[1] = 0u; break;
        case 6: c[0] = 1024u + (c[0] & 1023u); c[1] = 0x80000000u; c[2] = 0xFFFFFFFFu; break;
        default: break;
        }
        if (!same(c, key, nullptr)) return 1;
    }
    printf("ok %ld\n", pairs);
    return 0;
}
