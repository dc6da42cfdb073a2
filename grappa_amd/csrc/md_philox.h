// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011; the constants of Random123), one
// function for the device (csrc/dynamics.hip) and the host (grappa_md_philox): counter-based, so a stream has no state -- the four
// output words are a function of the 64-bit key and the 128-bit counter alone.  Plain C++: a host-only program may include this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GRAPPA_PHILOX_FN __host__ __device__ inline
#else
#define GRAPPA_PHILOX_FN inline
#endif

// key = (k0, k1) = (low, high half of the 64-bit key), counter = (c0, c1, c2, c3) -> out[0..3]
GRAPPA_PHILOX_FN void grappa_philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;          // (the key schedule: bumped after every round; the bump after the last one is unused)
        k1 += W1;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
