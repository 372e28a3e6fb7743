// philox4x32.hpp -- the site bootstrap's counter-based generator.  Plain C++ when it is not compiled
// by hipcc, so that a host program (tests/native/philox_kat.cpp) pins the very code the draw kernel runs.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TPHIP_PHILOX_FN __host__ __device__ __forceinline__
#else
#define TPHIP_PHILOX_FN inline
#endif

namespace tphip {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011), the constants of the paper.  ctr is replaced by the output words.
TPHIP_PHILOX_FN void philox4x32_10(uint32_t* ctr, uint32_t k0, uint32_t k1) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    ctr[0] = c0; ctr[1] = c1; ctr[2] = c2; ctr[3] = c3;
}

// high 64 bits of a 64 x 64-bit product
TPHIP_PHILOX_FN uint64_t mul_hi_u64(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

// Philox call j of replicate b of the locus with stream id `id` and n columns: draws 2j and 2j + 1 (the caller discards the
// second one when 2j + 1 == n).  key = (seed & 0xffffffff, seed >> 32), counter = (j, b, id & 0xffffffff, id >> 32);
// draw 2j = ((x1 2^32 + x0) n) >> 64, draw 2j + 1 the same from (x3, x2).
TPHIP_PHILOX_FN void bootstrap_draw_pair(uint64_t seed, uint64_t id, uint32_t b, uint32_t j, uint64_t n, uint64_t* d0, uint64_t* d1) {
    uint32_t x[4] = {j, b, (uint32_t)id, (uint32_t)(id >> 32)};
    philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
    *d0 = mul_hi_u64(((uint64_t)x[1] << 32) | x[0], n);
    *d1 = mul_hi_u64(((uint64_t)x[3] << 32) | x[2], n);
}

}  // namespace tphip
