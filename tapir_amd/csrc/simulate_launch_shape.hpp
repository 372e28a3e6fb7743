// simulate_launch_shape.hpp -- how simulate_columns_kernel (simulate_kernels.hpp) is launched for a tree, decided on the
// host alone: no HIP header, so tests/native/sim_launch_dump.cpp compiles it with g++ (tests/test_sim_launch.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace tphip {

constexpr int kSimMaxBlock = 256;
constexpr int kSimMinBlock = 64;
constexpr size_t kSimLdsBytes = 160 * 1024;
constexpr size_t kSimLdsDefaultBytes = 48 * 1024;   // a launch with more dynamic LDS needs hipFuncSetAttribute first

// dynamic LDS of a launch: one packed word of 16 2-bit states per 16 internal nodes and thread
inline size_t sim_lds_bytes(int32_t words, int32_t block) { return (size_t)words * (size_t)block * sizeof(uint32_t); }

// words = ceil(nint / 16); block = the largest of 256, 128, 64 whose words fit the LDS.  false: not even 64 columns fit.
inline bool sim_launch_shape(int32_t nint, int32_t* words, int32_t* block) {
    const int32_t w = (nint + 15) / 16;
    int32_t b = kSimMaxBlock;
    while (b > kSimMinBlock && sim_lds_bytes(w, b) > kSimLdsBytes) b >>= 1;
    *words = w;
    *block = b;
    return sim_lds_bytes(w, b) <= kSimLdsBytes;
}

}  // namespace tphip
