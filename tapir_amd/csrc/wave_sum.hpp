// wave_sum.hpp -- the sum of a double over the 64 lanes of a wave by a butterfly: a fixed shape, every lane ends with the same
// bits.  Shared by every kernel header that adds over a wave.
#pragma once
#include <hip/hip_runtime.h>

namespace tphip {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace tphip
