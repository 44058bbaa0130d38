// A workgroup's exclusive scan, for the body coders' offset kernels (tga.hip,
// hdr.hip, iris.hip, webp.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rr {

// Exclusive scan of one value a thread over a workgroup of WAVES whole waves of
// 64 lanes; returns the total. Every thread of the workgroup calls it.
// lds_waves: WAVES words of LDS, free again when the call returns.
template <int WAVES>
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t& v, uint32_t* lds_waves) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds_waves[w] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < WAVES; ++k) {
        if (k < w) before += lds_waves[k];
        total += lds_waves[k];
    }
    v = before + inc - v;
    __syncthreads();
    return total;
}

}  // namespace rr
