// The device side of PNG's adaptive row filter (png_filter.h), shared by the
// 8-bit and the 16-bit coder (png.hip, png16.hip): k_png_pick chooses every
// row's filter type, PngAdaptiveFront is the byte function that puts the
// filtered rows in front of the deflate coder (deflate.hpp k_deflate_front).
//
// Src: the raw scanlines, src(row, q) = byte q < BPP W of image row `row`
// before the filter. BPP: bytes a pixel (C at 8 bits, 2C at 16).
#pragma once

#include <hip/hip_runtime.h>

#include "deflate.hpp"
#include "png_filter.h"

namespace rr {

// Raw scanlines held as bytes, `row_bytes` a row (the 16-bit coder's k_png16_raw).
struct PngRawRows {
    const uint8_t* __restrict__ raw;
    uint32_t row_bytes;
    __device__ __forceinline__ uint32_t operator()(uint32_t row, uint32_t q) const {
        return raw[(size_t)row * row_bytes + q];
    }
};

// x's neighbours a, b, c in the image (row above = the image's, whatever the band).
template <int BPP, class Src>
__device__ __forceinline__ void png_neighbours(const Src& src, uint32_t row, uint32_t q, uint32_t& a, uint32_t& b,
                                               uint32_t& c) {
    const bool left = q >= (uint32_t)BPP, above = row > 0u;
    a = left ? src(row, q - BPP) : 0u;
    b = above ? src(row - 1u, q) : 0u;
    c = (left && above) ? src(row - 1u, q - BPP) : 0u;
}

// One workgroup per image row: the five scores over the row's n bytes, then
// ftype[row] by png_pick. A score stays below 2^32: n <= 2^22 bytes (W <= 2^20
// at 4 bytes, 2^19 at 8), 128 a byte at most. No atomics, and no lane waits
// for another workgroup.
template <int BPP, class Src>
__global__ __launch_bounds__(256) void k_png_pick(Src src, uint32_t n, int H, uint8_t* __restrict__ ftype) {
    constexpr int kThreads = 256;
    __shared__ uint32_t red[kPngFilterTypes][kThreads / 64];
    const uint32_t row = blockIdx.x;
    if ((int)row >= H) return;
    uint32_t score[kPngFilterTypes] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t q = threadIdx.x; q < n; q += kThreads) {
        uint32_t a, b, c;
        png_neighbours<BPP>(src, row, q, a, b, c);
        png_score(src(row, q), a, b, c, score);
    }
    for (int t = 0; t < kPngFilterTypes; ++t) {
        const uint32_t s = wave_sum(score[t]);
        if ((threadIdx.x & 63) == 0) red[t][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total[kPngFilterTypes];
        for (int t = 0; t < kPngFilterTypes; ++t) {
            total[t] = 0u;
            for (int w = 0; w < kThreads / 64; ++w) total[t] += red[t][w];
        }
        ftype[row] = (uint8_t)png_pick(total, H == 1 || n <= (uint32_t)BPP);
    }
}

// Byte j of a band: the row's filter type in front of its residuals under that
// type. A pure function of the image and of ftype, which k_png_pick wrote in
// an earlier launch on the same stream.
template <int BPP, class Src>
struct PngAdaptiveFront {
    Src src;
    const uint8_t* __restrict__ ftype;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t, uint32_t j) const {
        const uint32_t r = j / p.stride, x = j - r * p.stride;
        const uint32_t row = (uint32_t)row0 + r;
        const uint32_t type = ftype[row];
        if (x == 0) return type;
        uint32_t a, b, c;
        png_neighbours<BPP>(src, row, x - 1u, a, b, c);
        return png_residual(type, src(row, x - 1u), a, b, c);
    }
};

template <int BPP, class Src>
void png_adaptive_front_device(const Src& src, const DeflatePlan& p, const DeflateBufs& c, uint8_t* ftype,
                               hipStream_t st) {
    k_png_pick<BPP, Src><<<dim3((unsigned)p.H), 256, 0, st>>>(src, p.stride - 1u, p.H, ftype);
    k_deflate_front<<<dim3(p.nsub, p.nbands), 256, 0, st>>>(PngAdaptiveFront<BPP, Src>{src, ftype}, p, c.filt,
                                                             c.adler_part);
}

}  // namespace rr
