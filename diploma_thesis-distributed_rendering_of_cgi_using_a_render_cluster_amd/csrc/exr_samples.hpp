// The samples of an OPEN_EXR file as functions of the film, and the byte
// OpenEXR's ZIP and RLE codecs see at a position: what exr.hip's deflate front
// ends and exr_codec.hip's per-scanline coders share. Device code only.
//
// A band of `rows` scanlines from image row row0 holds per scanline the planes
// (C = 4: A, B, G, R; 3: B, G, R; 1: Y) of W samples each; sample k counts
// scanline by scanline, plane by plane. The codecs' preprocessing moves the
// even-indexed bytes of the band's n bytes to the first (n + 1) / 2 positions
// and the odd-indexed bytes behind them, then replaces every byte but the
// first by its difference to its predecessor + 128 (n is even here).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "grey.h"

namespace rr {

namespace {

// float -> half bits: clamped to +-65504, round to nearest even, subnormals kept.
__device__ __forceinline__ uint32_t half_bits(float f) {
    const uint32_t x = __float_as_uint(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    uint32_t a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return sign | 0x7E00u;  // NaN
    a = min(a, 0x477FE000u);                     // 65504
    if (a >= 0x38800000u) {                      // >= 2^-14: a normal half
        a -= 112u << 23;
        a += 0xFFFu + ((a >> 13) & 1u);
        return sign | (a >> 13);
    }
    const uint32_t e = a >> 23;
    if (e < 102u) return sign;  // < 2^-25: below half of the smallest subnormal (and 0)
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    const uint32_t s = 126u - e;  // 14 .. 24: m * 2^(e - 150) in units of 2^-24
    uint32_t h = m >> s;
    const uint32_t rem = m & ((1u << s) - 1u), mid = 1u << (s - 1u);
    if (rem > mid || (rem == mid && (h & 1u))) h += 1u;
    return sign | h;
}

struct Film {
    const float4* px;
    float inv_spp;
    int alpha_one;
};

// Mean of sample k of a band of an image W wide: C = 1: Y, the Rec.709 luma of
// the means (products and sums rounded one by one, left to right).
template <int C>
__device__ __forceinline__ float sample_mean(const Film& fm, int width, int row0, uint32_t k) {
    const uint32_t W = (uint32_t)width, row_samples = (uint32_t)C * W;
    const uint32_t row = k / row_samples, rem = k - row * row_samples;
    const uint32_t ch = rem / W, x = rem - ch * W;
    const float4 v = fm.px[(size_t)(row0 + (int)row) * W + x];
    if constexpr (C == 4) {
        const float c = ch == 0 ? v.w : ch == 1 ? v.z : ch == 2 ? v.y : v.x;
        // alpha_one: 0 the film's alpha mean, 1 A = 1, 2 a mask: A = 1 where film.w != 0, else 0
        if (ch == 0 && fm.alpha_one) return (fm.alpha_one == 2 && c == 0.0f) ? 0.0f : 1.0f;
        return __fmul_rn(c, fm.inv_spp);
    } else if constexpr (C == 3) {
        const float c = ch == 0 ? v.z : ch == 1 ? v.y : v.x;
        return __fmul_rn(c, fm.inv_spp);
    } else {
        const float r = __fmul_rn(v.x, fm.inv_spp), g = __fmul_rn(v.y, fm.inv_spp), b = __fmul_rn(v.z, fm.inv_spp);
        return luma709(r, g, b);
    }
}

// Half of sample k of a band.
template <int C>
__device__ __forceinline__ uint32_t sample_half(const Film& fm, int W, int row0, uint32_t k) {
    return half_bits(sample_mean<C>(fm, W, row0, k));
}

// Bits of sample k of a band of FLOAT channels: the mean itself, no clamp and no rounding.
template <int C>
__device__ __forceinline__ uint32_t sample_float(const Film& fm, int W, int row0, uint32_t k) {
    return __float_as_uint(sample_mean<C>(fm, W, row0, k));
}

// Byte j of a band of halfs after the reorder (before the predictor): within a
// half of the reordered bytes, position k is sample k.
template <int C>
__device__ __forceinline__ uint32_t reordered_byte(const Film& fm, int W, int row0, uint32_t half_n, uint32_t j) {
    const bool hi = j >= half_n;
    const uint32_t h = sample_half<C>(fm, W, row0, hi ? j - half_n : j);
    return hi ? h >> 8 : h & 0xFFu;
}

// Byte j of a band of floats after the reorder (before the predictor): the
// first n / 2 positions alternate bytes 0 and 2 of consecutive samples, the
// second n / 2 bytes 1 and 3: position q of a half belongs to sample q / 2.
template <int C>
__device__ __forceinline__ uint32_t reordered_byte32(const Film& fm, int W, int row0, uint32_t half_n, uint32_t j) {
    const bool hi = j >= half_n;
    const uint32_t q = hi ? j - half_n : j;
    const uint32_t bits = sample_float<C>(fm, W, row0, q >> 1);
    return (bits >> (16u * (q & 1u) + (hi ? 8u : 0u))) & 0xFFu;
}

// Byte j of a band of n bytes as the ZIP and RLE coders see it: reordered, less
// its predecessor + 128. Full: FLOAT channels, else HALF.
template <int C, bool Full>
__device__ __forceinline__ uint32_t exr_pred_byte(const Film& fm, int W, int row0, uint32_t n, uint32_t j) {
    if constexpr (Full) {
        uint32_t v = reordered_byte32<C>(fm, W, row0, n / 2, j);
        if (j > 0) v = (v - reordered_byte32<C>(fm, W, row0, n / 2, j - 1) + 128u) & 0xFFu;
        return v;
    } else {
        uint32_t v = reordered_byte<C>(fm, W, row0, n / 2, j);
        if (j > 0) v = (v - reordered_byte<C>(fm, W, row0, n / 2, j - 1) + 128u) & 0xFFu;
        return v;
    }
}

}  // namespace

}  // namespace rr
