// Dither of the 8-bit image (rr_set_dither): the noise Blender 3.6 adds to the
// display-referred floats before it turns them into bytes (imbuf
// dither_random_value, float_to_byte_dither_v4), host and device. The rule
// and its constants are restated from memory of that source, which is not
// present here: parity with Blender's own files stays unpinned.
//
// For the pixel in column x of the row yb from the bottom, in a W x H image
// dithered with intensity g (inv_w = 1.0f / (float)W, inv_h = 1.0f / (float)H):
//   s  = (float)x * inv_w,  t = (float)yb * inv_h
//   h0 = fract(sin_fixed(s * 12.9898f + t * 78.233f) * 43758.5453f)
//   h1 = fract(sin_fixed(s * 19.9898f + t * 119.233f) * 798.5453f)
//   n  = h0 + h1 - 0.5f           triangle-shaped, in [-0.5, 1.5)
//   code = quantize8(d + n * 0.0033f * g)   the same n for R, G and B
// Every product and sum is a float32 operation of its own, left to right,
// contraction off and no fmaf, so tests/dither.py restates it bit for bit in
// numpy float32.
#pragma once
#pragma clang fp contract(off)

#include "rr_device.h"

namespace rr {

constexpr float kDitherAx = 12.9898f, kDitherAy = 78.233f, kDitherAm = 43758.5453f;
constexpr float kDitherBx = 19.9898f, kDitherBy = 119.233f, kDitherBm = 798.5453f;
constexpr float kDitherScale = 0.0033f;

// sin(a) without libm, written like log2_fixed / exp2_fixed (view_filmic.h):
// libm's sinf, the device's and numpy's differ in their last bits, which the
// hash multiplies by 43758.5453. a = n pi/2 + r with n the nearest integer
// (|r| <= pi/4 and a rounding's worth), pi/2 in three parts (Cody-Waite;
// n * 1.5703125 and n * 4.83751297e-4 are exact for |n| < 2^13), then the
// odd series of sin r to r^7 or the even one of cos r to r^8 (minimax
// coefficients, truncation < 1e-7), picked and signed by n mod 4.
// |sin_fixed(a) - sin(a)| <= 2^-18 for |a| <= 256 (tests/test_dither_format.py;
// the hash's arguments reach 139.2). 0 for |a| > 8192 and for NaN.
RR_HD float sin_fixed(float a) {
    if (!(fabsf(a) <= 8192.0f)) return 0.0f;
    const float h = a * 0.636619747f + 0.5f;
    int n = (int)h;
    if ((float)n > h) n = n - 1;
    const float fn = (float)n;
    const float r = ((a - fn * 1.5703125f) - fn * 4.83751297e-4f) - fn * 7.54978996e-8f;
    const float z = r * r;
    float v;
    if (n & 1) v = ((2.44331568e-5f * z - 1.38873165e-3f) * z + 4.16666456e-2f) * z * z - 0.5f * z + 1.0f;
    else v = ((-1.95152959e-4f * z + 8.33216123e-3f) * z - 0.166666552f) * z * r + r;
    return (n & 2) ? 0.0f - v : v;
}

// x - floor(x) of a finite x
RR_HD float fract_fixed(float x) { return x - floorf(x); }

// The n of the pixel in column x, row yb from the bottom.
RR_HD float dither_noise(int x, int yb, float inv_w, float inv_h) {
    const float s = (float)x * inv_w, t = (float)yb * inv_h;
    const float h0 = fract_fixed(sin_fixed(s * kDitherAx + t * kDitherAy) * kDitherAm);
    const float h1 = fract_fixed(sin_fixed(s * kDitherBx + t * kDitherBy) * kDitherBm);
    return h0 + h1 - 0.5f;
}

}  // namespace rr
