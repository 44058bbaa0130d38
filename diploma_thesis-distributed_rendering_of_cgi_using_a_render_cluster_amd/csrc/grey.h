// The grey (BW colour mode) rule of every output format, shared by the device
// coders and the host encoders: Rec.709 luma, weights 0.2126, 0.7152, 0.0722.
// Every product and sum is a float32 operation of its own, left to right, no
// fmaf, so numpy's float32 restates it bit for bit (tests/color_modes.py).
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define RR_GREY_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_GREY_HD inline
#endif

namespace rr {

RR_GREY_HD float luma709(float r, float g, float b) {
#pragma clang fp contract(off)
    const float pr = 0.2126f * r, pg = 0.7152f * g, pb = 0.0722f * b;
    const float s = pr + pg;
    return s + pb;
}

// An RGBA8 pixel's grey code (8-bit files: JPEG, PNG 8), from the image after
// the view transform.
RR_GREY_HD uint32_t grey8(uint32_t r, uint32_t g, uint32_t b) {
#pragma clang fp contract(off)
    const float k = 1.0f / 255.0f;
    const float l = luma709((float)r * k, (float)g * k, (float)b * k);
    if (l <= 0.0f) return 0u;
    if (l > 1.0f - 0.5f / 255.0f) return 255u;
    return (uint32_t)(255.0f * l + 0.5f);
}

}  // namespace rr
