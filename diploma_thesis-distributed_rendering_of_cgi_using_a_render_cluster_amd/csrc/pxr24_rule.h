// The 24-bit form PXR24 chunks hold of FLOAT samples (rr_set_exr_codec
// RR_EXR_CODEC_PXR24), shared by the device front end (exr.hip Pxr24Front) and
// the host entry point rr_debug_float24: sign, the 8 exponent bits and the top
// 15 mantissa bits, rounded to nearest (halves away from zero in magnitude). A
// reader returns the 24 bits << 8 as the float's bits.
//
// With s, e, m the sign, exponent and mantissa fields of the bits in place:
//   finite    i = ((e | m) + (m & 0x80)) >> 8; a round-up that would reach the
//             exponent of infinity (i >= 0x7f8000) truncates instead
//   infinity  e >> 8
//   NaN       (e >> 8) | (m >> 8), with the lowest bit set when that leaves no
//             mantissa bit: a NaN stays a NaN
// and the result is (s >> 8) | i.
//
// Restated from OpenEXR's floatToFloat24 from memory: not pinned against an
// OpenEXR library (there was none at hand). Integers only.
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define RR_PXR24_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_PXR24_HD inline
#endif

namespace rr {

RR_PXR24_HD uint32_t float24_bits(uint32_t bits) {
    const uint32_t s = bits & 0x80000000u, e = bits & 0x7F800000u, m = bits & 0x007FFFFFu;
    uint32_t i;
    if (e == 0x7F800000u) {
        if (m) {
            const uint32_t mm = m >> 8;
            i = (e >> 8) | mm | (mm == 0u ? 1u : 0u);
        } else {
            i = e >> 8;
        }
    } else {
        i = ((e | m) + (m & 0x00000080u)) >> 8;
        if (i >= 0x7F8000u) i = (e | m) >> 8;
    }
    return (s >> 8) | i;
}

}  // namespace rr
