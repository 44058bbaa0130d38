// The packet rule the run-length coded formats share (TARGA, HDR, IRIS), stated
// once for the host encoders (image_io) and the device packer (rle_device.hpp).
// A format gives its numbers in a traits struct T (tga_rule.h TgaRle<C>,
// hdr_rule.h HdrRle, iris_rule.h IrisRle):
//   kMinRun     elements a run stretch has at least (2 .. 4)
//   kRunPacket  elements a run packet stands for at most
//   kLitPacket  elements a literal packet holds at most
//   kElemBytes  bytes of an element (a TARGA pixel's C, else 1)
//   header(run, count)  the header byte of a packet of `count` elements
//
// Within a row (or plane, or row-plane) of W elements, which no packet crosses:
//  1. It is cut into maximal runs of equal consecutive elements.
//  2. A run of at least kMinRun elements is a run stretch.
//  3. The elements between run stretches, and between a run stretch and an end,
//     form literal stretches.
//  4. A stretch of n elements is n / cap packets of cap elements, cap being
//     kRunPacket or kLitPacket, then one packet of the remainder if there is
//     one. A run packet is its header byte and one element, a literal packet
//     its header byte and its elements.
//
// With eq(j) = "element j equals element j - 1" (false for j <= 0 and j >= W),
// element i lies in a run stretch when one of the kMinRun windows of
// kMinRun - 1 consecutive eq bits that cover it, eq(i - kMinRun + 2 ..) to
// eq(i + 1 ..), is all set; a stretch starts at i when i = 0, when i's kind
// differs from i - 1's, or when i is in a run stretch and !eq(i) (the next
// run). The device reads these from a window of eight eq bits anchored at
// eq(i - 3). Integers only.
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define RR_RLE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_RLE_HD inline
#endif

namespace rr {

// The device's window of element i: bit k is eq(i - 3 + k), k = 0 .. 7. Its
// kind and "a stretch starts at i" and "at i + 1" read eq(i - kMinRun + 1) ..
// eq(i + kMinRun), which the window holds for kMinRun <= 4.
constexpr int kRleWinBack = 3, kRleWinFwd = 4;
constexpr uint32_t kRleWinMask = (1u << (kRleWinBack + 1 + kRleWinFwd)) - 1u;

// Whether element i is in a run stretch, from eq(i - 2 + k) in bit k of `e`
// (read: eq(i - kMinRun + 2) .. eq(i + kMinRun - 1)).
template <class T>
RR_RLE_HD bool rle_in_run(uint32_t e) {
    static_assert(T::kMinRun >= 2 && T::kMinRun <= (uint32_t)kRleWinFwd && T::kMinRun <= (uint32_t)kRleWinBack + 1u,
                  "the eq bits of the kind of i - 1 and of i + 1 lie in eq(i - 3) .. eq(i + 4)");
    uint32_t all = e;  // bit k: the window of kMinRun - 1 bits from bit k is all set
    for (uint32_t j = 1; j + 1 < T::kMinRun; ++j) all &= e >> j;
    return (all & (((1u << T::kMinRun) - 1u) << (4u - T::kMinRun))) != 0u;
}

// Whether a stretch starts at element i > 0, from eq(i - 3 + k) in bit k of `e`
// (read: eq(i - kMinRun + 1) .. eq(i + kMinRun - 1)).
template <class T>
RR_RLE_HD bool rle_stretch_start(uint32_t e) {
    const bool run = rle_in_run<T>(e >> 1), before = rle_in_run<T>(e);
    return run != before || (run && !((e >> 3) & 1u));
}

// The elements a packet of the kind holds at most.
template <class T>
RR_RLE_HD constexpr uint32_t rle_packet_cap(bool run) {
    return run ? T::kRunPacket : T::kLitPacket;
}

}  // namespace rr
