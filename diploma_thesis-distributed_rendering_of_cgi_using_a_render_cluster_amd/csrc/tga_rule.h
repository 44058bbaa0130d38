// The packet rule of run-length coded TARGA files ("TARGA"), shared by the
// host encoder (image_io encode_tga) and the device coder (tga.hip), and the
// sizes both take from it. A pixel is C bytes in file order (C = 4: B, G, R, A;
// 3: B, G, R; 1: the grey code of grey.h); rows go bottom row first.
//
// Packets never cross a row. Within a row of W pixels:
//  1. The row is cut into maximal runs of equal consecutive pixels (all C bytes
//     equal).
//  2. A run of at least tga_min_run(C) pixels is a run stretch: 2 pixels for
//     C = 3 and 4, 3 for C = 1, where a two-pixel run would cost a split of the
//     literals around it (up to two bytes) and save nothing.
//  3. The pixels between run stretches, and between a run stretch and a row
//     end, form literal stretches.
//  4. A stretch of n pixels is n / 128 packets of 128 pixels, then one packet
//     of the remainder if there is one. A run packet is the byte
//     0x80 | (count - 1) and one pixel, a literal packet the byte count - 1 and
//     count pixels.
// A row is longest when all of it is literal: W C + ceil(W / 128) bytes.
// The rule is the project's own: Blender's encoder picks its packets
// differently; every decoder returns the same pixels.
//
// With eq(j) = "pixel j equals pixel j - 1" (false for j <= 0 and j >= W),
// pixel i lies in a run stretch when its run has tga_min_run(C) pixels:
//   C = 3, 4: eq(i) | eq(i + 1)
//   C = 1:    eq(i - 1) & eq(i) | eq(i) & eq(i + 1) | eq(i + 1) & eq(i + 2)
// and a stretch starts at i when i = 0, when i's kind differs from i - 1's, or
// when i is in a run stretch and !eq(i) (the next run). Integers only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#define RR_TGA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_TGA_HD inline
#endif

namespace rr {

constexpr uint32_t kTgaPacket = 128;  // pixels a packet holds at most
constexpr uint32_t kTgaHeaderBytes = 18;
constexpr int kTgaMaxSide = 65535;    // width and height are uint16 fields

RR_TGA_HD constexpr uint32_t tga_min_run(int C) { return C == 1 ? 3u : 2u; }

// The bytes a coded row takes at most (all literal), and a raw row's bytes.
RR_TGA_HD constexpr uint64_t tga_row_max_bytes(uint64_t W, uint64_t C) {
    return W * C + (W + kTgaPacket - 1) / kTgaPacket;
}

// The body's bound: raw: its exact length. 0: W, H or C outside the format, or
// a body of 2 GB and more.
RR_TGA_HD uint64_t tga_body_max_bytes(int W, int H, int C, bool rle) {
    if (W <= 0 || H <= 0 || W > kTgaMaxSide || H > kTgaMaxSide || (C != 1 && C != 3 && C != 4)) return 0;
    const uint64_t n = (uint64_t)H * (rle ? tga_row_max_bytes((uint64_t)W, (uint64_t)C) : (uint64_t)W * (uint64_t)C);
    return n < (1ull << 31) ? n : 0;
}

// Whether pixel i is in a run stretch, from eq(i - 2 + k) in bit k of `e`
// (k = 0 .. 4: eq(i - 2) .. eq(i + 2)).
template <int C>
RR_TGA_HD bool tga_in_run(uint32_t e) {
    const bool m1 = (e >> 1) & 1u, z = (e >> 2) & 1u, p1 = (e >> 3) & 1u, p2 = (e >> 4) & 1u;
    if (C == 1) return (m1 && z) || (z && p1) || (p1 && p2);
    return z || p1;
}

// Whether a stretch starts at pixel i > 0, from eq(i - 3 + k) in bit k of `e`
// (k = 0 .. 5: eq(i - 3) .. eq(i + 2)).
template <int C>
RR_TGA_HD bool tga_stretch_start(uint32_t e) {
    const bool run = tga_in_run<C>(e >> 1), before = tga_in_run<C>(e);
    return run != before || (run && !((e >> 3) & 1u));
}

// The header byte of a packet of `count` pixels.
RR_TGA_HD uint32_t tga_packet_header(bool run, uint32_t count) { return (run ? 0x80u : 0u) | (count - 1u); }

}  // namespace rr
