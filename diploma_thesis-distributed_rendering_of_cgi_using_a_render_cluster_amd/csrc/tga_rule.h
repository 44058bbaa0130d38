// The packet rule of run-length coded TARGA files ("TARGA"), shared by the
// host encoder (image_io encode_tga) and the device coder (tga.hip), and the
// sizes both take from it. A pixel is C bytes in file order (C = 4: B, G, R, A;
// 3: B, G, R; 1: the grey code of grey.h); rows go bottom row first.
//
// Packets never cross a row. Within a row of W pixels the packets follow the
// shared rule of rle_rule.h with the numbers of TgaRle<C>:
//  - pixels are equal when all C bytes are;
//  - a run of at least 2 pixels is a run stretch for C = 3 and 4, of at least 3
//    for C = 1, where a two-pixel run would cost a split of the literals around
//    it (up to two bytes) and save nothing;
//  - a packet holds at most 128 pixels. A run packet is the byte
//    0x80 | (count - 1) and one pixel, a literal packet the byte count - 1 and
//    count pixels.
// A row is longest when all of it is literal: W C + ceil(W / 128) bytes.
// The rule is the project's own: Blender's encoder picks its packets
// differently; every decoder returns the same pixels.
//
// With eq(j) = "pixel j equals pixel j - 1" (false for j <= 0 and j >= W),
// pixel i lies in a run stretch (rle_in_run) when
//   C = 3, 4: eq(i) | eq(i + 1)
//   C = 1:    eq(i - 1) & eq(i) | eq(i) & eq(i + 1) | eq(i + 1) & eq(i + 2)
// Integers only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rle_rule.h"

#define RR_TGA_HD RR_RLE_HD

namespace rr {

constexpr uint32_t kTgaPacket = 128;  // pixels a packet holds at most
constexpr uint32_t kTgaHeaderBytes = 18;
constexpr int kTgaMaxSide = 65535;    // width and height are uint16 fields

// The numbers of the packet rule for pixels of C bytes.
template <int C>
struct TgaRle {
    static constexpr uint32_t kMinRun = C == 1 ? 3 : 2;
    static constexpr uint32_t kRunPacket = kTgaPacket, kLitPacket = kTgaPacket;
    static constexpr uint32_t kElemBytes = C;
    static RR_TGA_HD uint32_t header(bool run, uint32_t count) { return (run ? 0x80u : 0u) | (count - 1u); }
};

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

}  // namespace rr
