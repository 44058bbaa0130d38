// The rules of Radiance RGBE files ("HDR", .hdr), shared by the host encoder
// (image_io encode_hdr) and the device coder (hdr.hip), and the sizes both
// take from them: how three floats become an RGBE quad, and how a scanline of
// quads is run-length coded. Integers on the floats' bits, no float operation.
//
// The RGBE rule. Per channel: a negative value, -0 or NaN becomes 0; a value
// above 0x1.fep126f becomes that value (+inf and FLT_MAX land on mantissa 255,
// exponent byte 255). Per pixel, with m the largest of the three clamped
// channels: m < 1e-32f gives the quad 0, 0, 0, 0. Otherwise, with E m's biased
// exponent (bits >> 23), the exponent byte is E + 2 (frexp's e + 128), and a
// channel with biased exponent Ec and 24-bit significand s gives the byte
// s >> (16 + E - Ec), 0 when that shift is 32 or more or the channel is
// denormal: floor(c 2^(8 - e)), truncation, no float division anywhere.
// UNPINNED: this is the project's own rule and is not pinned against Blender's
// files. Blender computes frexp(m) * 256 / m in float and truncates the
// product (quoted from memory; there is no Blender to check it against); the
// two agree except where that quotient rounds off a power of two.
//
// The scanline rule. Rows go top row first, pixels left to right. A row with
// W < 8 or W > 32767 is flat: W quads R, G, B, E and nothing else. Every other
// row is the bytes 2, 2, W >> 8, W & 255 and then the R, the G, the B and the E
// plane, W bytes each, coded on its own; packets never cross a plane or a row.
// Within a plane the packets follow the shared rule of rle_rule.h with the
// numbers of HdrRle:
//  - a run of at least 4 bytes (Radiance's MINRUN) is a run stretch; a run of
//    3 saves nothing once the literals around it are split;
//  - a run packet stands for at most 127 bytes (a stretch's last may be
//    shorter than 4; count 1 is legal), a literal packet holds at most 128. A
//    run packet is the byte 128 + count and the value, a literal packet the
//    byte count and count bytes.
// A plane is longest when all of it is literal: W + ceil(W / 128) bytes.
// Radiance's own encoder picks its packets differently (a greedy serial scan
// with a special case for short runs); every decoder returns the same quads
// from either.
//
// With eq(j) = "byte j equals byte j - 1" (false for j <= 0 and j >= W), byte
// i lies in a run stretch (rle_in_run) when one of the four windows of three
// consecutive eq bits that cover it, eq(i - 2 .. i) to eq(i + 1 .. i + 3), is
// all set.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rle_rule.h"

#define RR_HDR_HD RR_RLE_HD

namespace rr {

constexpr uint32_t kHdrMinRun = 4;        // bytes a run stretch has at least
constexpr uint32_t kHdrRunPacket = 127;   // bytes a run packet stands for at most
constexpr uint32_t kHdrLitPacket = 128;   // bytes a literal packet holds at most
constexpr int kHdrCodedMinW = 8, kHdrCodedMaxW = 32767;  // the widths of coded rows
constexpr uint32_t kHdrMaxBits = 0x7EFF0000u;   // 0x1.fep126f
constexpr uint32_t kHdrTinyBits = 0x0A4FB11Fu;  // 1e-32f

// ---- the RGBE rule ----------------------------------------------------------

// A channel's clamped value, as bits: never negative, never NaN, at most 0x1.fep126f.
RR_HDR_HD uint32_t hdr_clamp_bits(uint32_t b) {
    if (b >> 31) return 0u;          // negative values, -0, NaNs with the sign set
    if (b > 0x7F800000u) return 0u;  // NaN
    return b > kHdrMaxBits ? kHdrMaxBits : b;
}

// A clamped channel's byte beside a largest channel of biased exponent E.
RR_HDR_HD uint32_t hdr_mantissa(uint32_t c, uint32_t E) {
    const uint32_t Ec = c >> 23;
    if (Ec == 0u) return 0u;  // zero and denormals
    const uint32_t shift = 16u + E - Ec;
    return shift >= 32u ? 0u : ((c & 0x7FFFFFu) | 0x800000u) >> shift;
}

// The quad of three floats given by their bits, as one word: R in the low
// byte, then G, B, E: the file's four bytes read as a little-endian word.
RR_HDR_HD uint32_t hdr_quad(uint32_t r, uint32_t g, uint32_t b) {
    r = hdr_clamp_bits(r), g = hdr_clamp_bits(g), b = hdr_clamp_bits(b);
    uint32_t m = r > g ? r : g;  // non-negative floats order as their bits do
    m = m > b ? m : b;
    if (m < kHdrTinyBits) return 0u;
    const uint32_t E = m >> 23;
    return hdr_mantissa(r, E) | hdr_mantissa(g, E) << 8 | hdr_mantissa(b, E) << 16 | (E + 2u) << 24;
}

// ---- the scanline rule ------------------------------------------------------

RR_HDR_HD constexpr bool hdr_row_flat(int W) { return W < kHdrCodedMinW || W > kHdrCodedMaxW; }

// The bytes a coded plane takes at most (all literal), and a row (coded: the
// four marker bytes and four planes; flat: its quads).
RR_HDR_HD constexpr uint64_t hdr_plane_max_bytes(uint64_t W) { return W + (W + kHdrLitPacket - 1) / kHdrLitPacket; }
RR_HDR_HD constexpr uint64_t hdr_row_max_bytes(int W) {
    return hdr_row_flat(W) ? 4ull * (uint64_t)W : 4ull + 4ull * hdr_plane_max_bytes((uint64_t)W);
}

// The body's bound (a flat body's exact length). 0: W or H not positive, or a
// body of 2 GB and more.
RR_HDR_HD uint64_t hdr_body_max_bytes(int W, int H) {
    if (W <= 0 || H <= 0) return 0;
    const uint64_t row = hdr_row_max_bytes(W);
    if (row >= (1ull << 31)) return 0;
    const uint64_t n = (uint64_t)H * row;
    return n < (1ull << 31) ? n : 0;
}

// The numbers of the packet rule for a plane's bytes.
struct HdrRle {
    static constexpr uint32_t kMinRun = kHdrMinRun, kRunPacket = kHdrRunPacket, kLitPacket = kHdrLitPacket;
    static constexpr uint32_t kElemBytes = 1;
    static RR_HDR_HD uint32_t header(bool run, uint32_t count) { return (run ? 128u : 0u) + count; }
};

}  // namespace rr
