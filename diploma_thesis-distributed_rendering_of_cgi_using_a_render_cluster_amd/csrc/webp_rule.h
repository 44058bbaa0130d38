// The rules of the lossless WebP files ("WEBP", .webp: a RIFF container with one
// VP8L chunk) this project writes, shared by the host encoder (image_io
// encode_webp) and the device coder (webp.hip), and the sizes both take from
// them.
//
// The payload is an LSB-first bit stream: byte 0x2F, 14 bits W - 1, 14 bits
// H - 1, the alpha hint, 3 bits version 0; the subtract-green transform; the
// predictor transform with one block size for the whole image (block bits 9)
// and mode 1, the left neighbour, in every block, its sub-image coded with five
// one-symbol codes; then the main image: no colour cache, no meta prefix codes,
// five prefix codes (green + lengths 280 symbols, red, blue, alpha 256 each,
// distance 40) and the pixels in scan order.
//
// The pixel word is A << 24 | R << 16 | G << 8 | B. C = 4: the RGBA8 pixel as it
// is; C = 3: alpha 255; C = 1: the grey code of grey.h in R, G and B, alpha 255.
// Subtract-green takes G from R and B; the residual is the word minus its
// prediction, per channel mod 256: pixel (0, 0) is predicted by 0xFF000000, the
// rest of row 0 by its left neighbour, the rest of column 0 by the pixel above,
// every other pixel by its left neighbour (mode 1).
//
// The run rule, the project's own (any reader returns the same pixels whatever
// the rule; only the bytes are ours). The unit is the residual word. No copy
// crosses a row, and a row's first pixel is a literal. Within a row, with
// eq(j) = "residual j equals residual j - 1" (false for j <= 0 and j >= W):
//  1. A stretch is a maximal run of pixels with eq set.
//  2. A stretch is cut into chunks of kWebpMaxCopy pixels and the remainder.
//  3. A chunk of at least kWebpMinRun pixels is one copy of its length at
//     distance 1 (distance code 2, "the pixel to the left"); the pixels of a
//     shorter chunk are literals, and so is every pixel outside a stretch.
// A literal is the G, R, B, A residuals through their codes; a copy the green
// symbol 256 + prefix(length), the prefix's extra bits, the distance symbol
// prefix(2) = 1, which has no extra bits.
//
// The prefix codes: an alphabet with at most two used symbols, all below 256,
// is written as a simple code (one symbol: 0 bits a use, two: 1 bit, the lower
// symbol 0); an unused alphabet as the simple code of symbol 0. Every other
// alphabet is a normal code: lengths of at most 15 bits from the Huffman tree
// over (count, index) with the repair of deflate.hip's build_lengths, canonical
// codes, all 19 code-length-code lengths, every symbol's length as a plain
// length 0 .. 15 (no repeat codes) through a code-length code of at most 7
// bits; a code-length alphabet with one used symbol gives it length 1, and its
// uses take 0 bits. Integers only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "grey.h"

#if defined(__HIP__)
#define RR_WEBP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_WEBP_HD inline
#endif

namespace rr {

constexpr uint32_t kWebpMinRun = 3;      // pixels a copy stands for at least (2 .. 8)
constexpr uint32_t kWebpMaxCopy = 4096;  // and at most: the format's longest length
constexpr int kWebpMaxSide = 16384;      // width and height are 14-bit fields
constexpr uint32_t kWebpBlockBits = 9;   // the predictor's block size, the format's largest
static_assert(kWebpMinRun >= 2 && kWebpMinRun <= 8, "the window of webp_kind");

// The five alphabets in one table: green + lengths, red, blue, alpha, distance.
constexpr int kWebpGreen = 0, kWebpRed = 280, kWebpBlue = 536, kWebpAlpha = 792, kWebpDist = 1048;
constexpr int kWebpSyms = 1088;
constexpr int kWebpAlphabets = 5;
constexpr uint32_t kWebpDistSym = 1;  // prefix(2): distance code 2
constexpr int kWebpMaxBits = 15, kWebpClMaxBits = 7;
RR_WEBP_HD constexpr int webp_base(int a) { return a == 0 ? kWebpGreen : a == 1 ? kWebpRed : a == 2 ? kWebpBlue : a == 3 ? kWebpAlpha : kWebpDist; }
RR_WEBP_HD constexpr int webp_size(int a) { return a == 0 ? 280 : a == 4 ? 40 : 256; }

// The order in which a normal code states its 19 code-length-code lengths:
// 17, 18, 0, 1, 2, 3, 4, 5, 16, 6 .. 15.
RR_WEBP_HD constexpr int webp_cl_order(int k) { return k == 0 ? 17 : k == 1 ? 18 : k < 8 ? k - 2 : k == 8 ? 16 : k - 3; }

constexpr uint32_t kWebpRiffBytes = 20;  // "RIFF" size "WEBP" "VP8L" size

// The bits a token takes at most (a literal: four codes of 15 bits; a copy
// takes fewer), and the header: the fixed fields and five normal codes.
constexpr uint64_t kWebpTokenMaxBits = 4 * kWebpMaxBits;
constexpr uint64_t kWebpHeaderMaxBits = 128 + kWebpAlphabets * 64 + (uint64_t)kWebpSyms * kWebpClMaxBits;

// The payload's bound in bytes: the header and every pixel a literal at its
// longest. 0: W or H outside the format, C not 1, 3 or 4, or 2 GB and more.
RR_WEBP_HD uint64_t webp_body_max_bytes(int W, int H, int C) {
    if (W <= 0 || H <= 0 || W > kWebpMaxSide || H > kWebpMaxSide || (C != 1 && C != 3 && C != 4)) return 0;
    const uint64_t bits = kWebpHeaderMaxBits + (uint64_t)W * (uint64_t)H * kWebpTokenMaxBits;
    const uint64_t bound = (bits + 7) / 8;
    return bound < (1ull << 31) ? bound : 0;
}

// The pixel word after subtract-green of an RGBA8 pixel (R in the low byte) in
// colour mode C.
RR_WEBP_HD uint32_t webp_pixel(uint32_t rgba, int C) {
    uint32_t r = rgba & 255u, g = (rgba >> 8) & 255u, b = (rgba >> 16) & 255u, a = rgba >> 24;
    if (C == 1) r = g = b = grey8(r, g, b);
    if (C != 4) a = 255u;
    return a << 24 | ((r - g) & 255u) << 16 | g << 8 | ((b - g) & 255u);
}

// x - p per channel mod 256.
RR_WEBP_HD uint32_t webp_sub(uint32_t x, uint32_t p) {
    uint32_t r = 0;
    for (int k = 0; k < 32; k += 8) r |= (((x >> k) - (p >> k)) & 255u) << k;
    return r;
}

constexpr uint32_t kWebpFirstPrediction = 0xFF000000u;

// The prefix symbol of a length or distance code v >= 1, its extra bits and
// their count.
RR_WEBP_HD void webp_prefix(uint32_t v, uint32_t& sym, uint32_t& nb, uint32_t& extra) {
    if (v <= 2u) {
        sym = v - 1u, nb = 0u, extra = 0u;
        return;
    }
    const uint32_t d = v - 1u;
    const uint32_t h = 31u - (uint32_t)__builtin_clz(d);
    sym = 2u * h + ((d >> (h - 1u)) & 1u);
    nb = h - 1u;
    extra = d & ((1u << nb) - 1u);
}

// What pixel i of a row is in the token stream, from eq(i + k) in bit k of
// `win` (k = 0 .. kWebpMinRun - 1) and, where eq(i), its position q in its
// stretch: a literal, the first pixel of a copy, or a pixel a copy covers.
enum { kWebpLiteral = 0, kWebpCopy = 1, kWebpCovered = 2 };
RR_WEBP_HD int webp_kind(uint32_t win, uint32_t q) {
    if (!(win & 1u)) return kWebpLiteral;
    const uint32_t m = q % kWebpMaxCopy;  // the position in its chunk
    if (m >= kWebpMinRun) return kWebpCovered;
    const uint32_t need = ((1u << (kWebpMinRun - 1u - m)) - 1u) << 1;  // eq(i + 1 .. i + kWebpMinRun - 1 - m)
    if ((win & need) != need) return kWebpLiteral;                     // a chunk shorter than kWebpMinRun
    return m == 0u ? kWebpCopy : kWebpCovered;
}

}  // namespace rr
