// The adaptive row filter of PNG files (rr_set_png_compression), shared by the
// host encoder (image_io encode_png) and the device coders (png.hip,
// png16.hip): libpng's default for 8- and 16-bit grey, RGB and RGBA images,
// which Blender leaves in place behind write_still. Restated from the PNG
// specification and libpng 1.6's png_write_find_filter, and pinned against
// libpng 1.6.37's own files (tests/test_png_compression_format.py).
//
// For byte x of a scanline of n raw bytes, bpp bytes a pixel:
//   a = the byte bpp positions before it (0 for the first pixel),
//   b = the same byte of the image row above (0 on the first row),
//   c = the row above's byte bpp positions before (0 where either is absent).
// Residuals mod 256 of the five types: None x, Sub x - a, Up x - b, Average
// x - ((a + b) >> 1), Paeth x - paeth(a, b, c). A type's score is the sum over
// the row of r < 128 ? r : 256 - r (the filter byte is not counted); the row
// takes the smallest, the types tried in the order 0 .. 4 and a later one only
// when strictly smaller. libpng leaves out the types that need a neighbour an
// image does not have: in an image of one row Up, Average and Paeth, in an
// image one pixel wide Sub, Average and Paeth. Up then equals None and Paeth
// equals Sub (one row), Sub equals None and Paeth equals Up (one pixel), so
// they never win anyway; Average could, and is not tried in such an image.
// Integers only: host and device give the same bytes.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#define RR_PNGF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_PNGF_HD inline
#endif

namespace rr {

constexpr int kPngFilterTypes = 5;

RR_PNGF_HD uint32_t png_paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int ia = (int)a, ib = (int)b, ic = (int)c;
    int pa = ib - ic, pb = ia - ic, pc = ia + ib - 2 * ic;
    pa = pa < 0 ? -pa : pa;
    pb = pb < 0 ? -pb : pb;
    pc = pc < 0 ? -pc : pc;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// The byte a filter type predicts for x.
RR_PNGF_HD uint32_t png_predict(uint32_t type, uint32_t a, uint32_t b, uint32_t c) {
    return type == 0 ? 0u : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
}

RR_PNGF_HD uint32_t png_residual(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    return (x - png_predict(type, a, b, c)) & 0xFFu;
}

RR_PNGF_HD uint32_t png_cost(uint32_t r) { return r < 128u ? r : 256u - r; }

// score[t] += the cost of byte x under every type t.
template <class Sum>
RR_PNGF_HD void png_score(uint32_t x, uint32_t a, uint32_t b, uint32_t c, Sum score[kPngFilterTypes]) {
    score[0] += png_cost(x);
    score[1] += png_cost((x - a) & 0xFFu);
    score[2] += png_cost((x - b) & 0xFFu);
    score[3] += png_cost((x - ((a + b) >> 1)) & 0xFFu);
    score[4] += png_cost((x - png_paeth(a, b, c)) & 0xFFu);
}

// The type a row takes: order 0 .. 4, a later one only when strictly smaller.
// thin: the image has one row or is one pixel wide (no Average).
template <class Sum>
RR_PNGF_HD uint32_t png_pick(const Sum score[kPngFilterTypes], bool thin) {
    uint32_t best = 0;
    for (uint32_t t = 1; t < (uint32_t)kPngFilterTypes; ++t)
        if (score[t] < score[best] && !(thin && t == 3u)) best = t;
    return best;
}

// Host: the type of the row `cur` of n bytes below `up` (nullptr: the first
// row) in an image of `rows` rows.
inline uint32_t png_pick_row(const uint8_t* cur, const uint8_t* up, size_t n, size_t bpp, size_t rows) {
    uint64_t score[kPngFilterTypes] = {0, 0, 0, 0, 0};
    for (size_t q = 0; q < n; ++q) {
        const uint32_t a = q >= bpp ? cur[q - bpp] : 0u, b = up ? up[q] : 0u, c = (up && q >= bpp) ? up[q - bpp] : 0u;
        png_score(cur[q], a, b, c, score);
    }
    return png_pick(score, rows == 1 || n <= bpp);
}

// Host: the row's n residuals under `type` into out.
inline void png_filter_row(uint32_t type, const uint8_t* cur, const uint8_t* up, size_t n, size_t bpp, uint8_t* out) {
    for (size_t q = 0; q < n; ++q) {
        const uint32_t a = q >= bpp ? cur[q - bpp] : 0u, b = up ? up[q] : 0u, c = (up && q >= bpp) ? up[q - bpp] : 0u;
        out[q] = (uint8_t)png_residual(type, cur[q], a, b, c);
    }
}

}  // namespace rr
