// 8-bit PNG encode on the device: the Sub-filtered scanlines of the RGBA8 frame
// in front of the deflate coder (deflate.hip), so only the zlib stream crosses
// PCIe and the host writes the chunk framing (image_io png_wrap_stream).
// Replaces the PNG side of Blender's write_still (render-timing-script.py:83-92).
//
// A row is C W + 1 filtered bytes (C = 4 RGBA, 3 RGB, 1 grey: rr_set_color_mode):
// filter type 1 (Sub), then every image byte less the byte C positions (one
// pixel) before it. The bands are the pieces of one zlib stream with the stored
// fallback; the match distances are 1 (zero runs), C (the pixel period) and
// C W + 1 (the filtered row above).
// With rr_set_png_compression 0 .. 100 a row takes libpng's adaptive filter
// instead (png_filter.h): k_png_pick chooses every row's type, and
// PngAdaptiveFront forms the rows (png_adaptive.hpp); same plan, same coder.
// Same image -> same bytes.
#include <hip/hip_runtime.h>

#include "deflate.hpp"
#include "device.hpp"
#include "grey.h"
#include "png_adaptive.hpp"

namespace rr {

namespace {

// Byte q < C W of an image row before the filter. C = 4: RGBA as stored; 3:
// R, G, B; 1: the grey code.
template <int C>
__device__ __forceinline__ uint32_t png8_byte(const uint8_t* __restrict__ src, uint32_t q) {
    if constexpr (C == 4) return src[q];
    else if constexpr (C == 3) return src[4u * (q / 3u) + q % 3u];
    else return grey8(src[4u * q], src[4u * q + 1u], src[4u * q + 2u]);
}

template <int C>
struct Png8Front {
    const uint8_t* __restrict__ rgba;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t, uint32_t j) const {
        const uint32_t row = j / p.stride, x = j - row * p.stride;
        uint32_t v = 1u;  // filter type Sub
        if (x > 0) {
            const uint8_t* src = rgba + (size_t)(row0 + (int)row) * ((size_t)p.W * 4);
            v = (png8_byte<C>(src, x - 1) - (x > (uint32_t)C ? png8_byte<C>(src, x - 1 - C) : 0u)) & 0xFFu;
        }
        return v;
    }
};

// The raw scanlines of the adaptive filter, read in place from the RGBA8 frame.
template <int C>
struct Png8Rows {
    const uint8_t* __restrict__ rgba;
    uint32_t W;
    __device__ __forceinline__ uint32_t operator()(uint32_t row, uint32_t q) const {
        return png8_byte<C>(rgba + (size_t)row * ((size_t)W * 4), q);
    }
};

}  // namespace

// The free distance of a grey image, where the sample and the pixel period are
// one (profiles/color_modes.md).
#ifndef RR_PNG8_Y_DIST
#define RR_PNG8_Y_DIST 0
#endif

bool png_plan(int W, int H, int C, DeflatePlan& p) {
    // a band's bit offsets (at most 16 bits a byte) stay below 2^32
    if (W <= 0 || H <= 0 || W > (1 << 20) || (C != 1 && C != 3 && C != 4)) return false;
    const bool ok = deflate_plan(W, H, (uint32_t)C * (uint32_t)W + 1u, p);
    p.dist[0] = 1u;
    p.dist[1] = C == 1 ? (uint32_t)RR_PNG8_Y_DIST : (uint32_t)C;
    p.dist[2] = p.stride <= 32768u ? p.stride : 0u;
    if (C != 4) deflate_distinct(p);  // narrow images: a row of 2 or 3 bytes
    return ok;
}

void png_encode_device(const uint8_t* d_rgba, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* host_out,
                       uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    const dim3 grid(p.nsub, p.nbands);
    if (C == 1) k_deflate_front<<<grid, 256, 0, st>>>(Png8Front<1>{d_rgba}, p, c.filt, c.adler_part);
    else if (C == 3) k_deflate_front<<<grid, 256, 0, st>>>(Png8Front<3>{d_rgba}, p, c.filt, c.adler_part);
    else k_deflate_front<<<grid, 256, 0, st>>>(Png8Front<4>{d_rgba}, p, c.filt, c.adler_part);
    deflate_bands_device(p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

void png_encode_device_adaptive(const uint8_t* d_rgba, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* ftype,
                                uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    const uint32_t W = (uint32_t)p.W;
    if (C == 1) png_adaptive_front_device<1>(Png8Rows<1>{d_rgba, W}, p, c, ftype, st);
    else if (C == 3) png_adaptive_front_device<3>(Png8Rows<3>{d_rgba, W}, p, c, ftype, st);
    else png_adaptive_front_device<4>(Png8Rows<4>{d_rgba, W}, p, c, ftype, st);
    deflate_bands_device(p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

}  // namespace rr
