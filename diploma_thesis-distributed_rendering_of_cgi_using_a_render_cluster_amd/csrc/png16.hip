// 16-bit PNG encode on the device: the film's display-referred image as RGBA
// with 16-bit samples, quantised from the float values after exposure and view
// transform (the 8-bit image is not involved), deflated by deflate.hip, so
// only the zlib stream crosses PCIe and the host writes the chunk framing
// (image_io png_wrap_stream, depth 16). Replaces Blender's
// image_settings.color_depth = '16' behind write_still
// (render-timing-script.py:83-92).
//
// A row is 8W + 1 filtered bytes: filter type 1 (Sub), then per pixel R, G, B,
// A as big-endian 16-bit samples, each byte less the byte 8 positions (one
// pixel) before it. A = 65535. With rr_set_color_mode the pixel is R, G, B
// (rows of 6W + 1 bytes) or one grey sample (2W + 1), the filter distance the
// pixel's size.
//
//  - Png16Sub: the filtered byte at a position, the front end of the deflate
//    coder (deflate.hpp k_deflate_front). A position computes its own sample
//    and its left neighbour's. Per sample, in the
//    operation order of paths.hpp tonemap / view.hip k_view:
//    c = sum * inv_spp * exposure_scale, then
//      Standard: quantize16(srgb_oetf16(clamp(c, 0, 1)))
//      Raw:      quantize16(clamp(c, 0, 1))
//      Filmic, Filmic Log, False Color: quantize16(filmic_display(c)) (the
//                quantiser clamps, as at 8 bits)
//    and with a display gamma other than 1, display_gamma of the value before
//    quantize16 (and before the BW luma), for every view;
//    with contraction off, so a host restatement gives the same bits
//    (tests/png16_reader.py, tests/view_settings.py).
//  - deflate.hip's stages over the bands of one zlib stream with the stored
//    fallback, with the distances
//    2 (equal neighbouring samples: grey pixels, and every zero run), 8 (the
//    pixel period) and 8W + 1 (the filtered row above).
//  - deflate.hip's scan + gather into pinned host memory.
// With rr_set_png_compression 0 .. 100 a row takes libpng's adaptive filter
// instead (png_filter.h). A raw byte costs a view-transform evaluation and an
// adaptive row needs each under five filters with three neighbours, so
// k_png16_raw writes the raw big-endian scanlines once (every sample evaluated
// once, by sample16 / grey16 as above); k_png_pick and PngAdaptiveFront
// (png_adaptive.hpp) read those bytes. Same plan, same coder.
// Same film -> same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "deflate.hpp"
#include "device.hpp"
#include "grey.h"
#include "png_adaptive.hpp"
#include "view_filmic.h"

namespace rr {

namespace {

// The third match distance, 1 or 2 (profiles/png16_device.md).
#ifndef RR_PNG16_DIST3
#define RR_PNG16_DIST3 2
#endif

// The display-referred value of one channel's film sum (Standard and Raw):
// mean, exposure, clamp, view transform.
__device__ __forceinline__ float display1(const Png16Front& f, float a) {
    const float c = a * f.inv_spp * f.exposure_scale;
    float v = fminf(fmaxf(c, 0.0f), 1.0f);
    if (f.view_transform == 0) v = srgb_oetf16(v, f.srgb16);
    return v;
}

// X, below: the front end of a frame whose settings go beyond Standard, Raw
// and Filmic at display gamma 1 (png16_extended): the other views of the
// Filmic family and the display gamma are compiled into it alone, so the
// plain one keeps the instructions and registers it had before them.

// The three display-referred values of a film sum through the Filmic family's chain.
template <bool X>
__device__ __forceinline__ void display_filmic(const Png16Front& f, float4 acc, float d[3]) {
    const float c[3] = {acc.x * f.inv_spp * f.exposure_scale, acc.y * f.inv_spp * f.exposure_scale,
                        acc.z * f.inv_spp * f.exposure_scale};
    filmic_display(f.filmic, X ? f.view_transform : RR_VIEW_FILMIC, c, d);
    if (X && f.filmic.inv_gamma != 0.0f)
        for (int k = 0; k < 3; ++k) d[k] = display_gamma(d[k], f.filmic.inv_gamma);
}

// display1 and the display gamma.
template <bool X>
__device__ __forceinline__ float display1g(const Png16Front& f, float a) {
    const float v = display1(f, a);
    if (X && f.filmic.inv_gamma != 0.0f) return display_gamma(v, f.filmic.inv_gamma);
    return v;
}

// The 16-bit sample of channel ch (0 R, 1 G, 2 B) of a film sum.
template <bool X>
__device__ __forceinline__ uint32_t sample16(const Png16Front& f, float4 acc, uint32_t ch) {
    if (X && f.alpha_mask && acc.w == 0.0f) return 0u;  // outside an uncropped region: black, whatever the view
    if (f.view_transform >= RR_VIEW_FILMIC) {  // the Filmic family
        float d[3];
        display_filmic<X>(f, acc, d);
        return quantize16(ch == 0 ? d[0] : ch == 1 ? d[1] : d[2]);
    }
    return quantize16(display1g<X>(f, ch == 0 ? acc.x : ch == 1 ? acc.y : acc.z));
}

// The 16-bit grey sample of a film sum (Blender's BW colour mode): Rec.709 luma
// of the three display-referred values, products and sums rounded one by one.
template <bool X>
__device__ __forceinline__ uint32_t grey16(const Png16Front& f, float4 acc) {
    if (X && f.alpha_mask && acc.w == 0.0f) return 0u;
    float d[3];
    if (f.view_transform >= RR_VIEW_FILMIC) {  // the Filmic family
        display_filmic<X>(f, acc, d);
    } else {
        d[0] = display1g<X>(f, acc.x);
        d[1] = display1g<X>(f, acc.y);
        d[2] = display1g<X>(f, acc.z);
    }
    return quantize16(luma709(d[0], d[1], d[2]));
}

// Byte q < 2C W of an image row before the filter. C = 4: R, G, B, A = 65535;
// 3: R, G, B; 1: grey.
template <int C, bool X>
__device__ __forceinline__ uint32_t row_byte(const Png16Front& f, const float4* __restrict__ row, uint32_t q) {
    uint32_t s;
    if constexpr (C == 4) {
        const uint32_t ch = (q >> 1) & 3u;
        if (ch == 3u) return (X && f.alpha_mask && row[q >> 3].w == 0.0f) ? 0u : 0xFFu;  // A = 65535, or the mask's 0
        s = sample16<X>(f, row[q >> 3], ch);
    } else if constexpr (C == 3) {
        const uint32_t k = q >> 1, px = k / 3u;
        s = sample16<X>(f, row[px], k - 3u * px);
    } else {
        s = grey16<X>(f, row[q >> 1]);
    }
    return (q & 1u) ? s & 0xFFu : s >> 8;
}

// Byte j of a band: filter type 1 (Sub) in front of every row of differences.
template <int C, bool X = false>
struct Png16Sub {
    Png16Front f;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t, uint32_t j) const {
        const uint32_t row = j / p.stride, x = j - row * p.stride;
        if (x == 0) return 1u;
        const float4* src = f.film + (size_t)(row0 + (int)row) * (size_t)p.W;
        uint32_t v = row_byte<C, X>(f, src, x - 1u);
        if (x > 2u * C) v = (v - row_byte<C, X>(f, src, x - 1u - 2u * C)) & 0xFFu;
        return v;
    }
};

// The raw scanlines of a frame, 2C W bytes a row, one pixel a lane: the
// samples row_byte gives, each evaluated once.
template <int C, bool X>
__global__ __launch_bounds__(256) void k_png16_raw(Png16Front f, size_t npix, uint8_t* __restrict__ raw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const float4 acc = f.film[i];
    auto be = [](uint32_t s) { return (s >> 8) | ((s & 0xFFu) << 8); };  // the sample's two bytes, high first
    if constexpr (C == 1) {
        reinterpret_cast<uint16_t*>(raw)[i] = (uint16_t)be(grey16<X>(f, acc));
    } else {
        const uint32_t r = be(sample16<X>(f, acc, 0u)), g = be(sample16<X>(f, acc, 1u)), b = be(sample16<X>(f, acc, 2u));
        if constexpr (C == 3) {
            uint16_t* o = reinterpret_cast<uint16_t*>(raw) + 3 * i;
            o[0] = (uint16_t)r;
            o[1] = (uint16_t)g;
            o[2] = (uint16_t)b;
        } else {
            reinterpret_cast<uint2*>(raw)[i] = make_uint2(r | (g << 16), b | ((X && f.alpha_mask && acc.w == 0.0f) ? 0u : 0xFFFF0000u));  // A = 65535, or the mask's 0
        }
    }
}

// Whether a frame's settings need the extended front end.
bool png16_extended(const Png16Front& f) {
    return f.view_transform > RR_VIEW_FILMIC || f.filmic.inv_gamma != 0.0f || f.alpha_mask != 0;
}

}  // namespace

// The free distance of a grey image, where the sample and the pixel period are
// one (profiles/color_modes.md).
#ifndef RR_PNG16_Y_DIST
#define RR_PNG16_Y_DIST 0
#endif

bool png16_plan(int W, int H, int C, DeflatePlan& p) {
    // a band's bit offsets (at most 16 bits a byte, 128 W + 16 bytes) stay below 2^32
    if (W <= 0 || H <= 0 || W > (1 << 19) || (C != 1 && C != 3 && C != 4)) return false;
    const bool ok = deflate_plan(W, H, 2u * (uint32_t)C * (uint32_t)W + 1u, p);
    p.dist[0] = RR_PNG16_DIST3;
    p.dist[1] = C == 1 ? (uint32_t)RR_PNG16_Y_DIST : 2u * (uint32_t)C;
    p.dist[2] = p.stride <= 32768u ? p.stride : 0u;
    if (C != 4) deflate_distinct(p);  // narrow images: a row of 3 bytes
    p.own_stream = 0;
    return ok;
}

void png16_encode_device(const Png16Front& f, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* host_out,
                         uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    const dim3 grid(p.nsub, p.nbands);
    if (png16_extended(f)) {
        if (C == 1) k_deflate_front<<<grid, 256, 0, st>>>(Png16Sub<1, true>{f}, p, c.filt, c.adler_part);
        else if (C == 3) k_deflate_front<<<grid, 256, 0, st>>>(Png16Sub<3, true>{f}, p, c.filt, c.adler_part);
        else k_deflate_front<<<grid, 256, 0, st>>>(Png16Sub<4, true>{f}, p, c.filt, c.adler_part);
    } else if (C == 1) k_deflate_front<<<grid, 256, 0, st>>>(Png16Sub<1>{f}, p, c.filt, c.adler_part);
    else if (C == 3) k_deflate_front<<<grid, 256, 0, st>>>(Png16Sub<3>{f}, p, c.filt, c.adler_part);
    else k_deflate_front<<<grid, 256, 0, st>>>(Png16Sub<4>{f}, p, c.filt, c.adler_part);
    deflate_bands_device(p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

void png16_encode_device_adaptive(const Png16Front& f, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* raw,
                                  uint8_t* ftype, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    const size_t npix = (size_t)p.W * (size_t)p.H;  // < 2^30: the plan's stream is below 2 GB
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (png16_extended(f)) {
        if (C == 1) k_png16_raw<1, true><<<grid, 256, 0, st>>>(f, npix, raw);
        else if (C == 3) k_png16_raw<3, true><<<grid, 256, 0, st>>>(f, npix, raw);
        else k_png16_raw<4, true><<<grid, 256, 0, st>>>(f, npix, raw);
    } else if (C == 1) k_png16_raw<1, false><<<grid, 256, 0, st>>>(f, npix, raw);
    else if (C == 3) k_png16_raw<3, false><<<grid, 256, 0, st>>>(f, npix, raw);
    else k_png16_raw<4, false><<<grid, 256, 0, st>>>(f, npix, raw);
    const PngRawRows rows{raw, p.stride - 1u};
    if (C == 1) png_adaptive_front_device<2>(rows, p, c, ftype, st);
    else if (C == 3) png_adaptive_front_device<6>(rows, p, c, ftype, st);
    else png_adaptive_front_device<8>(rows, p, c, ftype, st);
    deflate_bands_device(p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

}  // namespace rr
