// OpenEXR encode on the device: the film's means as half-float A, B, G, R
// planes, ZIP compression (zlib over chunks of 16 scanlines), so only the
// compressed chunks cross PCIe and the host writes header, offset table and
// chunk framing (image_io exr_wrap_stream). Replaces the OPEN_EXR side of
// Blender's write_still (render-timing-script.py:83-92).
//
// A chunk of `rows` scanlines holds n = 8W * rows bytes: per scanline the
// planes A, B, G, R of W halfs each. OpenEXR's ZIP preprocessing moves the
// even-indexed (low) bytes to the first n / 2 positions and the odd-indexed
// (high) bytes behind them, then replaces every byte but the first by its
// difference to its predecessor + 128. Within a half of the reordered bytes,
// position k is the sample (row k / 4W, plane k % 4W / W, x k % W).
//
//  - ExrFront: the preprocessed byte at a position, the front end of the
//    deflate coder (deflate.hpp k_deflate_front). A position converts its own
//    sample and its predecessor's.
//  - deflate.hip's stages over bands = chunks, every band a stream of its own
//    (own_stream), with the distances 1, W (the same pixel in the neighbouring
//    plane: grey pixels give equal planes) and 4W (the scanline above within a
//    half).
//  - k_exr_raw: a chunk whose zlib stream would not be smaller than n carries
//    its n unprocessed bytes; the codes stage decides, this kernel writes them.
//  - deflate.hip's scan + gather into pinned host memory.
// Same film -> same bytes.
//
// PXR24 (rr_set_exr_codec) is a third front end: Pxr24Front and pxr24_plan
// below; the raw kernels are the two here. NONE and RLE, a chunk per
// scanline and no deflate, are exr_codec.hip.
//
// FLOAT channels (Blender's "Float (Full)", rr_set_exr_depth 32) are a second
// front end of the same shape: ExrFloatFront, k_exr32_raw and exr32_plan below,
// n = 16W * rows bytes a chunk, the means' own bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "deflate.hpp"
#include "device.hpp"
#include "exr_samples.hpp"
#include "pxr24_rule.h"

namespace rr {

namespace {

constexpr int kThreads = 256;

// Byte j of a chunk as the coder sees it (exr_samples.hpp exr_pred_byte).
template <int C>
struct ExrFront {
    Film fm;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t n, uint32_t j) const {
        return exr_pred_byte<C, false>(fm, p.W, row0, n, j);
    }
};

// Raw chunks (rec mode 1): the n bytes as the file's reader expects them, unprocessed.
template <int C>
__global__ __launch_bounds__(kThreads) void k_exr_raw(Film fm, DeflatePlan p, const uint32_t* __restrict__ rec,
                                                      uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    if (rec[4 * (size_t)b] == 0u) return;
    const int row0 = b * kDeflateBandRows;
    const uint32_t n = p.raw_stride * (uint32_t)min(kDeflateBandRows, p.H - row0);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;  // sample
    if (2u * k >= n) return;
    const uint32_t h = sample_half<C>(fm, p.W, row0, k);
    uint8_t* o = out + (size_t)b * p.band_cap + 2u * k;  // band_cap is a multiple of 16
    *reinterpret_cast<uint16_t*>(o) = (uint16_t)h;
}

// ---- FLOAT channels (rr_set_exr_depth 32): the film's means as they are ----
// A chunk of `rows` scanlines holds n = 16W * rows bytes: per scanline the
// planes A, B, G, R of W little-endian floats each. After the reorder the
// first n / 2 positions alternate bytes 0 and 2 of consecutive samples, the
// second n / 2 bytes 1 and 3: position q of a half belongs to sample q / 2.

// Byte j of a FLOAT chunk as the coder sees it (exr_samples.hpp exr_pred_byte).
template <int C>
struct ExrFloatFront {
    Film fm;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t n, uint32_t j) const {
        return exr_pred_byte<C, true>(fm, p.W, row0, n, j);
    }
};

// Raw FLOAT chunks (rec mode 1): k_exr_raw with 4-byte samples.
template <int C>
__global__ __launch_bounds__(kThreads) void k_exr32_raw(Film fm, DeflatePlan p, const uint32_t* __restrict__ rec,
                                                        uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    if (rec[4 * (size_t)b] == 0u) return;
    const int row0 = b * kDeflateBandRows;
    const uint32_t n = p.raw_stride * (uint32_t)min(kDeflateBandRows, p.H - row0);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;  // sample
    if (4u * k >= n) return;                                 // n = 16W * rows: whole samples
    uint8_t* o = out + (size_t)b * p.band_cap + 4u * k;      // band_cap is a multiple of 16, n <= band_cap
    *reinterpret_cast<uint32_t*>(o) = sample_float<C>(fm, p.W, row0, k);
}

// ---- PXR24 (rr_set_exr_codec RR_EXR_CODEC_PXR24): a third front end ----
// A chunk of `rows` scanlines holds per scanline and channel one run of W
// pixels: with v the half's 16 bits (S = 2) or the float's 24-bit form
// (pxr24_rule.h, S = 3) and p the value of the pixel before (0 at x = 0), the
// difference d = v - p as S planes of W bytes, the most significant first. A
// scanline takes S C W bytes. A raw chunk is the file's own halfs or floats
// (k_exr_raw, k_exr32_raw; DeflatePlan::raw_stride).
template <int C, bool Full>
struct Pxr24Front {
    Film fm;
    __device__ __forceinline__ uint32_t value(int W, int row0, uint32_t k) const {
        if constexpr (Full) return float24_bits(sample_float<C>(fm, W, row0, k));
        else return sample_half<C>(fm, W, row0, k);
    }
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t, uint32_t j) const {
        constexpr uint32_t S = Full ? 3u : 2u;
        const uint32_t W = (uint32_t)p.W, run = S * W;
        const uint32_t row = j / p.stride, r = j - row * p.stride;
        const uint32_t ch = r / run, q = r - ch * run;
        const uint32_t plane = q / W, x = q - plane * W;
        const uint32_t k = (row * (uint32_t)C + ch) * W + x;
        uint32_t d = value(p.W, row0, k);
        if (x > 0) d -= value(p.W, row0, k - 1u);
        return (d >> (8u * (S - 1u - plane))) & 0xFFu;
    }
};

}  // namespace

// The free distance of a one-channel (Y) chunk, where two of the three
// coincide (profiles/color_modes.md).
#ifndef RR_EXR_Y_DIST
#define RR_EXR_Y_DIST 0
#endif
#ifndef RR_EXR32_Y_DIST
#define RR_EXR32_Y_DIST 0
#endif

bool exr_plan(int W, int H, int C, DeflatePlan& p) {
    // a band's bit offsets (at most 16 bits a byte, 128 W bytes) stay below 2^32
    if (W <= 0 || H <= 0 || W > (1 << 19) || (C != 1 && C != 3 && C != 4)) return false;
    const bool ok = deflate_plan(W, H, 2u * (uint32_t)C * (uint32_t)W, p);
    const uint32_t w = (uint32_t)W, cw = (uint32_t)C * w;
    // 1; W: the same pixel in the neighbouring plane; C W: the scanline above
    // within a half. One plane: the last two are one, and no distance is listed twice.
    p.dist[0] = 1u;
    p.dist[1] = w <= 32768u ? w : 0u;
    const uint32_t free_y = (uint32_t)(RR_EXR_Y_DIST);  // may name w
    p.dist[2] = C == 1 ? (free_y <= 32768u ? free_y : 0u) : cw <= 32768u ? cw : 0u;
    if (C != 4) deflate_distinct(p);  // narrow images: W = 1, 2
    p.own_stream = 1;
    return ok;
}

// Which of the four candidate distances of a FLOAT chunk (1, 2, 2W, 8W) the
// coder's three leave out (profiles/exr32_device.md).
#ifndef RR_EXR32_DROP
#define RR_EXR32_DROP 0
#endif

bool exr32_plan(int W, int H, int C, DeflatePlan& p) {
    // a band's bit offsets (at most 16 bits a byte, 256 W bytes) stay below 2^30, as exr_plan's
    if (W <= 0 || H <= 0 || W > (1 << 18) || (C != 1 && C != 3 && C != 4)) return false;
    const bool ok = deflate_plan(W, H, 4u * (uint32_t)C * (uint32_t)W, p);
    const uint32_t w = (uint32_t)W;
    // 1; 2: the same byte of the previous sample (a flat area has period 2
    // after the predictor); 2W: the same pixel in the neighbouring plane; 2C W:
    // the scanline above within a half
    const uint32_t cand[4] = {1u, 2u, 2u * w, 2u * (uint32_t)C * w};
    int k = 0;
    for (int i = 0; i < 4; ++i)
        if (i != RR_EXR32_DROP) p.dist[k++] = cand[i] <= 32768u ? cand[i] : 0u;
    const uint32_t free_y = (uint32_t)(RR_EXR32_Y_DIST);  // may name w
    if (C == 1) p.dist[2] = free_y <= 32768u ? free_y : 0u;  // 2W twice: the freed slot
    if (C != 4) deflate_distinct(p);  // narrow images: W = 1
    p.own_stream = 1;
    return ok;
}

bool pxr24_plan(int W, int H, int C, int depth, DeflatePlan& p) {
    // the ranges of the ZIP coder at the same depth
    const bool full = depth == 32;
    if (W <= 0 || H <= 0 || W > (full ? 1 << 18 : 1 << 19) || (C != 1 && C != 3 && C != 4)) return false;
    const uint32_t w = (uint32_t)W, cw = (uint32_t)C * w;
    const uint32_t stride = (full ? 3u : 2u) * cw;
    const bool ok = deflate_plan(W, H, stride, p, (full ? 4u : 2u) * cw);
    // 1; W: the next byte plane of the same run; the row's stride: the scanline above
    p.dist[0] = 1u;
    p.dist[1] = w <= 32768u ? w : 0u;
    p.dist[2] = stride <= 32768u ? stride : 0u;
    deflate_distinct(p);  // narrow images: W = 1
    p.own_stream = 1;
    return ok;
}

size_t exr_stream_max_bytes(const DeflatePlan& p) { return (size_t)p.raw_stride * (size_t)p.H; }

namespace {

template <int C>
void exr_launch(const Film& fm, bool full, bool pxr24, const DeflatePlan& p, const DeflateBufs& c, hipStream_t st) {
    const dim3 front(p.nsub, p.nbands);
    if (pxr24 && full) k_deflate_front<<<front, 256, 0, st>>>(Pxr24Front<C, true>{fm}, p, c.filt, c.adler_part);
    else if (pxr24) k_deflate_front<<<front, 256, 0, st>>>(Pxr24Front<C, false>{fm}, p, c.filt, c.adler_part);
    else if (full) k_deflate_front<<<front, 256, 0, st>>>(ExrFloatFront<C>{fm}, p, c.filt, c.adler_part);
    else k_deflate_front<<<front, 256, 0, st>>>(ExrFront<C>{fm}, p, c.filt, c.adler_part);
    deflate_bands_device(p, c, st);
    const uint32_t raw_full = p.raw_stride * (uint32_t)std::min(p.H, kDeflateBandRows);  // band_full but for PXR24 FLOAT
    const dim3 grid((raw_full / (full ? 4 : 2) + kThreads - 1) / kThreads, p.nbands);
    if (full) k_exr32_raw<C><<<grid, kThreads, 0, st>>>(fm, p, c.rec, c.out);
    else k_exr_raw<C><<<grid, kThreads, 0, st>>>(fm, p, c.rec, c.out);
}

void exr_encode(const Film& fm, bool full, bool pxr24, int C, const DeflatePlan& p, uint32_t* scratch,
                uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    if (C == 1) exr_launch<1>(fm, full, pxr24, p, c, st);
    else if (C == 3) exr_launch<3>(fm, full, pxr24, p, c, st);
    else exr_launch<4>(fm, full, pxr24, p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

}  // namespace

void exr_encode_device(const float4* d_film, float inv_spp, int alpha_one, int C, const DeflatePlan& p,
                       uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    exr_encode(Film{d_film, inv_spp, alpha_one}, false, false, C, p, scratch, host_out, host_tab, st);
}

void exr32_encode_device(const float4* d_film, float inv_spp, int alpha_one, int C, const DeflatePlan& p,
                         uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    exr_encode(Film{d_film, inv_spp, alpha_one}, true, false, C, p, scratch, host_out, host_tab, st);
}

void pxr24_encode_device(const float4* d_film, float inv_spp, int alpha_one, int C, int depth, const DeflatePlan& p,
                         uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    exr_encode(Film{d_film, inv_spp, alpha_one}, depth == 32, true, C, p, scratch, host_out, host_tab, st);
}

}  // namespace rr
