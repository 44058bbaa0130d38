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
// FLOAT channels (Blender's "Float (Full)", rr_set_exr_depth 32) are a second
// front end of the same shape: ExrFloatFront, k_exr32_raw and exr32_plan below,
// n = 16W * rows bytes a chunk, the means' own bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "deflate.hpp"
#include "device.hpp"
#include "grey.h"

namespace rr {

namespace {

constexpr int kThreads = 256;

// float -> half bits: clamped to +-65504, round to nearest even, subnormals kept.
__device__ __forceinline__ uint32_t half_bits(float f) {
    const uint32_t x = __float_as_uint(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    uint32_t a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return sign | 0x7E00u;  // NaN
    a = min(a, 0x477FE000u);                     // 65504
    if (a >= 0x38800000u) {                      // >= 2^-14: a normal half
        a -= 112u << 23;
        a += 0xFFFu + ((a >> 13) & 1u);
        return sign | (a >> 13);
    }
    const uint32_t e = a >> 23;
    if (e < 102u) return sign;  // < 2^-25: below half of the smallest subnormal (and 0)
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    const uint32_t s = 126u - e;  // 14 .. 24: m * 2^(e - 150) in units of 2^-24
    uint32_t h = m >> s;
    const uint32_t rem = m & ((1u << s) - 1u), mid = 1u << (s - 1u);
    if (rem > mid || (rem == mid && (h & 1u))) h += 1u;
    return sign | h;
}

struct Film {
    const float4* px;
    float inv_spp;
    int alpha_one;
};

// Mean of sample k of a band: k counts scanline by scanline, plane by plane.
// C = 4: planes A, B, G, R; C = 3: B, G, R; C = 1: Y, the Rec.709 luma of the
// means (products and sums rounded one by one, left to right).
template <int C>
__device__ __forceinline__ float sample_mean(const Film& fm, const DeflatePlan& p, int row0, uint32_t k) {
    const uint32_t W = (uint32_t)p.W, row_samples = (uint32_t)C * W;
    const uint32_t row = k / row_samples, rem = k - row * row_samples;
    const uint32_t ch = rem / W, x = rem - ch * W;
    const float4 v = fm.px[(size_t)(row0 + (int)row) * W + x];
    if constexpr (C == 4) {
        const float c = ch == 0 ? v.w : ch == 1 ? v.z : ch == 2 ? v.y : v.x;
        return (ch == 0 && fm.alpha_one) ? 1.0f : __fmul_rn(c, fm.inv_spp);
    } else if constexpr (C == 3) {
        const float c = ch == 0 ? v.z : ch == 1 ? v.y : v.x;
        return __fmul_rn(c, fm.inv_spp);
    } else {
        const float r = __fmul_rn(v.x, fm.inv_spp), g = __fmul_rn(v.y, fm.inv_spp), b = __fmul_rn(v.z, fm.inv_spp);
        return luma709(r, g, b);
    }
}

// Half of sample k of a band.
template <int C>
__device__ __forceinline__ uint32_t sample_half(const Film& fm, const DeflatePlan& p, int row0, uint32_t k) {
    return half_bits(sample_mean<C>(fm, p, row0, k));
}

// Byte j of a band after the reorder (before the predictor).
template <int C>
__device__ __forceinline__ uint32_t reordered_byte(const Film& fm, const DeflatePlan& p, int row0, uint32_t half_n,
                                                   uint32_t j) {
    const bool hi = j >= half_n;
    const uint32_t h = sample_half<C>(fm, p, row0, hi ? j - half_n : j);
    return hi ? h >> 8 : h & 0xFFu;
}

// Byte j of a chunk as the coder sees it: reordered, less its predecessor + 128.
template <int C>
struct ExrFront {
    Film fm;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t n, uint32_t j) const {
        uint32_t v = reordered_byte<C>(fm, p, row0, n / 2, j);
        if (j > 0) v = (v - reordered_byte<C>(fm, p, row0, n / 2, j - 1) + 128u) & 0xFFu;
        return v;
    }
};

// Raw chunks (rec mode 1): the n bytes as the file's reader expects them, unprocessed.
template <int C>
__global__ __launch_bounds__(kThreads) void k_exr_raw(Film fm, DeflatePlan p, const uint32_t* __restrict__ rec,
                                                      uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    if (rec[4 * (size_t)b] == 0u) return;
    const int row0 = b * kDeflateBandRows;
    const uint32_t n = p.stride * (uint32_t)min(kDeflateBandRows, p.H - row0);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;  // sample
    if (2u * k >= n) return;
    const uint32_t h = sample_half<C>(fm, p, row0, k);
    uint8_t* o = out + (size_t)b * p.band_cap + 2u * k;  // band_cap is a multiple of 16
    *reinterpret_cast<uint16_t*>(o) = (uint16_t)h;
}

// ---- FLOAT channels (rr_set_exr_depth 32): the film's means as they are ----
// A chunk of `rows` scanlines holds n = 16W * rows bytes: per scanline the
// planes A, B, G, R of W little-endian floats each. After the reorder the
// first n / 2 positions alternate bytes 0 and 2 of consecutive samples, the
// second n / 2 bytes 1 and 3: position q of a half belongs to sample q / 2.

// Bits of sample k of a band: the mean itself, no clamp and no rounding.
template <int C>
__device__ __forceinline__ uint32_t sample_float(const Film& fm, const DeflatePlan& p, int row0, uint32_t k) {
    return __float_as_uint(sample_mean<C>(fm, p, row0, k));
}

// Byte j of a band of floats after the reorder (before the predictor).
template <int C>
__device__ __forceinline__ uint32_t reordered_byte32(const Film& fm, const DeflatePlan& p, int row0, uint32_t half_n,
                                                     uint32_t j) {
    const bool hi = j >= half_n;
    const uint32_t q = hi ? j - half_n : j;
    const uint32_t bits = sample_float<C>(fm, p, row0, q >> 1);
    return (bits >> (16u * (q & 1u) + (hi ? 8u : 0u))) & 0xFFu;
}

// Byte j of a FLOAT chunk as the coder sees it: reordered, less its predecessor + 128.
template <int C>
struct ExrFloatFront {
    Film fm;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t n, uint32_t j) const {
        uint32_t v = reordered_byte32<C>(fm, p, row0, n / 2, j);
        if (j > 0) v = (v - reordered_byte32<C>(fm, p, row0, n / 2, j - 1) + 128u) & 0xFFu;
        return v;
    }
};

// Raw FLOAT chunks (rec mode 1): k_exr_raw with 4-byte samples.
template <int C>
__global__ __launch_bounds__(kThreads) void k_exr32_raw(Film fm, DeflatePlan p, const uint32_t* __restrict__ rec,
                                                        uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    if (rec[4 * (size_t)b] == 0u) return;
    const int row0 = b * kDeflateBandRows;
    const uint32_t n = p.stride * (uint32_t)min(kDeflateBandRows, p.H - row0);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;  // sample
    if (4u * k >= n) return;                                 // n = 16W * rows: whole samples
    uint8_t* o = out + (size_t)b * p.band_cap + 4u * k;      // band_cap is a multiple of 16, n <= band_cap
    *reinterpret_cast<uint32_t*>(o) = sample_float<C>(fm, p, row0, k);
}

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

size_t exr_stream_max_bytes(const DeflatePlan& p) { return (size_t)p.stride * (size_t)p.H; }

namespace {

template <int C>
void exr_launch(const Film& fm, bool full, const DeflatePlan& p, const DeflateBufs& c, hipStream_t st) {
    if (full) k_deflate_front<<<dim3(p.nsub, p.nbands), 256, 0, st>>>(ExrFloatFront<C>{fm}, p, c.filt, c.adler_part);
    else k_deflate_front<<<dim3(p.nsub, p.nbands), 256, 0, st>>>(ExrFront<C>{fm}, p, c.filt, c.adler_part);
    deflate_bands_device(p, c, st);
    const dim3 grid((p.band_full / (full ? 4 : 2) + kThreads - 1) / kThreads, p.nbands);
    if (full) k_exr32_raw<C><<<grid, kThreads, 0, st>>>(fm, p, c.rec, c.out);
    else k_exr_raw<C><<<grid, kThreads, 0, st>>>(fm, p, c.rec, c.out);
}

void exr_encode(const Film& fm, bool full, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* host_out,
                uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    if (C == 1) exr_launch<1>(fm, full, p, c, st);
    else if (C == 3) exr_launch<3>(fm, full, p, c, st);
    else exr_launch<4>(fm, full, p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

}  // namespace

void exr_encode_device(const float4* d_film, float inv_spp, bool alpha_one, int C, const DeflatePlan& p,
                       uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    exr_encode(Film{d_film, inv_spp, alpha_one ? 1 : 0}, false, C, p, scratch, host_out, host_tab, st);
}

void exr32_encode_device(const float4* d_film, float inv_spp, bool alpha_one, int C, const DeflatePlan& p,
                         uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    exr_encode(Film{d_film, inv_spp, alpha_one ? 1 : 0}, true, C, p, scratch, host_out, host_tab, st);
}

}  // namespace rr
