// OpenEXR encode on the device with a chunk per scanline: the codecs NONE and
// RLE of rr_set_exr_codec (Blender's image_settings.exr_codec behind
// write_still, render-timing-script.py:83-92). Only the chunks' payloads cross
// PCIe; the host writes header, offset table and chunk framing (image_io
// exr_wrap_rows). See exr_codec.hpp, and exr_rle_rule.h for the packet rule.
//
// A scanline holds n = 2 C W (HALF) or 4 C W (FLOAT) bytes: the planes A, B,
// G, R / B, G, R / Y of W samples each (exr_samples.hpp).
//
// NONE: k_exr_rows_raw (a thread per sample stores its half or float, what
// exr.hip's raw kernels do for a chunk that goes raw, over every row) ->
// k_body_gather.
// RLE: k_exr_rle_size (a workgroup per scanline: rle_pack_row over the
// scanline's n predicted bytes, each a pure function of two neighbouring
// samples, nothing staged) -> k_exr_rle_scan (a scanline whose packets are
// not shorter than n goes raw; the scanlines' offsets by min(packed, n), so
// the dense body is bounded by the raw size; the host's table) ->
// k_exr_rle_emit (a thread per byte: a packet's first byte stores the header,
// every literal byte and every run packet's first byte its value; a raw
// scanline's thread its unprocessed byte) -> k_body_gather.
// Integers only behind the samples, no atomics, no workgroup waits for
// another; order comes from the launches. Same film -> same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "deflate.hpp"
#include "device.hpp"
#include "exr_codec.hpp"
#include "exr_rle_rule.h"
#include "exr_samples.hpp"
#include "rle_device.hpp"
#include "wg_scan.hpp"

namespace rr {

namespace {

constexpr int kThreads = kBodyChunk;
constexpr int kWaves = kBodyWaves;
static_assert(exr_rle_row_max_bytes(kExrRleMaxRowBytes) <= kRecOffset, "a row offset fits the record");

// Byte j of scanline y as the file's reader expects it, unprocessed.
template <int C, bool Full>
__device__ __forceinline__ uint32_t raw_byte(const Film& fm, int W, int y, uint32_t j) {
    if constexpr (Full) return (sample_float<C>(fm, W, y, j >> 2) >> (8u * (j & 3u))) & 0xFFu;
    else return (sample_half<C>(fm, W, y, j >> 1) >> (8u * (j & 1u))) & 0xFFu;
}

// NONE: a thread per sample of the image stores its half or float.
template <int C, bool Full>
__global__ __launch_bounds__(kThreads) void k_exr_rows_raw(Film fm, int W, uint32_t samples, uint8_t* __restrict__ body,
                                                           uint32_t* __restrict__ total) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= samples) return;
    if (k == 0) total[0] = samples * (Full ? 4u : 2u);
    if constexpr (Full) reinterpret_cast<uint32_t*>(body)[k] = sample_float<C>(fm, W, 0, k);
    else reinterpret_cast<uint16_t*>(body)[k] = (uint16_t)sample_half<C>(fm, W, 0, k);
}

// RLE: one workgroup per scanline y: rle_pack_row over its n predicted bytes.
template <int C, bool Full>
__global__ __launch_bounds__(kThreads) void k_exr_rle_size(Film fm, int W, int H, uint32_t n,
                                                           uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                           uint32_t* __restrict__ row_bytes) {
    const int y = blockIdx.x;
    if (y >= H) return;
    const auto eq = [fm, W, y, n](int j) {
        if (j <= 0 || (uint32_t)j >= n) return false;
        return exr_pred_byte<C, Full>(fm, W, y, n, (uint32_t)j) == exr_pred_byte<C, Full>(fm, W, y, n, (uint32_t)j - 1u);
    };
    const uint32_t bytes = rle_pack_row<ExrRle>(eq, (int)n, rec, hdr, (size_t)y * (size_t)n);
    if (threadIdx.x == 0) row_bytes[y] = bytes;
}

// The scanlines' chunk lengths (the packets', or n where those are not shorter)
// into their offsets in the body, the body's length and the host's table
// {mode, bytes}. One workgroup; a body stays below 2^31 bytes (exr_rows_plan).
__global__ __launch_bounds__(kThreads) void k_exr_rle_scan(int H, uint32_t n, const uint32_t* __restrict__ row_bytes,
                                                           uint32_t* __restrict__ row_off,
                                                           uint32_t* __restrict__ total, uint32_t* __restrict__ tab) {
    __shared__ uint32_t ws[kWaves];
    uint32_t base = 0;
    for (int r0 = 0; r0 < H; r0 += kThreads) {
        const int r = r0 + (int)threadIdx.x;
        const uint32_t packed = r < H ? row_bytes[r] : 0u;
        const uint32_t len = min(packed, n);
        uint32_t v = len;
        const uint32_t sum = wg_exclusive_scan<kWaves>(v, ws);
        if (r < H) {
            row_off[r] = base + v;
            tab[2 * (size_t)r] = packed < n ? 0u : 1u;
            tab[2 * (size_t)r + 1] = len;
        }
        base += sum;
    }
    if (threadIdx.x == 0) total[0] = base;
}

// A thread per byte of the image. cap: the body's bound, which the scan keeps
// (a store beyond it is dropped, and the host refuses the length).
template <int C, bool Full>
__global__ __launch_bounds__(kThreads) void k_exr_rle_emit(Film fm, int W, int H, uint32_t n,
                                                           const uint32_t* __restrict__ rec,
                                                           const uint8_t* __restrict__ hdr,
                                                           const uint32_t* __restrict__ row_bytes,
                                                           const uint32_t* __restrict__ row_off, uint32_t cap,
                                                           uint8_t* __restrict__ body) {
    const int y = blockIdx.x;  // rows in x: an image has more rows than a grid has y
    const uint32_t j = blockIdx.y * kThreads + threadIdx.x;
    if (j >= n || y >= H) return;
    const uint64_t row0 = row_off[y];
    if (row_bytes[y] >= n) {  // raw
        if (row0 + j < (uint64_t)cap) body[row0 + j] = (uint8_t)raw_byte<C, Full>(fm, W, y, j);
        return;
    }
    const size_t at = (size_t)y * (size_t)n + (size_t)j;
    const uint32_t r = rec[at];
    if (!(r & kRecWrites)) return;
    const bool first = (r & kRecFirst) != 0u;
    uint64_t pos = row0 + (r & kRecOffset);
    if (pos + (first ? 1u : 0u) + 1u > (uint64_t)cap) return;
    if (first) body[pos++] = hdr[at];
    body[pos] = (uint8_t)exr_pred_byte<C, Full>(fm, W, y, n, j);
}

template <int C, bool Full>
void launch(const Film& fm, const ExrRowsPlan& p, const ExrRowsBufs& b, uint32_t* host_tab, hipStream_t st) {
    const int W = p.W, H = p.H;
    const uint32_t n = p.row_bytes;
    if (!p.rle) {
        const uint32_t samples = (uint32_t)p.C * (uint32_t)W * (uint32_t)H;
        k_exr_rows_raw<C, Full><<<dim3((samples + kThreads - 1) / kThreads), kThreads, 0, st>>>(fm, W, samples, b.body,
                                                                                               b.total);
        return;
    }
    k_exr_rle_size<C, Full><<<dim3((unsigned)H), kThreads, 0, st>>>(fm, W, H, n, b.rec, b.hdr, b.row_bytes);
    k_exr_rle_scan<<<1, kThreads, 0, st>>>(H, n, b.row_bytes, b.row_off, b.total, host_tab);
    k_exr_rle_emit<C, Full><<<dim3((unsigned)H, (n + kThreads - 1) / kThreads), kThreads, 0, st>>>(
        fm, W, H, n, b.rec, b.hdr, b.row_bytes, b.row_off, p.body_cap, b.body);
}

template <bool Full>
void launch_c(const Film& fm, const ExrRowsPlan& p, const ExrRowsBufs& b, uint32_t* host_tab, hipStream_t st) {
    if (p.C == 1) launch<1, Full>(fm, p, b, host_tab, st);
    else if (p.C == 3) launch<3, Full>(fm, p, b, host_tab, st);
    else launch<4, Full>(fm, p, b, host_tab, st);
}

}  // namespace

bool exr_rows_plan(int W, int H, int C, int depth, bool rle, ExrRowsPlan& p) {
    const bool full = depth == 32;
    DeflatePlan zip;  // the ZIP coder's ranges: its stream's bound is above the raw size
    if (!(full ? exr32_plan(W, H, C, zip) : exr_plan(W, H, C, zip))) return false;
    const uint32_t row_bytes = (full ? 4u : 2u) * (uint32_t)C * (uint32_t)W;
    p = ExrRowsPlan{W, H, C, full, rle, row_bytes, row_bytes * (uint32_t)H};
    return true;
}

ExrRowsBufs exr_rows_carve(const ExrRowsPlan& p, uint32_t* base) {
    ExrRowsBufs b{};
    Carver c{base};
    b.body = reinterpret_cast<uint8_t*>(c.take(up16(p.body_cap) + 16));
    b.total = c.take(16);
    if (p.rle) {
        b.rec = c.take((size_t)p.body_cap * 4);
        b.row_bytes = c.take((size_t)p.H * 4);
        b.row_off = c.take((size_t)p.H * 4);
        b.hdr = reinterpret_cast<uint8_t*>(c.take(p.body_cap));
    }
    b.words = c.words;
    return b;
}

size_t exr_rows_scratch_words(const ExrRowsPlan& p) { return exr_rows_carve(p, nullptr).words; }

void exr_rows_encode_device(const float4* d_film, float inv_spp, int alpha_one, const ExrRowsPlan& p,
                            uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st) {
    const ExrRowsBufs b = exr_rows_carve(p, scratch);
    const Film fm{d_film, inv_spp, alpha_one};
    if (p.full) launch_c<true>(fm, p, b, host_tab, st);
    else launch_c<false>(fm, p, b, host_tab, st);
    body_gather(b.body, b.total, p.body_cap, host_out, st);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
