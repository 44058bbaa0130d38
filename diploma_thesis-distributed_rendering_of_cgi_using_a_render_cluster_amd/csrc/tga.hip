// TARGA encode on the device: the body of a "TARGA" / "TARGA_RAW" file from the
// RGBA8 frame, so only the file's bytes cross PCIe and the host writes the
// 18-byte header (image_io tga_header_bytes). See tga.hpp, and tga_rule.h for
// the packet rule, which the host encoder (image_io encode_tga) states as a
// walk over the runs and the device packer (rle_device.hpp) as bit operations
// on ballots.
//
// "TARGA": k_tga_size (a workgroup per file row: every pixel's offset in its
// coded row and its packet's header byte, the row's length) -> k_tga_scan (the
// rows' offsets in file order, the body's length) -> k_tga_emit (a thread per
// pixel stores its bytes) -> k_body_gather (the dense body to pinned host
// memory, 16 bytes a thread). "TARGA_RAW": k_tga_raw -> k_body_gather.
// Integers only, no atomics, no workgroup waits for another; order comes from
// the launches. Same image -> same bytes.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "grey.h"
#include "rle_device.hpp"
#include "tga.hpp"
#include "tga_rule.h"
#include "wg_scan.hpp"

namespace rr {

namespace {

static_assert(kTgaChunk == kBodyChunk, "the packer's step");
constexpr int kThreads = kBodyChunk;
constexpr int kWaves = kBodyWaves;
static_assert(tga_row_max_bytes(kTgaMaxSide, 4) <= kRecOffset, "a row offset fits the record");

// What two pixels compare by: all C bytes of the file's pixel. v: the RGBA8
// pixel as one word (R in the low byte).
template <int C>
__device__ __forceinline__ uint32_t tga_key(uint32_t v) {
    if constexpr (C == 4) return v;
    else if constexpr (C == 3) return v & 0x00FFFFFFu;
    else return grey8(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u);
}

// The pixel's C bytes in file order: B, G, R(, A) or the grey code.
template <int C>
__device__ __forceinline__ void tga_put(uint8_t* __restrict__ o, uint32_t v) {
    if constexpr (C == 1) {
        o[0] = (uint8_t)tga_key<1>(v);
    } else {
        o[0] = (uint8_t)(v >> 16);
        o[1] = (uint8_t)(v >> 8);
        o[2] = (uint8_t)v;
        if constexpr (C == 4) o[3] = (uint8_t)(v >> 24);
    }
}

// One workgroup per file row f (image row H - 1 - f): rle_pack_row over the
// row's pixels, equal when all C bytes are.
template <int C>
__global__ __launch_bounds__(kThreads) void k_tga_size(const uint8_t* __restrict__ rgba, int W, int H,
                                                       uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                       uint32_t* __restrict__ row_bytes) {
    const int f = blockIdx.x;
    if (f >= H) return;
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(rgba) + (size_t)(H - 1 - f) * (size_t)W;
    const auto eq = [row, W](int j) {
        if (j <= 0 || j >= W) return false;
        return tga_key<C>(row[j]) == tga_key<C>(row[j - 1]);
    };
    const uint32_t bytes = rle_pack_row<TgaRle<C>>(eq, W, rec, hdr, (size_t)f * (size_t)W);
    if (threadIdx.x == 0) row_bytes[f] = bytes;
}

// The rows' lengths, in file order, into their offsets in the body and the
// body's length. One workgroup; a body stays below 2^31 bytes (tga_plan).
__global__ __launch_bounds__(kThreads) void k_tga_scan(int H, const uint32_t* __restrict__ row_bytes,
                                                       uint32_t* __restrict__ row_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t ws[kWaves];
    uint32_t base = 0;
    for (int r0 = 0; r0 < H; r0 += kThreads) {
        const int r = r0 + (int)threadIdx.x;
        uint32_t v = r < H ? row_bytes[r] : 0u;
        const uint32_t sum = wg_exclusive_scan<kWaves>(v, ws);
        if (r < H) row_off[r] = base + v;
        base += sum;
    }
    if (threadIdx.x == 0) total[0] = base;
}

// A thread per pixel: a packet's first pixel stores the header byte, and every
// literal pixel and every run packet's first pixel its C bytes, at the row's
// offset + the pixel's offset in the row. cap: the body's bound, which the
// rule keeps (a store beyond it is dropped, and the host refuses the length).
template <int C>
__global__ __launch_bounds__(kThreads) void k_tga_emit(const uint8_t* __restrict__ rgba, int W, int H,
                                                       const uint32_t* __restrict__ rec,
                                                       const uint8_t* __restrict__ hdr,
                                                       const uint32_t* __restrict__ row_off, uint32_t cap,
                                                       uint8_t* __restrict__ body) {
    const int f = blockIdx.y, x = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (x >= W || f >= H) return;
    const size_t at = (size_t)f * (size_t)W + (size_t)x;
    const uint32_t r = rec[at];
    if (!(r & kRecWrites)) return;
    const bool first = (r & kRecFirst) != 0u;
    uint64_t pos = (uint64_t)row_off[f] + (r & kRecOffset);
    if (pos + (first ? 1u : 0u) + (uint32_t)C > (uint64_t)cap) return;
    if (first) body[pos++] = hdr[at];
    const uint32_t v = reinterpret_cast<const uint32_t*>(rgba)[(size_t)(H - 1 - f) * (size_t)W + (size_t)x];
    tga_put<C>(body + pos, v);
}

// "TARGA_RAW": a thread per pixel stores its C bytes, rows bottom first.
template <int C>
__global__ __launch_bounds__(kThreads) void k_tga_raw(const uint8_t* __restrict__ rgba, int W, int H,
                                                      uint8_t* __restrict__ body, uint32_t* __restrict__ total) {
    const int f = blockIdx.y, x = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (x >= W || f >= H) return;
    if (x == 0 && f == 0) total[0] = (uint32_t)W * (uint32_t)H * (uint32_t)C;
    const uint32_t v = reinterpret_cast<const uint32_t*>(rgba)[(size_t)(H - 1 - f) * (size_t)W + (size_t)x];
    tga_put<C>(body + ((size_t)f * (size_t)W + (size_t)x) * (size_t)C, v);
}

}  // namespace

bool tga_plan(int W, int H, int C, bool rle, TgaPlan& p) {
    const uint64_t cap = tga_body_max_bytes(W, H, C, rle);
    p = TgaPlan{W, H, C, rle, (uint32_t)cap};
    return cap != 0;
}

TgaBufs tga_carve(const TgaPlan& p, uint32_t* base) {
    TgaBufs b{};
    Carver c{base};
    const size_t npix = (size_t)p.W * (size_t)p.H;
    b.body = reinterpret_cast<uint8_t*>(c.take(up16(p.body_cap) + 16));
    b.total = c.take(16);
    if (p.rle) {
        b.rec = c.take(npix * 4);
        b.row_bytes = c.take((size_t)p.H * 4);
        b.row_off = c.take((size_t)p.H * 4);
        b.hdr = reinterpret_cast<uint8_t*>(c.take(npix));
    }
    b.words = c.words;
    return b;
}

size_t tga_scratch_words(const TgaPlan& p) { return tga_carve(p, nullptr).words; }

void tga_encode_device(const uint8_t* d_rgba, const TgaPlan& p, uint32_t* scratch, uint8_t* host_out, hipStream_t st) {
    const TgaBufs b = tga_carve(p, scratch);
    const int W = p.W, H = p.H;
    const dim3 pixels((unsigned)((W + kThreads - 1) / kThreads), (unsigned)H);
    if (p.rle) {
        if (p.C == 1) k_tga_size<1><<<dim3((unsigned)H), kThreads, 0, st>>>(d_rgba, W, H, b.rec, b.hdr, b.row_bytes);
        else if (p.C == 3) k_tga_size<3><<<dim3((unsigned)H), kThreads, 0, st>>>(d_rgba, W, H, b.rec, b.hdr, b.row_bytes);
        else k_tga_size<4><<<dim3((unsigned)H), kThreads, 0, st>>>(d_rgba, W, H, b.rec, b.hdr, b.row_bytes);
        k_tga_scan<<<1, kThreads, 0, st>>>(H, b.row_bytes, b.row_off, b.total);
        if (p.C == 1) k_tga_emit<1><<<pixels, kThreads, 0, st>>>(d_rgba, W, H, b.rec, b.hdr, b.row_off, p.body_cap, b.body);
        else if (p.C == 3) k_tga_emit<3><<<pixels, kThreads, 0, st>>>(d_rgba, W, H, b.rec, b.hdr, b.row_off, p.body_cap, b.body);
        else k_tga_emit<4><<<pixels, kThreads, 0, st>>>(d_rgba, W, H, b.rec, b.hdr, b.row_off, p.body_cap, b.body);
    } else {
        if (p.C == 1) k_tga_raw<1><<<pixels, kThreads, 0, st>>>(d_rgba, W, H, b.body, b.total);
        else if (p.C == 3) k_tga_raw<3><<<pixels, kThreads, 0, st>>>(d_rgba, W, H, b.body, b.total);
        else k_tga_raw<4><<<pixels, kThreads, 0, st>>>(d_rgba, W, H, b.body, b.total);
    }
    body_gather(b.body, b.total, p.body_cap, host_out, st);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
