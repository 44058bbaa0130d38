// HDR encode on the device: the body of a Radiance RGBE file ("HDR") from the
// slot's film, so only the file's bytes cross PCIe and the host writes the text
// header (image_io hdr_header_bytes). See hdr.hpp, and hdr_rule.h for the RGBE
// rule and the scanline rule, which the host encoder (image_io encode_hdr)
// states as a walk over the runs and the device packer (rle_device.hpp) as bit
// operations on ballots.
//
// Coded rows (8 <= W <= 32767): k_hdr_quad (a thread per pixel: the quad of the
// film's means, one word) -> k_hdr_size (a workgroup per row and plane: every
// byte's offset in its coded plane and its packet's header byte, the plane's
// length) -> k_hdr_scan (a row is 4 marker bytes and its four planes: the rows'
// offsets, the body's length) -> k_hdr_emit (a thread per plane byte stores its
// byte, one lane a row the marker) -> k_body_gather (the dense body to pinned
// host memory, 16 bytes a thread). Flat rows: k_hdr_quad -> k_body_gather, the
// quads are the body. Integers only after k_hdr_quad, no atomics, no workgroup
// waits for another; order comes from the launches. Same film -> same bytes.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "grey.h"
#include "hdr.hpp"
#include "hdr_rule.h"
#include "rle_device.hpp"
#include "wg_scan.hpp"

namespace rr {

namespace {

static_assert(kHdrChunk == kBodyChunk, "the packer's step");
constexpr int kThreads = kBodyChunk;
constexpr int kWaves = kBodyWaves;
static_assert(hdr_plane_max_bytes(kHdrCodedMaxW) <= kRecOffset, "a plane offset fits the record");

// A thread per pixel: the RGBE quad of the film's means, the products formed
// as exr.hip sample_mean forms them. C = 1: the luma of the means in all three
// channels. A flat frame's quads are its body: pixel 0 stores the length.
template <int C>
__global__ __launch_bounds__(kThreads) void k_hdr_quad(const float4* __restrict__ film, float inv_spp, uint32_t npix,
                                                       uint32_t* __restrict__ quad, uint32_t* __restrict__ total,
                                                       uint32_t flat_bytes) {
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= npix) return;
    if (i == 0 && flat_bytes) total[0] = flat_bytes;
    const float4 v = film[i];
    const float r = __fmul_rn(v.x, inv_spp), g = __fmul_rn(v.y, inv_spp), b = __fmul_rn(v.z, inv_spp);
    if constexpr (C == 1) {
        const uint32_t y = __float_as_uint(luma709(r, g, b));
        quad[i] = hdr_quad(y, y, y);
    } else {
        quad[i] = hdr_quad(__float_as_uint(r), __float_as_uint(g), __float_as_uint(b));
    }
}

// One workgroup per row y and plane pl: rle_pack_row over the plane's bytes,
// byte pl of the row's quads.
__global__ __launch_bounds__(kThreads) void k_hdr_size(const uint32_t* __restrict__ quad, int W, int H,
                                                       uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                       uint32_t* __restrict__ plane_bytes) {
    const int y = blockIdx.x, pl = blockIdx.y;
    if (y >= H || pl >= 4) return;
    const uint32_t* __restrict__ row = quad + (size_t)y * (size_t)W;
    const int sh8 = 8 * pl;
    const auto eq = [row, sh8, W](int j) {
        if (j <= 0 || j >= W) return false;
        return (((row[j] ^ row[j - 1]) >> sh8) & 255u) == 0u;
    };
    const uint32_t bytes = rle_pack_row<HdrRle>(eq, W, rec, hdr, ((size_t)y * 4 + (size_t)pl) * (size_t)W);
    if (threadIdx.x == 0) plane_bytes[4 * (size_t)y + (size_t)pl] = bytes;
}

// A row's length is 4 plus its four planes: the rows' offsets in the body and
// the body's length. One workgroup; a body stays below 2^31 bytes (hdr_plan).
__global__ __launch_bounds__(kThreads) void k_hdr_scan(int H, const uint32_t* __restrict__ plane_bytes,
                                                       uint32_t* __restrict__ row_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t ws[kWaves];
    uint32_t base = 0;
    for (int r0 = 0; r0 < H; r0 += kThreads) {
        const int r = r0 + (int)threadIdx.x;
        uint32_t v = 0u;
        if (r < H) {
            const uint4 p = *reinterpret_cast<const uint4*>(plane_bytes + 4 * (size_t)r);
            v = 4u + p.x + p.y + p.z + p.w;
        }
        const uint32_t sum = wg_exclusive_scan<kWaves>(v, ws);
        if (r < H) row_off[r] = base + v;
        base += sum;
    }
    if (threadIdx.x == 0) total[0] = base;
}

// A thread per plane byte (blockIdx.x: the row; blockIdx.y: plane and step): a
// packet's first byte stores the header byte, and every literal byte and every
// run packet's first byte its value, at the row's offset + 4 + the planes
// before + the byte's offset in its plane. Plane 0's byte 0 also stores the
// row's marker 2, 2, W >> 8, W & 255. cap: the body's bound, which the rule
// keeps (a store beyond it is dropped, and the host refuses the length).
__global__ __launch_bounds__(kThreads) void k_hdr_emit(const uint32_t* __restrict__ quad, int W, int H, int steps,
                                                       const uint32_t* __restrict__ rec,
                                                       const uint8_t* __restrict__ hdr,
                                                       const uint32_t* __restrict__ plane_bytes,
                                                       const uint32_t* __restrict__ row_off, uint32_t cap,
                                                       uint8_t* __restrict__ body) {
    const int y = blockIdx.x, pl = (int)blockIdx.y / steps;
    const int x = ((int)blockIdx.y - pl * steps) * kThreads + (int)threadIdx.x;
    if (x >= W || y >= H || pl >= 4) return;
    const uint64_t row_at = row_off[y];
    if (pl == 0 && x == 0 && row_at + 4u <= (uint64_t)cap) {
        body[row_at] = 2;
        body[row_at + 1] = 2;
        body[row_at + 2] = (uint8_t)(W >> 8);
        body[row_at + 3] = (uint8_t)W;
    }
    const size_t at = ((size_t)y * 4 + (size_t)pl) * (size_t)W + (size_t)x;
    const uint32_t r = rec[at];
    if (!(r & kRecWrites)) return;
    const bool first = (r & kRecFirst) != 0u;
    uint64_t pos = row_at + 4u + (r & kRecOffset);
    for (int k = 0; k < pl; ++k) pos += plane_bytes[4 * (size_t)y + (size_t)k];
    if (pos + (first ? 2u : 1u) > (uint64_t)cap) return;
    if (first) body[pos++] = hdr[at];
    body[pos] = (uint8_t)(quad[(size_t)y * (size_t)W + (size_t)x] >> (8 * pl));
}

}  // namespace

bool hdr_plan(int W, int H, int C, HdrPlan& p) {
    const uint64_t cap = (C == 1 || C == 3) ? hdr_body_max_bytes(W, H) : 0;
    p = HdrPlan{W, H, C, hdr_row_flat(W), (uint32_t)cap};
    return cap != 0;
}

HdrBufs hdr_carve(const HdrPlan& p, uint32_t* base) {
    HdrBufs b{};
    Carver c{base};
    const size_t npix = (size_t)p.W * (size_t)p.H;
    b.quad = c.take(up16(npix * 4) + 16);
    b.total = c.take(16);
    if (!p.flat) {
        b.body = reinterpret_cast<uint8_t*>(c.take(up16(p.body_cap) + 16));
        b.rec = c.take(npix * 16);
        b.plane_bytes = c.take((size_t)p.H * 16);
        b.row_off = c.take((size_t)p.H * 4);
        b.hdr = reinterpret_cast<uint8_t*>(c.take(npix * 4));
    }
    b.words = c.words;
    return b;
}

size_t hdr_scratch_words(const HdrPlan& p) { return hdr_carve(p, nullptr).words; }

void hdr_encode_device(const float4* d_film, float inv_spp, const HdrPlan& p, uint32_t* scratch, uint8_t* host_out,
                       hipStream_t st) {
    const HdrBufs b = hdr_carve(p, scratch);
    const int W = p.W, H = p.H;
    const uint32_t npix = (uint32_t)W * (uint32_t)H;  // below 2^29: 4 W H is below 2^31 (hdr_plan)
    const dim3 pixels((npix + kThreads - 1) / kThreads);
    const uint32_t flat_bytes = p.flat ? p.body_cap : 0u;
    if (p.C == 1) k_hdr_quad<1><<<pixels, kThreads, 0, st>>>(d_film, inv_spp, npix, b.quad, b.total, flat_bytes);
    else k_hdr_quad<3><<<pixels, kThreads, 0, st>>>(d_film, inv_spp, npix, b.quad, b.total, flat_bytes);
    const uint8_t* body = reinterpret_cast<const uint8_t*>(b.quad);
    if (!p.flat) {
        const int steps = (W + kThreads - 1) / kThreads;  // at most 128: W <= 32767
        k_hdr_size<<<dim3((unsigned)H, 4u), kThreads, 0, st>>>(b.quad, W, H, b.rec, b.hdr, b.plane_bytes);
        k_hdr_scan<<<1, kThreads, 0, st>>>(H, b.plane_bytes, b.row_off, b.total);
        k_hdr_emit<<<dim3((unsigned)H, (unsigned)(4 * steps)), kThreads, 0, st>>>(b.quad, W, H, steps, b.rec, b.hdr,
                                                                                 b.plane_bytes, b.row_off, p.body_cap,
                                                                                 b.body);
        body = b.body;
    }
    body_gather(body, b.total, p.body_cap, host_out, st);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
