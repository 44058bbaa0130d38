// HDR encode on the device: the body of a Radiance RGBE file ("HDR") from the
// slot's film, so only the file's bytes cross PCIe and the host writes the text
// header (image_io hdr_header_bytes). See hdr.hpp, and hdr_rule.h for the RGBE
// rule and the scanline rule, which the host encoder (image_io encode_hdr)
// states as a walk over the runs and the kernels below as bit operations on
// ballots.
//
// Coded rows (8 <= W <= 32767): k_hdr_quad (a thread per pixel: the quad of the
// film's means, one word) -> k_hdr_size (a workgroup per row and plane: every
// byte's offset in its coded plane and its packet's header byte, the plane's
// length) -> k_hdr_scan (a row is 4 marker bytes and its four planes: the rows'
// offsets, the body's length) -> k_hdr_emit (a thread per plane byte stores its
// byte, one lane a row the marker) -> k_hdr_gather (the dense body to pinned
// host memory, 16 bytes a thread). Flat rows: k_hdr_quad -> k_hdr_gather, the
// quads are the body. Integers only after k_hdr_quad, no atomics, no workgroup
// waits for another; order comes from the launches. Same film -> same bytes.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "grey.h"
#include "hdr.hpp"
#include "hdr_rule.h"

namespace rr {

namespace {

constexpr int kThreads = kHdrChunk;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kRecWrites = 1u << 30, kRecFirst = 1u << 31, kRecOffset = kRecWrites - 1u;
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

// eq(j) of hdr_rule.h in a plane of W bytes: byte `sh8` / 8 of the row's quads.
__device__ __forceinline__ bool hdr_eq(const uint32_t* __restrict__ row, int sh8, int j, int W) {
    if (j <= 0 || j >= W) return false;
    return (((row[j] ^ row[j - 1]) >> sh8) & 255u) == 0u;
}

__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }

// One workgroup per row y and plane pl, kHdrChunk bytes a step, one a lane.
// Per step: the eq bits as one ballot word a wave, with three bits of the step
// before and four of the step after (ew); from a lane's eight bits
// eq(i - 3 .. i + 4) its kind (the four three-in-a-row windows that cover it),
// whether a stretch starts at i and at i + 1; the stretch starts as ballot
// words (sw), whose highest set bit at or below a lane is its stretch's first
// byte, found across the step's words and else carried from the steps before
// (`carry`); the position in the stretch modulo 127 (runs) or 128 (literals)
// says "first of its packet"; ballots of "first" and "writes its byte" (fw,
// pw) give the byte offset by population counts, with the bytes of the steps
// before carried in `base`. A packet's last byte knows its count and stores
// the header byte at the packet's first byte.
__global__ __launch_bounds__(kThreads) void k_hdr_size(const uint32_t* __restrict__ quad, int W, int H,
                                                       uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                       uint32_t* __restrict__ plane_bytes) {
    __shared__ uint64_t ew[kWaves + 2], sw[kWaves], fw[kWaves], pw[kWaves];
    const int y = blockIdx.x, pl = blockIdx.y;
    if (y >= H || pl >= 4) return;
    const uint32_t* __restrict__ row = quad + (size_t)y * (size_t)W;
    const int sh8 = 8 * pl;
    const size_t at0 = ((size_t)y * 4 + (size_t)pl) * (size_t)W;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;      // first byte of the stretch open at the step's start
    uint32_t base = 0;  // bytes of the coded plane before the step
    for (int c0 = 0; c0 < W; c0 += kThreads) {
        const int i = c0 + t;
        const bool valid = i < W;
        const uint64_t e = __ballot(hdr_eq(row, sh8, i, W));
        if (lane == 0) ew[1 + w] = e;
        if (w == 0) {  // eq(c0 - 3 .. c0 - 1)
            const uint64_t b = __ballot(lane >= 61 && hdr_eq(row, sh8, c0 - 64 + lane, W));
            if (lane == 0) ew[0] = b;
        }
        if (w == kWaves - 1) {  // eq(c0 + 256 .. c0 + 259)
            const uint64_t b = __ballot(lane < 4 && hdr_eq(row, sh8, c0 + kThreads + lane, W));
            if (lane == 0) ew[kWaves + 1] = b;
        }
        __syncthreads();
        // bit k of win: eq(i - 3 + k)
        const int pos = 61 + t, word = pos >> 6, sh = pos & 63;
        const uint32_t win = (uint32_t)((ew[word] >> sh) | (sh ? ew[word + 1] << (64 - sh) : 0ull)) & 0xFFu;
        const bool run = hdr_in_run(win >> 1);
        const bool start = i == 0 || hdr_stretch_start(win & 0x7Fu);
        const bool next_starts = i + 1 >= W || hdr_stretch_start(win >> 1);
        const uint64_t s = __ballot(valid && start);
        if (lane == 0) sw[w] = s;
        __syncthreads();
        int first_px = carry;
        {
            const uint64_t m = sw[w] & (~0ull >> (63 - lane));
            if (m) {
                first_px = c0 + 64 * w + top_bit(m);
            } else {
                for (int k = w - 1; k >= 0; --k)
                    if (sw[k]) {
                        first_px = c0 + 64 * k + top_bit(sw[k]);
                        break;
                    }
            }
        }
        for (int k = kWaves - 1; k >= 0; --k)  // the same for every lane
            if (sw[k]) {
                carry = c0 + 64 * k + top_bit(sw[k]);
                break;
            }
        const uint32_t q = (uint32_t)(i - first_px) % (run ? kHdrRunPacket : kHdrLitPacket);
        const bool first = valid && q == 0u;
        const bool writes = valid && (!run || q == 0u);
        const uint64_t fb = __ballot(first), pb = __ballot(writes);
        if (lane == 0) {
            fw[w] = fb;
            pw[w] = pb;
        }
        __syncthreads();
        uint32_t off = base;
        for (int k = 0; k < kWaves; ++k) {
            const uint32_t n = (uint32_t)__popcll(pw[k]) + (uint32_t)__popcll(fw[k]);
            if (k < w) off += n;
            base += n;
        }
        const uint64_t below = (1ull << lane) - 1ull;
        off += (uint32_t)__popcll(pw[w] & below) + (uint32_t)__popcll(fw[w] & below);
        if (valid) {
            rec[at0 + (size_t)i] = off | (writes ? kRecWrites : 0u) | (first ? kRecFirst : 0u);
            if (q == (run ? kHdrRunPacket : kHdrLitPacket) - 1u || next_starts)
                hdr[at0 + (size_t)(i - (int)q)] = (uint8_t)hdr_packet_header(run, q + 1u);
        }
    }
    if (t == 0) plane_bytes[4 * (size_t)y + (size_t)pl] = base;
}

// Exclusive scan of one value a thread over the workgroup; returns the total.
__device__ uint32_t hdr_wg_scan(uint32_t& v, uint32_t* lds_waves) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds_waves[w] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < kWaves; ++k) {
        if (k < w) before += lds_waves[k];
        total += lds_waves[k];
    }
    v = before + inc - v;
    __syncthreads();
    return total;
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
        const uint32_t sum = hdr_wg_scan(v, ws);
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

// The dense body to pinned host memory: [uint64 length][8 B pad][bytes], 16
// bytes a thread (the body's buffer and the stream are whole 16-byte units).
// A length above cap (never, by the rule) is reported as it is and the copy
// stops at cap: the host refuses it.
__global__ __launch_bounds__(kThreads) void k_hdr_gather(const uint8_t* __restrict__ body,
                                                         const uint32_t* __restrict__ total, uint32_t cap,
                                                         uint8_t* __restrict__ host) {
    const uint32_t len = total[0];
    const uint64_t o = 16ull * ((uint64_t)blockIdx.x * kThreads + threadIdx.x);
    if (o == 0) *reinterpret_cast<uint4*>(host) = make_uint4(len, 0u, 0u, 0u);
    if (o >= (uint64_t)min(len, cap)) return;
    *reinterpret_cast<uint4*>(host + 16 + o) = *reinterpret_cast<const uint4*>(body + o);
}

inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }

}  // namespace

bool hdr_plan(int W, int H, int C, HdrPlan& p) {
    const uint64_t cap = (C == 1 || C == 3) ? hdr_body_max_bytes(W, H) : 0;
    p = HdrPlan{W, H, C, hdr_row_flat(W), (uint32_t)cap};
    return cap != 0;
}

HdrBufs hdr_carve(const HdrPlan& p, uint32_t* base) {
    HdrBufs b{};
    size_t at = 0;  // in 32-bit words; every part starts 16-byte aligned
    auto take = [&](size_t bytes) {
        uint32_t* r = base ? base + at : nullptr;
        at += up16(bytes) / 4;
        return r;
    };
    const size_t npix = (size_t)p.W * (size_t)p.H;
    b.quad = take(up16(npix * 4) + 16);
    b.total = take(16);
    if (!p.flat) {
        b.body = reinterpret_cast<uint8_t*>(take(up16(p.body_cap) + 16));
        b.rec = take(npix * 16);
        b.plane_bytes = take((size_t)p.H * 16);
        b.row_off = take((size_t)p.H * 4);
        b.hdr = reinterpret_cast<uint8_t*>(take(npix * 4));
    }
    b.words = at;
    return b;
}

size_t hdr_scratch_words(const HdrPlan& p) { return hdr_carve(p, nullptr).words; }

size_t hdr_stream_bytes(const HdrPlan& p) { return 16 + up16(p.body_cap); }

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
    const size_t units = up16(p.body_cap) / 16;
    k_hdr_gather<<<dim3((unsigned)((units + kThreads - 1) / kThreads)), kThreads, 0, st>>>(body, b.total, p.body_cap,
                                                                                           host_out);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
