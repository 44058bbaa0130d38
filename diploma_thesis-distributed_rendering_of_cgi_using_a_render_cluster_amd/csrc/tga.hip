// TARGA encode on the device: the body of a "TARGA" / "TARGA_RAW" file from the
// RGBA8 frame, so only the file's bytes cross PCIe and the host writes the
// 18-byte header (image_io tga_header_bytes). See tga.hpp, and tga_rule.h for
// the packet rule, which the host encoder (image_io encode_tga) states as a
// walk over the runs and the kernels below as bit operations on ballots.
//
// "TARGA": k_tga_size (a workgroup per file row: every pixel's offset in its
// coded row and its packet's header byte, the row's length) -> k_tga_scan (the
// rows' offsets in file order, the body's length) -> k_tga_emit (a thread per
// pixel stores its bytes) -> k_tga_gather (the dense body to pinned host
// memory, 16 bytes a thread). "TARGA_RAW": k_tga_raw -> k_tga_gather.
// Integers only, no atomics, no workgroup waits for another; order comes from
// the launches. Same image -> same bytes.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "grey.h"
#include "tga.hpp"
#include "tga_rule.h"

namespace rr {

namespace {

constexpr int kThreads = kTgaChunk;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kRecWrites = 1u << 30, kRecFirst = 1u << 31, kRecOffset = kRecWrites - 1u;
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

// eq(j) of tga_rule.h in a row of W pixels.
template <int C>
__device__ __forceinline__ bool tga_eq(const uint32_t* __restrict__ row, int j, int W) {
    if (j <= 0 || j >= W) return false;
    return tga_key<C>(row[j]) == tga_key<C>(row[j - 1]);
}

__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }

// One workgroup per file row f (image row H - 1 - f), kTgaChunk pixels a step,
// one a lane. Per step: the eq bits as one ballot word a wave, with three bits
// of the neighbouring steps on either side (ew); from a lane's seven bits
// eq(i - 3 .. i + 3) its kind, whether a stretch starts at i and at i + 1; the
// stretch starts as ballot words (sw), whose highest set bit at or below a
// lane is its stretch's first pixel, found across the step's words and else
// carried from the steps before (`carry`); the position in the stretch modulo
// 128 says "first of its packet"; ballots of "first" and "writes its pixel"
// (fw, pw) give the byte offset by population counts, with the bytes of the
// steps before carried in `base`. A packet's last pixel knows its count and
// stores the header byte at the packet's first pixel.
template <int C>
__global__ __launch_bounds__(kThreads) void k_tga_size(const uint8_t* __restrict__ rgba, int W, int H,
                                                       uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                       uint32_t* __restrict__ row_bytes) {
    __shared__ uint64_t ew[kWaves + 2], sw[kWaves], fw[kWaves], pw[kWaves];
    const int f = blockIdx.x;
    if (f >= H) return;
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(rgba) + (size_t)(H - 1 - f) * (size_t)W;
    const size_t at0 = (size_t)f * (size_t)W;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;      // first pixel of the stretch open at the step's start
    uint32_t base = 0;  // bytes of the row before the step
    for (int c0 = 0; c0 < W; c0 += kThreads) {
        const int i = c0 + t;
        const bool valid = i < W;
        const uint64_t e = __ballot(tga_eq<C>(row, i, W));
        if (lane == 0) ew[1 + w] = e;
        if (w == 0) {  // eq(c0 - 3 .. c0 - 1)
            const uint64_t b = __ballot(lane >= 61 && tga_eq<C>(row, c0 - 64 + lane, W));
            if (lane == 0) ew[0] = b;
        }
        if (w == kWaves - 1) {  // eq(c0 + 256 .. c0 + 258)
            const uint64_t b = __ballot(lane < 3 && tga_eq<C>(row, c0 + kThreads + lane, W));
            if (lane == 0) ew[kWaves + 1] = b;
        }
        __syncthreads();
        // bit k of win: eq(i - 3 + k)
        const int pos = 61 + t, word = pos >> 6, sh = pos & 63;
        const uint32_t win = (uint32_t)((ew[word] >> sh) | (sh ? ew[word + 1] << (64 - sh) : 0ull)) & 0x7Fu;
        const bool run = tga_in_run<C>(win >> 1);
        const bool start = i == 0 || tga_stretch_start<C>(win & 0x3Fu);
        const bool next_starts = i + 1 >= W || tga_stretch_start<C>(win >> 1);
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
        const uint32_t q = (uint32_t)(i - first_px) & (kTgaPacket - 1u);
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
            const uint32_t n = (uint32_t)C * (uint32_t)__popcll(pw[k]) + (uint32_t)__popcll(fw[k]);
            if (k < w) off += n;
            base += n;
        }
        const uint64_t below = (1ull << lane) - 1ull;
        off += (uint32_t)C * (uint32_t)__popcll(pw[w] & below) + (uint32_t)__popcll(fw[w] & below);
        if (valid) {
            rec[at0 + (size_t)i] = off | (writes ? kRecWrites : 0u) | (first ? kRecFirst : 0u);
            if (q == kTgaPacket - 1u || next_starts)
                hdr[at0 + (size_t)(i - (int)q)] = (uint8_t)tga_packet_header(run, q + 1u);
        }
    }
    if (t == 0) row_bytes[f] = base;
}

// Exclusive scan of one value a thread over the workgroup; returns the total.
__device__ uint32_t tga_wg_scan(uint32_t& v, uint32_t* lds_waves) {
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

// The rows' lengths, in file order, into their offsets in the body and the
// body's length. One workgroup; a body stays below 2^31 bytes (tga_plan).
__global__ __launch_bounds__(kThreads) void k_tga_scan(int H, const uint32_t* __restrict__ row_bytes,
                                                       uint32_t* __restrict__ row_off, uint32_t* __restrict__ total) {
    __shared__ uint32_t ws[kWaves];
    uint32_t base = 0;
    for (int r0 = 0; r0 < H; r0 += kThreads) {
        const int r = r0 + (int)threadIdx.x;
        uint32_t v = r < H ? row_bytes[r] : 0u;
        const uint32_t sum = tga_wg_scan(v, ws);
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

// The dense body to pinned host memory: [uint64 length][8 B pad][bytes], 16
// bytes a thread (the body's buffer and the stream are whole 16-byte units).
// A length above cap (never, by the rule) is reported as it is and the copy
// stops at cap: the host refuses it.
__global__ __launch_bounds__(kThreads) void k_tga_gather(const uint8_t* __restrict__ body,
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

bool tga_plan(int W, int H, int C, bool rle, TgaPlan& p) {
    const uint64_t cap = tga_body_max_bytes(W, H, C, rle);
    p = TgaPlan{W, H, C, rle, (uint32_t)cap};
    return cap != 0;
}

TgaBufs tga_carve(const TgaPlan& p, uint32_t* base) {
    TgaBufs b{};
    size_t at = 0;  // in 32-bit words; every part starts 16-byte aligned
    auto take = [&](size_t bytes) {
        uint32_t* r = base ? base + at : nullptr;
        at += up16(bytes) / 4;
        return r;
    };
    const size_t npix = (size_t)p.W * (size_t)p.H;
    b.body = reinterpret_cast<uint8_t*>(take(up16(p.body_cap) + 16));
    b.total = take(16);
    if (p.rle) {
        b.rec = take(npix * 4);
        b.row_bytes = take((size_t)p.H * 4);
        b.row_off = take((size_t)p.H * 4);
        b.hdr = reinterpret_cast<uint8_t*>(take(npix));
    }
    b.words = at;
    return b;
}

size_t tga_scratch_words(const TgaPlan& p) { return tga_carve(p, nullptr).words; }

size_t tga_stream_bytes(const TgaPlan& p) { return 16 + up16(p.body_cap); }

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
    const size_t units = up16(p.body_cap) / 16;
    k_tga_gather<<<dim3((unsigned)((units + kThreads - 1) / kThreads)), kThreads, 0, st>>>(b.body, b.total, p.body_cap,
                                                                                           host_out);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
