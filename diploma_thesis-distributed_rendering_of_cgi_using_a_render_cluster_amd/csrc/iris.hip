// IRIS encode on the device: the body of a Silicon Graphics image file ("IRIS",
// .rgb) from the RGBA8 frame, so only the file's bytes cross PCIe and the host
// writes the 512-byte header (image_io iris_header_bytes). See iris.hpp, and
// iris_rule.h for the file and the packet rule, which the host encoder
// (image_io encode_iris) states as a walk over the runs and the kernels below
// as bit operations on ballots.
//
// k_iris_size (a workgroup per file row and channel: every byte's offset in its
// coded row-plane and its packet's header byte, the row-plane's length) ->
// k_iris_scan (the row-planes' offsets in the order they are stored, the body's
// length, and both tables, big-endian) -> k_iris_emit (a thread per byte stores
// its packet's header, its byte, the terminator) -> k_iris_gather (the dense
// body to pinned host memory, 16 bytes a thread). Integers only, no atomics, no
// workgroup waits for another; order comes from the launches. Same image ->
// same bytes.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "grey.h"
#include "iris.hpp"
#include "iris_rule.h"
#include "wg_scan.hpp"

namespace rr {

namespace {

constexpr int kThreads = kIrisChunk;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kRecWrites = 1u << 30, kRecFirst = 1u << 31, kRecOffset = kRecWrites - 1u;
static_assert(iris_plane_max_bytes(kIrisMaxSide) <= kRecOffset, "a row-plane offset fits the record");

// Byte j of a row-plane: the channel at bit sh8 of the interleaved RGBA8 pixel
// (R in the low byte), or the pixel's grey code.
template <bool GREY>
__device__ __forceinline__ uint32_t iris_byte(const uint32_t* __restrict__ row, int sh8, int j) {
    const uint32_t v = row[j];
    if constexpr (GREY) return grey8(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u);
    else return (v >> sh8) & 255u;
}

// eq(j) of iris_rule.h in a row-plane of W bytes.
template <bool GREY>
__device__ __forceinline__ bool iris_eq(const uint32_t* __restrict__ row, int sh8, int j, int W) {
    if (j <= 0 || j >= W) return false;
    if constexpr (GREY) return iris_byte<true>(row, sh8, j) == iris_byte<true>(row, sh8, j - 1);
    else return (((row[j] ^ row[j - 1]) >> sh8) & 255u) == 0u;
}

__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }

// One workgroup per file row f (image row H - 1 - f) and channel z, kIrisChunk
// bytes a step, one a lane. Per step: the eq bits as one ballot word a wave,
// with three bits of the neighbouring steps on either side (ew); from a lane's
// seven bits eq(i - 3 .. i + 3) its kind, whether a stretch starts at i and at
// i + 1; the stretch starts as ballot words (sw), whose highest set bit at or
// below a lane is its stretch's first byte, found across the step's words and
// else carried from the steps before (`carry`), so a stretch that straddles a
// wave or a step is cut where the rule cuts it; the position in the stretch
// modulo 127 says "first of its packet"; ballots of "first" and "writes its
// byte" (fw, pw) give the byte offset by population counts, with the bytes of
// the steps before carried in `base`. A packet's last byte knows its count and
// stores the header byte at the packet's first byte. The row-plane's length
// counts its terminator.
template <bool GREY>
__global__ __launch_bounds__(kThreads) void k_iris_size(const uint8_t* __restrict__ rgba, int W, int H, int C,
                                                        uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                        uint32_t* __restrict__ plane_bytes) {
    __shared__ uint64_t ew[kWaves + 2], sw[kWaves], fw[kWaves], pw[kWaves];
    const int f = blockIdx.x, z = blockIdx.y;
    if (f >= H || z >= C) return;
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(rgba) + (size_t)(H - 1 - f) * (size_t)W;
    const int sh8 = 8 * z;
    const size_t plane = (size_t)f * (size_t)C + (size_t)z;
    const size_t at0 = plane * (size_t)W;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;      // first byte of the stretch open at the step's start
    uint32_t base = 0;  // bytes of the coded row-plane before the step
    for (int c0 = 0; c0 < W; c0 += kThreads) {
        const int i = c0 + t;
        const bool valid = i < W;
        const uint64_t e = __ballot(iris_eq<GREY>(row, sh8, i, W));
        if (lane == 0) ew[1 + w] = e;
        if (w == 0) {  // eq(c0 - 3 .. c0 - 1)
            const uint64_t b = __ballot(lane >= 61 && iris_eq<GREY>(row, sh8, c0 - 64 + lane, W));
            if (lane == 0) ew[0] = b;
        }
        if (w == kWaves - 1) {  // eq(c0 + 256 .. c0 + 258)
            const uint64_t b = __ballot(lane < 3 && iris_eq<GREY>(row, sh8, c0 + kThreads + lane, W));
            if (lane == 0) ew[kWaves + 1] = b;
        }
        __syncthreads();
        // bit k of win: eq(i - 3 + k)
        const int pos = 61 + t, word = pos >> 6, sh = pos & 63;
        const uint32_t win = (uint32_t)((ew[word] >> sh) | (sh ? ew[word + 1] << (64 - sh) : 0ull)) & 0x7Fu;
        const bool run = iris_in_run(win >> 1);
        const bool start = i == 0 || iris_stretch_start(win & 0x3Fu);
        const bool next_starts = i + 1 >= W || iris_stretch_start(win >> 1);
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
        const uint32_t q = (uint32_t)(i - first_px) % kIrisPacket;
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
            if (q == kIrisPacket - 1u || next_starts)
                hdr[at0 + (size_t)(i - (int)q)] = (uint8_t)iris_packet_header(run, q + 1u);
        }
    }
    if (t == 0) plane_bytes[plane] = base + 1u;
}

__device__ __forceinline__ uint32_t big_endian(uint32_t v) { return __builtin_bswap32(v); }

// The row-planes' lengths, in the order the coded row-planes are stored (file
// row f, then channel z: index f C + z), into their offsets in the body and the
// body's length; the body starts with the two tables of n = H C entries. The
// same pass stores both tables: entry f + z H, big-endian, the row-plane's
// offset from the start of the file and its length. One workgroup; a body
// stays below 2^31 bytes (iris_plan).
__global__ __launch_bounds__(kThreads) void k_iris_scan(int H, int C, const uint32_t* __restrict__ plane_bytes,
                                                        uint32_t* __restrict__ plane_off,
                                                        uint32_t* __restrict__ tables, uint32_t* __restrict__ total) {
    __shared__ uint32_t ws[kWaves];
    const int n = H * C;
    uint32_t base = 8u * (uint32_t)n;
    for (int r0 = 0; r0 < n; r0 += kThreads) {
        const int r = r0 + (int)threadIdx.x;
        const uint32_t len = r < n ? plane_bytes[r] : 0u;
        uint32_t v = len;
        const uint32_t sum = wg_exclusive_scan<kWaves>(v, ws);
        if (r < n) {
            const int f = r / C, z = r - f * C;
            const int e = f + z * H;
            plane_off[r] = base + v;
            tables[e] = big_endian(kIrisHeaderBytes + base + v);
            tables[n + e] = big_endian(len);
        }
        base += sum;
    }
    if (threadIdx.x == 0) total[0] = base;
}

// A thread per byte of a row-plane (blockIdx.x: the file row; blockIdx.y:
// channel and step): a packet's first byte stores the header byte, and every
// literal byte and every run packet's first byte its value, at the row-plane's
// offset + the byte's offset in it; the row-plane's last byte also stores the
// terminator. cap: the body's bound, which the rule keeps (a store beyond it
// is dropped, and the host refuses the length).
template <bool GREY>
__global__ __launch_bounds__(kThreads) void k_iris_emit(const uint8_t* __restrict__ rgba, int W, int H, int C,
                                                        int steps, const uint32_t* __restrict__ rec,
                                                        const uint8_t* __restrict__ hdr,
                                                        const uint32_t* __restrict__ plane_bytes,
                                                        const uint32_t* __restrict__ plane_off, uint32_t cap,
                                                        uint8_t* __restrict__ body) {
    const int f = blockIdx.x, z = (int)blockIdx.y / steps;
    const int x = ((int)blockIdx.y - z * steps) * kThreads + (int)threadIdx.x;
    if (x >= W || f >= H || z >= C) return;
    const size_t plane = (size_t)f * (size_t)C + (size_t)z;
    const uint64_t plane_at = plane_off[plane];
    if (x == W - 1) {
        const uint64_t end = plane_at + plane_bytes[plane];
        if (end <= (uint64_t)cap) body[end - 1u] = 0;
    }
    const uint32_t r = rec[plane * (size_t)W + (size_t)x];
    if (!(r & kRecWrites)) return;
    const bool first = (r & kRecFirst) != 0u;
    uint64_t pos = plane_at + (r & kRecOffset);
    if (pos + (first ? 2u : 1u) > (uint64_t)cap) return;
    if (first) body[pos++] = hdr[plane * (size_t)W + (size_t)x];
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(rgba) + (size_t)(H - 1 - f) * (size_t)W;
    body[pos] = (uint8_t)iris_byte<GREY>(row, 8 * z, x);
}

// The dense body to pinned host memory: [uint64 length][8 B pad][bytes], 16
// bytes a thread (the body's buffer and the stream are whole 16-byte units).
// A length above cap (never, by the rule) is reported as it is and the copy
// stops at cap: the host refuses it.
__global__ __launch_bounds__(kThreads) void k_iris_gather(const uint8_t* __restrict__ body,
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

bool iris_plan(int W, int H, int C, IrisPlan& p) {
    const uint64_t cap = iris_body_max_bytes(W, H, C);
    p = IrisPlan{W, H, C, (uint32_t)cap};
    return cap != 0;
}

IrisBufs iris_carve(const IrisPlan& p, uint32_t* base) {
    IrisBufs b{};
    size_t at = 0;  // in 32-bit words; every part starts 16-byte aligned
    auto take = [&](size_t bytes) {
        uint32_t* r = base ? base + at : nullptr;
        at += up16(bytes) / 4;
        return r;
    };
    const size_t planes = (size_t)p.H * (size_t)p.C, nbytes = planes * (size_t)p.W;
    b.body = reinterpret_cast<uint8_t*>(take(up16(p.body_cap) + 16));
    b.total = take(16);
    b.rec = take(nbytes * 4);
    b.plane_bytes = take(planes * 4);
    b.plane_off = take(planes * 4);
    b.hdr = reinterpret_cast<uint8_t*>(take(nbytes));
    b.words = at;
    return b;
}

size_t iris_scratch_words(const IrisPlan& p) { return iris_carve(p, nullptr).words; }

size_t iris_stream_bytes(const IrisPlan& p) { return 16 + up16(p.body_cap); }

void iris_encode_device(const uint8_t* d_rgba, const IrisPlan& p, uint32_t* scratch, uint8_t* host_out,
                        hipStream_t st) {
    const IrisBufs b = iris_carve(p, scratch);
    const int W = p.W, H = p.H, C = p.C;
    const int steps = (W + kThreads - 1) / kThreads;  // at most 256: W <= 65535
    const dim3 planes((unsigned)H, (unsigned)C), bytes((unsigned)H, (unsigned)(C * steps));
    uint32_t* tables = reinterpret_cast<uint32_t*>(b.body);
    if (C == 1) k_iris_size<true><<<planes, kThreads, 0, st>>>(d_rgba, W, H, C, b.rec, b.hdr, b.plane_bytes);
    else k_iris_size<false><<<planes, kThreads, 0, st>>>(d_rgba, W, H, C, b.rec, b.hdr, b.plane_bytes);
    k_iris_scan<<<1, kThreads, 0, st>>>(H, C, b.plane_bytes, b.plane_off, tables, b.total);
    if (C == 1)
        k_iris_emit<true><<<bytes, kThreads, 0, st>>>(d_rgba, W, H, C, steps, b.rec, b.hdr, b.plane_bytes, b.plane_off,
                                                      p.body_cap, b.body);
    else
        k_iris_emit<false><<<bytes, kThreads, 0, st>>>(d_rgba, W, H, C, steps, b.rec, b.hdr, b.plane_bytes, b.plane_off,
                                                       p.body_cap, b.body);
    const size_t units = up16(p.body_cap) / 16;
    k_iris_gather<<<dim3((unsigned)((units + kThreads - 1) / kThreads)), kThreads, 0, st>>>(b.body, b.total, p.body_cap,
                                                                                            host_out);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
