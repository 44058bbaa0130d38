// IRIS encode on the device: the body of a Silicon Graphics image file ("IRIS",
// .rgb) from the RGBA8 frame, so only the file's bytes cross PCIe and the host
// writes the 512-byte header (image_io iris_header_bytes). See iris.hpp, and
// iris_rule.h for the file and the packet rule, which the host encoder
// (image_io encode_iris) states as a walk over the runs and the device packer
// (rle_device.hpp) as bit operations on ballots.
//
// k_iris_size (a workgroup per file row and channel: every byte's offset in its
// coded row-plane and its packet's header byte, the row-plane's length) ->
// k_iris_scan (the row-planes' offsets in the order they are stored, the body's
// length, and both tables, big-endian) -> k_iris_emit (a thread per byte stores
// its packet's header, its byte, the terminator) -> k_body_gather (the dense
// body to pinned host memory, 16 bytes a thread). Integers only, no atomics, no
// workgroup waits for another; order comes from the launches. Same image ->
// same bytes.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "grey.h"
#include "iris.hpp"
#include "iris_rule.h"
#include "rle_device.hpp"
#include "wg_scan.hpp"

namespace rr {

namespace {

static_assert(kIrisChunk == kBodyChunk, "the packer's step");
constexpr int kThreads = kBodyChunk;
constexpr int kWaves = kBodyWaves;
static_assert(iris_plane_max_bytes(kIrisMaxSide) <= kRecOffset, "a row-plane offset fits the record");

// Byte j of a row-plane: the channel at bit sh8 of the interleaved RGBA8 pixel
// (R in the low byte), or the pixel's grey code.
template <bool GREY>
__device__ __forceinline__ uint32_t iris_byte(const uint32_t* __restrict__ row, int sh8, int j) {
    const uint32_t v = row[j];
    if constexpr (GREY) return grey8(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u);
    else return (v >> sh8) & 255u;
}

// One workgroup per file row f (image row H - 1 - f) and channel z:
// rle_pack_row over the row-plane's bytes. The row-plane's length counts its
// terminator.
template <bool GREY>
__global__ __launch_bounds__(kThreads) void k_iris_size(const uint8_t* __restrict__ rgba, int W, int H, int C,
                                                        uint32_t* __restrict__ rec, uint8_t* __restrict__ hdr,
                                                        uint32_t* __restrict__ plane_bytes) {
    const int f = blockIdx.x, z = blockIdx.y;
    if (f >= H || z >= C) return;
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(rgba) + (size_t)(H - 1 - f) * (size_t)W;
    const int sh8 = 8 * z;
    const size_t plane = (size_t)f * (size_t)C + (size_t)z;
    const auto eq = [row, sh8, W](int j) {
        if (j <= 0 || j >= W) return false;
        if constexpr (GREY) return iris_byte<true>(row, sh8, j) == iris_byte<true>(row, sh8, j - 1);
        else return (((row[j] ^ row[j - 1]) >> sh8) & 255u) == 0u;
    };
    const uint32_t bytes = rle_pack_row<IrisRle>(eq, W, rec, hdr, plane * (size_t)W);
    if (threadIdx.x == 0) plane_bytes[plane] = bytes + 1u;
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

}  // namespace

bool iris_plan(int W, int H, int C, IrisPlan& p) {
    const uint64_t cap = iris_body_max_bytes(W, H, C);
    p = IrisPlan{W, H, C, (uint32_t)cap};
    return cap != 0;
}

IrisBufs iris_carve(const IrisPlan& p, uint32_t* base) {
    IrisBufs b{};
    Carver c{base};
    const size_t planes = (size_t)p.H * (size_t)p.C, nbytes = planes * (size_t)p.W;
    b.body = reinterpret_cast<uint8_t*>(c.take(up16(p.body_cap) + 16));
    b.total = c.take(16);
    b.rec = c.take(nbytes * 4);
    b.plane_bytes = c.take(planes * 4);
    b.plane_off = c.take(planes * 4);
    b.hdr = reinterpret_cast<uint8_t*>(c.take(nbytes));
    b.words = c.words;
    return b;
}

size_t iris_scratch_words(const IrisPlan& p) { return iris_carve(p, nullptr).words; }

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
    body_gather(b.body, b.total, p.body_cap, host_out, st);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
