// WEBP encode on the device: the VP8L payload of a lossless WebP file from the
// RGBA8 frame, so only the file's bytes cross PCIe and the host writes the 20
// RIFF bytes and the pad byte (image_io webp_wrap_stream). See webp.hpp, and
// webp_rule.h for the file, the run rule and the codes, which the host encoder
// (image_io encode_webp) states as a plain walk and the kernels below as
// ballots, counts and scans.
//
// k_webp_residual (a thread per pixel: colour mode, subtract-green, the
// prediction by one neighbour) -> k_webp_size (a workgroup per row: "equals the
// left residual", the stretches' first pixels from ballots, every pixel's kind,
// a copy's length at its first pixel, the five alphabets' counts from LDS into
// global counters) -> k_webp_codes (one workgroup: simple or normal form,
// build_lengths at 15 bits, the header's bits, the code table) -> k_webp_bits
// (a row's bits) -> k_webp_scan (the rows' offsets, the payload's length) ->
// k_webp_zero (the words the tokens go to) -> k_webp_emit (a thread per pixel
// ORs its token in at its row's offset + the scan of the tokens before it) ->
// k_body_gather (the dense payload to pinned host memory, 16 bytes a thread).
// Integer sums and ORs only, so nothing depends on the order of arrival: same
// image -> same bytes. No workgroup waits for another; order comes from the
// launches.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "prefix_code.hpp"
#include "rle_device.hpp"
#include "webp.hpp"
#include "webp_rule.h"
#include "wg_scan.hpp"

namespace rr {

namespace {

static_assert(kWebpChunk == kBodyChunk, "the shared step");
constexpr int kThreads = kBodyChunk;
constexpr int kWaves = kBodyWaves;
static_assert(kThreads == kCodeThreads, "build_lengths strides by the workgroup");
constexpr int kMaxRowGroups = 512;  // workgroups of the row kernels: each takes every kMaxRowGroups-th row
// The header's words: its longest form, rounded up to whole 16-byte units.
constexpr int kHdrWords = (int)((kWebpHeaderMaxBits + 31) / 32 + 3) / 4 * 4;
constexpr uint32_t kRecLen = (1u << 30) - 1u;
static_assert(kWebpMaxCopy <= kRecLen, "a copy's length fits the record");
static_assert((uint64_t)kWebpMaxSide * kWebpTokenMaxBits < (1ull << 24), "a step's bits fit the scan's 32-bit sums");

__global__ __launch_bounds__(kThreads) void k_webp_residual(const uint32_t* __restrict__ rgba, int W, int H, int C,
                                                            uint32_t* __restrict__ resid) {
    const size_t n = (size_t)W * (size_t)H;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % (size_t)W);
    const uint32_t pred = x > 0              ? webp_pixel(rgba[i - 1], C)
                          : i >= (size_t)W   ? webp_pixel(rgba[i - (size_t)W], C)
                                             : kWebpFirstPrediction;
    resid[i] = webp_sub(webp_pixel(rgba[i], C), pred);
}

// eq(j) of webp_rule.h in a row of W residuals.
__device__ __forceinline__ bool webp_eq(const uint32_t* __restrict__ row, int j, int W) {
    return j > 0 && j < W && row[j] == row[j - 1];
}

// A workgroup per row (every gridDim.x-th), kWebpChunk pixels a step, one a
// lane. Per step: the stretch starts (eq(i) and not eq(i - 1)) as one ballot
// word a wave, whose highest set bit at or below a lane is its stretch's first
// pixel, found across the step's words and else carried from the steps before;
// the position in the stretch and eq(i .. i + kWebpMinRun - 1) give the kind
// (webp_kind). A literal records itself and counts its four residuals; a
// chunk's last pixel knows the chunk's length and, where that makes a copy,
// records it at the chunk's first pixel and counts its two symbols; a covered
// pixel records itself. So every record is written by one thread. The counts
// are gathered in LDS and added to the global counters at the end.
__global__ __launch_bounds__(kThreads) void k_webp_size(const uint32_t* __restrict__ resid, int W, int H,
                                                        uint32_t* __restrict__ rec, uint32_t* __restrict__ hist) {
    __shared__ uint64_t sw[kWaves];
    __shared__ uint32_t h[kWebpSyms];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int s = t; s < kWebpSyms; s += kThreads) h[s] = 0u;
    __syncthreads();
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const uint32_t* __restrict__ row = resid + (size_t)y * (size_t)W;
        uint32_t* __restrict__ rrow = rec + (size_t)y * (size_t)W;
        int carry = 0;  // first pixel of the stretch open at the step's start
        for (int c0 = 0; c0 < W; c0 += kThreads) {
            const int i = c0 + t;
            const bool valid = i < W;
            uint32_t win = 0;
            for (uint32_t k = 0; k < kWebpMinRun; ++k) win |= (webp_eq(row, i + (int)k, W) ? 1u : 0u) << k;
            const bool e0 = (win & 1u) != 0u;
            const uint64_t s = __ballot(valid && e0 && !webp_eq(row, i - 1, W));
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
            __syncthreads();  // sw is free for the next step
            if (!valid) continue;
            const uint32_t q = e0 ? (uint32_t)(i - first_px) : 0u;
            const int kind = webp_kind(win, q);
            if (kind == kWebpLiteral) {
                const uint32_t v = row[i];
                rrow[i] = (uint32_t)kWebpLiteral << 30;
                atomicAdd(&h[kWebpGreen + ((v >> 8) & 255u)], 1u);
                atomicAdd(&h[kWebpRed + ((v >> 16) & 255u)], 1u);
                atomicAdd(&h[kWebpBlue + (v & 255u)], 1u);
                atomicAdd(&h[kWebpAlpha + (v >> 24)], 1u);
            } else if (kind == kWebpCovered) {
                rrow[i] = (uint32_t)kWebpCovered << 30;
            }
            if (e0) {
                const uint32_t m = q % kWebpMaxCopy;
                if ((m == kWebpMaxCopy - 1u || !(win & 2u)) && m + 1u >= kWebpMinRun) {  // a copy's last pixel
                    uint32_t sym, nb, extra;
                    webp_prefix(m + 1u, sym, nb, extra);
                    rrow[i - (int)m] = (uint32_t)kWebpCopy << 30 | (m + 1u);
                    atomicAdd(&h[kWebpGreen + 256 + sym], 1u);
                    atomicAdd(&h[kWebpDist + kWebpDistSym], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int s = t; s < kWebpSyms; s += kThreads)
        if (h[s]) atomicAdd(&hist[s], h[s]);
}

// ------------------------------------------------------------- codes ------
struct HeaderBits {
    uint32_t* words;
    uint32_t pos;
    __device__ void put(uint32_t v, int nb) {
        put_bits(words, pos, v, nb);
        pos += (uint32_t)nb;
    }
    // A simple code of n = 1 or 2 symbols, s0 < s1 < 256.
    __device__ void simple(int n, uint32_t s0, uint32_t s1) {
        put(1u, 1);
        put((uint32_t)(n - 1), 1);
        put(s0 > 1u ? 1u : 0u, 1);
        put(s0, s0 > 1u ? 8 : 1);
        if (n == 2) put(s1, 8);
    }
};

// One workgroup: the counts into the five codes and the header. Per alphabet:
// the used symbols' number, lowest and highest; a simple code where
// webp_rule.h says so, else build_lengths at 15 bits, the lengths' own counts,
// build_lengths at 7 bits for the code-length code (or length 1 for its only
// used symbol, whose uses then take no bits), canonical codes, and the header
// bits by lane 0 into LDS. The first kHdrWords words of the payload get the
// header and zeros behind it; meta[0] its bits.
__global__ __launch_bounds__(kThreads) void k_webp_codes(WebpPlan p, const uint32_t* __restrict__ hist,
                                                         uint32_t* __restrict__ codes_out,
                                                         uint32_t* __restrict__ body, uint32_t* __restrict__ meta) {
    __shared__ uint32_t freq[kWebpSyms];
    __shared__ uint8_t lens[kWebpSyms];
    __shared__ uint32_t codes[kWebpSyms];
    __shared__ TreeLds T;
    __shared__ uint32_t hw[kHdrWords];
    __shared__ uint32_t clfreq[19], clcode[19];
    __shared__ uint8_t cllen[19];
    __shared__ uint32_t used_n, used_lo, used_hi, cl_used, hdr_pos;
    const int t = threadIdx.x;
    for (int s = t; s < kWebpSyms; s += kThreads) freq[s] = hist[s], lens[s] = 0, codes[s] = 0u;
    for (int s = t; s < kHdrWords; s += kThreads) hw[s] = 0u;
    __syncthreads();
    if (t == 0) {
        HeaderBits b{hw, 0u};
        b.put(0x2Fu, 8);
        b.put((uint32_t)(p.W - 1), 14);
        b.put((uint32_t)(p.H - 1), 14);
        b.put(p.C == 4 ? 1u : 0u, 1);  // alpha_is_used
        b.put(0u, 3);                  // version
        b.put(1u, 1), b.put(2u, 2);    // a transform: subtract-green
        b.put(1u, 1), b.put(0u, 2);    // a transform: predictor
        b.put(kWebpBlockBits - 2u, 3);
        b.put(0u, 1);                  // its sub-image: no colour cache
        b.simple(1, 1u, 0u);           // green: mode 1 in every block
        for (int a = 1; a < kWebpAlphabets; ++a) b.simple(1, 0u, 0u);
        b.put(0u, 1);                  // no more transforms
        b.put(0u, 1), b.put(0u, 1);    // the image: no colour cache, no meta prefix codes
        hdr_pos = b.pos;
    }
    for (int a = 0; a < kWebpAlphabets; ++a) {
        const int base = webp_base(a), n = webp_size(a);
        if (t == 0) used_n = 0u, used_lo = 0xFFFFFFFFu, used_hi = 0u;
        __syncthreads();
        for (int s = t; s < n; s += kThreads)
            if (freq[base + s]) {
                atomicAdd(&used_n, 1u);
                atomicMin(&used_lo, (uint32_t)s);
                atomicMax(&used_hi, (uint32_t)s);
            }
        __syncthreads();
        const uint32_t nu = used_n, lo = used_lo, hi = used_hi;
        if (nu == 0u || (nu <= 2u && hi < 256u)) {  // the same in every thread
            if (t == 0) {
                HeaderBits b{hw, hdr_pos};
                b.simple(nu == 2u ? 2 : 1, nu ? lo : 0u, hi);
                if (nu == 2u) codes[base + lo] = 0u | 1u << 16, codes[base + hi] = 1u | 1u << 16;
                hdr_pos = b.pos;
            }
            __syncthreads();  // every thread has read the used_ words
            continue;
        }
        build_lengths(freq + base, n, kWebpMaxBits, lens + base, T);
        if (t == 0) {
            for (int k = 0; k < 19; ++k) clfreq[k] = 0u, cllen[k] = 0, clcode[k] = 0u;
            for (int s = 0; s < n; ++s) clfreq[lens[base + s]] += 1u;
            uint32_t cu = 0;
            for (int k = 0; k < 19; ++k)
                if (clfreq[k]) ++cu, cllen[k] = 1;  // (build_lengths writes them anew where there are two)
            cl_used = cu;
        }
        __syncthreads();
        if (cl_used >= 2u) build_lengths(clfreq, 19, kWebpClMaxBits, cllen, T);
        if (t == 0) {
            assign_codes(lens + base, n, codes + base);
            if (cl_used >= 2u) assign_codes(cllen, 19, clcode);
            HeaderBits b{hw, hdr_pos};
            b.put(0u, 1);
            b.put(19u - 4u, 4);
            for (int k = 0; k < 19; ++k) b.put(cllen[webp_cl_order(k)], 3);
            b.put(0u, 1);  // every symbol's length follows
            for (int s = 0; s < n; ++s) {
                const uint32_t c = clcode[lens[base + s]];
                b.put(c & 0xFFFFu, (int)(c >> 16));
            }
            hdr_pos = b.pos;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int s = t; s < kWebpSyms; s += kThreads) codes_out[s] = codes[s];
    for (int s = t; s < kHdrWords; s += kThreads) body[s] = hw[s];
    if (t == 0) meta[0] = hdr_pos;
}

// A pixel's token from its record and residual through the code table cd
// (code | length << 16 per symbol): the bits in v, LSB first, and their number
// (at most kWebpTokenMaxBits; 0 for a covered pixel).
__device__ __forceinline__ uint32_t webp_token(const uint32_t* cd, uint32_t rec, uint32_t res, uint64_t& v) {
    const uint32_t kind = rec >> 30;
    v = 0;
    if (kind == (uint32_t)kWebpCovered) return 0u;
    uint32_t nb = 0;
    auto add = [&](uint32_t c) {
        v |= (uint64_t)(c & 0xFFFFu) << nb;
        nb += c >> 16;
    };
    if (kind == (uint32_t)kWebpLiteral) {
        add(cd[kWebpGreen + ((res >> 8) & 255u)]);
        add(cd[kWebpRed + ((res >> 16) & 255u)]);
        add(cd[kWebpBlue + (res & 255u)]);
        add(cd[kWebpAlpha + (res >> 24)]);
    } else {
        uint32_t sym, xb, extra;
        webp_prefix(rec & kRecLen, sym, xb, extra);
        add(cd[kWebpGreen + 256 + sym]);
        add(extra | xb << 16);
        add(cd[kWebpDist + kWebpDistSym]);
    }
    return nb;
}

// A row's bits (a workgroup per row, every gridDim.x-th).
__global__ __launch_bounds__(kThreads) void k_webp_bits(const uint32_t* __restrict__ resid,
                                                        const uint32_t* __restrict__ rec,
                                                        const uint32_t* __restrict__ codes, int W, int H,
                                                        uint32_t* __restrict__ row_bits) {
    __shared__ uint32_t cd[kWebpSyms];
    __shared__ uint32_t ws[kWaves];
    const int t = threadIdx.x;
    for (int s = t; s < kWebpSyms; s += kThreads) cd[s] = codes[s];
    __syncthreads();
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const size_t at = (size_t)y * (size_t)W;
        uint32_t bits = 0;
        for (int c0 = 0; c0 < W; c0 += kThreads) {
            const int i = c0 + t;
            uint64_t v;
            uint32_t nb = i < W ? webp_token(cd, rec[at + (size_t)i], resid[at + (size_t)i], v) : 0u;
            bits += wg_exclusive_scan<kWaves>(nb, ws);
        }
        if (t == 0) row_bits[y] = bits;
    }
}

// The rows' bits into their offsets from the end of the header, and the
// payload's length in bytes: meta[1]. One workgroup; a step's sum stays below
// 2^32 (256 rows of less than 2^24 bits), the offsets are 64-bit.
__global__ __launch_bounds__(kThreads) void k_webp_scan(int H, const uint32_t* __restrict__ row_bits,
                                                        uint64_t* __restrict__ row_off, uint32_t* __restrict__ meta) {
    __shared__ uint32_t ws[kWaves];
    uint64_t base = 0;
    for (int r0 = 0; r0 < H; r0 += kThreads) {
        const int r = r0 + (int)threadIdx.x;
        uint32_t v = r < H ? row_bits[r] : 0u;
        const uint32_t sum = wg_exclusive_scan<kWaves>(v, ws);
        if (r < H) row_off[r] = base + v;
        base += sum;
    }
    if (threadIdx.x == 0) meta[1] = (uint32_t)((base + meta[0] + 7u) / 8u);
}

// Zeroes the payload's words behind the header's up to the payload's end and
// two words beyond it, 16 bytes a thread; units: the buffer's 16-byte units.
__global__ __launch_bounds__(kThreads) void k_webp_zero(uint32_t* __restrict__ body, const uint32_t* __restrict__ meta,
                                                        size_t units) {
    const size_t u = (size_t)(kHdrWords / 4) + (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= units || 16ull * u >= (uint64_t)meta[1] + 16ull) return;
    reinterpret_cast<uint4*>(body)[u] = make_uint4(0u, 0u, 0u, 0u);
}

// A workgroup per row (every gridDim.x-th), a thread per pixel: the scan of the
// tokens' bits gives each its place, and it ORs its bits into the zeroed words
// (at most 60 bits over three words). words: the buffer's words; a token that
// would pass them (never, by the bound) is dropped, and the host refuses the
// length.
__global__ __launch_bounds__(kThreads) void k_webp_emit(const uint32_t* __restrict__ resid,
                                                        const uint32_t* __restrict__ rec,
                                                        const uint32_t* __restrict__ codes, int W, int H,
                                                        const uint64_t* __restrict__ row_off,
                                                        const uint32_t* __restrict__ meta, uint32_t* __restrict__ body,
                                                        size_t words) {
    __shared__ uint32_t cd[kWebpSyms];
    __shared__ uint32_t ws[kWaves];
    const int t = threadIdx.x;
    for (int s = t; s < kWebpSyms; s += kThreads) cd[s] = codes[s];
    __syncthreads();
    const uint64_t hdr_bits = meta[0];
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const size_t at = (size_t)y * (size_t)W;
        uint64_t base = hdr_bits + row_off[y];
        for (int c0 = 0; c0 < W; c0 += kThreads) {
            const int i = c0 + t;
            uint64_t v = 0;
            const uint32_t nb = i < W ? webp_token(cd, rec[at + (size_t)i], resid[at + (size_t)i], v) : 0u;
            uint32_t off = nb;
            const uint32_t sum = wg_exclusive_scan<kWaves>(off, ws);
            if (nb) {
                const uint64_t pos = base + off;
                const size_t wd = (size_t)(pos >> 5);
                const uint32_t sh = (uint32_t)pos & 31u;
                if (wd + 2 < words) {
                    const uint64_t lo = v << sh;
                    const uint32_t hi = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
                    if ((uint32_t)lo) atomicOr(&body[wd], (uint32_t)lo);
                    if ((uint32_t)(lo >> 32)) atomicOr(&body[wd + 1], (uint32_t)(lo >> 32));
                    if (hi) atomicOr(&body[wd + 2], hi);
                }
            }
            base += sum;
        }
    }
}

// The payload buffer's bytes: the bound in whole 16-byte units and two more,
// and at least the header's words.
inline size_t body_bytes(const WebpPlan& p) {
    const size_t b = up16(p.body_cap) + 32;
    return b > (size_t)kHdrWords * 4 ? b : (size_t)kHdrWords * 4;
}

}  // namespace

bool webp_plan(int W, int H, int C, WebpPlan& p) {
    const uint64_t cap = webp_body_max_bytes(W, H, C);
    p = WebpPlan{W, H, C, (uint32_t)cap};
    return cap != 0;
}

WebpBufs webp_carve(const WebpPlan& p, uint32_t* base) {
    WebpBufs b{};
    Carver c{base};
    const size_t n = (size_t)p.W * (size_t)p.H;
    b.body = c.take(body_bytes(p));
    b.hist = c.take((size_t)kWebpSyms * 4);
    b.codes = c.take((size_t)kWebpSyms * 4);
    b.meta = c.take(16);
    b.row_off = reinterpret_cast<uint64_t*>(c.take((size_t)p.H * 8));
    b.row_bits = c.take((size_t)p.H * 4);
    b.resid = c.take(n * 4);
    b.rec = c.take(n * 4);
    b.words = c.words;
    return b;
}

size_t webp_scratch_words(const WebpPlan& p) { return webp_carve(p, nullptr).words; }

void webp_encode_device(const uint8_t* d_rgba, const WebpPlan& p, uint32_t* scratch, uint8_t* host_out,
                        hipStream_t st) {
    const WebpBufs b = webp_carve(p, scratch);
    const int W = p.W, H = p.H;
    const size_t n = (size_t)W * (size_t)H;
    const unsigned rows = (unsigned)(H < kMaxRowGroups ? H : kMaxRowGroups);
    const size_t units = body_bytes(p) / 16, words = units * 4;
    RR_HIP(hipMemsetAsync(b.hist, 0, (size_t)kWebpSyms * 4, st));
    k_webp_residual<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), kThreads, 0, st>>>(
        reinterpret_cast<const uint32_t*>(d_rgba), W, H, p.C, b.resid);
    k_webp_size<<<rows, kThreads, 0, st>>>(b.resid, W, H, b.rec, b.hist);
    k_webp_codes<<<1, kThreads, 0, st>>>(p, b.hist, b.codes, b.body, b.meta);
    k_webp_bits<<<rows, kThreads, 0, st>>>(b.resid, b.rec, b.codes, W, H, b.row_bits);
    k_webp_scan<<<1, kThreads, 0, st>>>(H, b.row_bits, b.row_off, b.meta);
    k_webp_zero<<<dim3((unsigned)((units + kThreads - 1) / kThreads)), kThreads, 0, st>>>(b.body, b.meta, units);
    k_webp_emit<<<rows, kThreads, 0, st>>>(b.resid, b.rec, b.codes, W, H, b.row_off, b.meta, b.body, words);
    body_gather(b.body, b.meta + 1, p.body_cap, host_out, st);  // meta[1]: the payload's bytes
    RR_HIP(hipGetLastError());
}

}  // namespace rr
