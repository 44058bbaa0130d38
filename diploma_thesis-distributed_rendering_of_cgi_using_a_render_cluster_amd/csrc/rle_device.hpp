// What the device body coders share. tga.hip, hdr.hip and iris.hip: the packer
// of one row by the packet rule of rle_rule.h and the records it leaves for the
// emit kernels. Those three and webp.hip: the step, top_bit, the carve helper of
// the slot scratch and the gather of the dense body into pinned host memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rle_rule.h"

namespace rr {

namespace {

// Elements a workgroup takes of its row per step, one a lane (k*Chunk of the
// coders' headers), and its waves.
constexpr int kBodyChunk = 256;
constexpr int kBodyWaves = kBodyChunk / 64;

// An element's record: its byte offset in its coded row | writes its bytes
// << 30 | first of its packet << 31.
constexpr uint32_t kRecWrites = 1u << 30, kRecFirst = 1u << 31, kRecOffset = kRecWrites - 1u;

__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }

// Codes one row (a TARGA row, an HDR plane, an IRIS row-plane) of W elements by
// the rule of rle_rule.h with T's numbers: leaves every element's record in
// rec[at0 + i] and, at a packet's first element, the packet's header byte in
// hdr[at0 + i]; returns the coded row's bytes. eq(j): "element j equals element
// j - 1", false for j <= 0 and j >= W. Every thread of a workgroup of
// kBodyChunk threads calls it, once (it holds barriers and ballots).
//
// kBodyChunk elements a step, one a lane. Per step: the eq bits as one ballot
// word a wave, with three bits of the step before and four of the step after
// (ew); from a lane's eight bits eq(i - 3 .. i + 4) its kind, whether a stretch
// starts at i and at i + 1; the stretch starts as ballot words (sw), whose
// highest set bit at or below a lane is its stretch's first element, found
// across the step's words and else carried from the steps before (`carry`), so
// a stretch that straddles a wave or a step is cut where the rule cuts it; the
// position in the stretch modulo the packet cap says "first of its packet";
// ballots of "first" and "writes its bytes" (fw, pw) give the byte offset by
// population counts, with the bytes of the steps before carried in `base`. A
// packet's last element knows its count and stores the header byte at the
// packet's first element.
template <class T, class Eq>
__device__ __forceinline__ uint32_t rle_pack_row(const Eq eq, int W, uint32_t* __restrict__ rec,
                                                 uint8_t* __restrict__ hdr, size_t at0) {
    constexpr int kWaves = kBodyWaves;
    __shared__ uint64_t ew[kWaves + 2], sw[kWaves], fw[kWaves], pw[kWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;      // first element of the stretch open at the step's start
    uint32_t base = 0;  // bytes of the coded row before the step
    for (int c0 = 0; c0 < W; c0 += kBodyChunk) {
        const int i = c0 + t;
        const bool valid = i < W;
        const uint64_t e = __ballot(eq(i));
        if (lane == 0) ew[1 + w] = e;
        if (w == 0) {  // eq(c0 - 3 .. c0 - 1)
            const uint64_t b = __ballot(lane >= 64 - kRleWinBack && eq(c0 - 64 + lane));
            if (lane == 0) ew[0] = b;
        }
        if (w == kWaves - 1) {  // eq(c0 + 256 .. c0 + 259)
            const uint64_t b = __ballot(lane < kRleWinFwd && eq(c0 + kBodyChunk + lane));
            if (lane == 0) ew[kWaves + 1] = b;
        }
        __syncthreads();
        // bit k of win: eq(i - 3 + k)
        const int pos = 64 - kRleWinBack + t, word = pos >> 6, sh = pos & 63;
        const uint32_t win = (uint32_t)((ew[word] >> sh) | (sh ? ew[word + 1] << (64 - sh) : 0ull)) & kRleWinMask;
        const bool run = rle_in_run<T>(win >> 1);
        const bool start = i == 0 || rle_stretch_start<T>(win);
        const bool next_starts = i + 1 >= W || rle_stretch_start<T>(win >> 1);
        const uint64_t s = __ballot(valid && start);
        if (lane == 0) sw[w] = s;
        __syncthreads();
        int first_el = carry;
        {
            const uint64_t m = sw[w] & (~0ull >> (63 - lane));
            if (m) {
                first_el = c0 + 64 * w + top_bit(m);
            } else {
                for (int k = w - 1; k >= 0; --k)
                    if (sw[k]) {
                        first_el = c0 + 64 * k + top_bit(sw[k]);
                        break;
                    }
            }
        }
        for (int k = kWaves - 1; k >= 0; --k)  // the same for every lane
            if (sw[k]) {
                carry = c0 + 64 * k + top_bit(sw[k]);
                break;
            }
        const uint32_t cap = rle_packet_cap<T>(run);
        const uint32_t q = (uint32_t)(i - first_el) % cap;
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
            const uint32_t n = T::kElemBytes * (uint32_t)__popcll(pw[k]) + (uint32_t)__popcll(fw[k]);
            if (k < w) off += n;
            base += n;
        }
        const uint64_t below = (1ull << lane) - 1ull;
        off += T::kElemBytes * (uint32_t)__popcll(pw[w] & below) + (uint32_t)__popcll(fw[w] & below);
        if (valid) {
            rec[at0 + (size_t)i] = off | (writes ? kRecWrites : 0u) | (first ? kRecFirst : 0u);
            if (q == cap - 1u || next_starts) hdr[at0 + (size_t)(i - (int)q)] = (uint8_t)T::header(run, q + 1u);
        }
    }
    return base;
}

inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }

// Carves the slot scratch, one allocation of 32-bit words, into parts that each
// start 16-byte aligned. base nullptr: only counts the words.
struct Carver {
    uint32_t* base;
    size_t words = 0;
    uint32_t* take(size_t bytes) {
        uint32_t* r = base ? base + words : nullptr;
        words += up16(bytes) / 4;
        return r;
    }
};

// The dense body to pinned host memory: [uint64 length][8 B pad][bytes], 16
// bytes a thread (the body's buffer and the stream are whole 16-byte units).
// A length above cap (never, by the formats' bounds) is reported as it is and
// the copy stops at cap: the host refuses it.
__global__ __launch_bounds__(kBodyChunk) void k_body_gather(const uint8_t* __restrict__ body,
                                                            const uint32_t* __restrict__ total, uint32_t cap,
                                                            uint8_t* __restrict__ host) {
    const uint32_t len = total[0];
    const uint64_t o = 16ull * ((uint64_t)blockIdx.x * kBodyChunk + threadIdx.x);
    if (o == 0) *reinterpret_cast<uint4*>(host) = make_uint4(len, 0u, 0u, 0u);
    if (o >= (uint64_t)min(len, cap)) return;
    *reinterpret_cast<uint4*>(host + 16 + o) = *reinterpret_cast<const uint4*>(body + o);
}

inline void body_gather(const void* body, const uint32_t* total, uint32_t cap, uint8_t* host, hipStream_t st) {
    const size_t units = up16(cap) / 16;
    k_body_gather<<<dim3((unsigned)((units + kBodyChunk - 1) / kBodyChunk)), kBodyChunk, 0, st>>>(
        static_cast<const uint8_t*>(body), total, cap, host);
}

}  // namespace

}  // namespace rr
