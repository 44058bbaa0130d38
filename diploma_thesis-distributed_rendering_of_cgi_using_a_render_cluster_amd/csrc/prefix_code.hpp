// The prefix-code pieces the device coders share (deflate.hip, webp.hip):
// length-limited Huffman code lengths, canonical codes bit-reversed for an
// LSB-first stream, and the bit store into zeroed words.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rr {

// Threads of a workgroup that calls build_lengths.
constexpr int kCodeThreads = 256;

namespace {  // each including file has its own copies, as device code has

// Code lengths (<= maxbits) of an alphabet of n <= 286 symbols with at least two
// nonzero counts: symbols ranked by (count, index), Huffman tree by the
// two-queue merge, depths capped and the Kraft sum repaired by moving leaves
// down (the scheme of miniz' tdefl_huffman_enforce_max_code_size), lengths
// handed out by rank. The whole workgroup calls it; lane 0 runs the tree.
struct TreeLds {
    uint16_t order[286];   // used symbols, ascending count
    uint32_t iw[286];      // internal node weights, in creation order
    uint16_t lpar[286];    // leaf -> internal node
    uint16_t ipar[286];    // internal -> internal node
    uint16_t idepth[286];
    uint32_t nused;
};

__device__ void build_lengths(const uint32_t* freq, int n, int maxbits, uint8_t* lens, TreeLds& T) {
    if (threadIdx.x == 0) T.nused = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < n; s += kCodeThreads) {
        lens[s] = 0;
        const uint32_t fs = freq[s];
        if (!fs) continue;
        uint32_t r = 0;
        for (int o = 0; o < n; ++o) {
            const uint32_t fo = freq[o];
            r += (fo && (fo < fs || (fo == fs && o < s))) ? 1u : 0u;
        }
        T.order[r] = (uint16_t)s;
        atomicAdd(&T.nused, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nu = (int)T.nused;
        int li = 0, ii = 0, ni = 0;
        for (int k = 0; k + 1 < nu; ++k) {
            uint32_t w = 0;
            for (int pick = 0; pick < 2; ++pick) {
                if (li < nu && (ii >= ni || freq[T.order[li]] <= T.iw[ii])) {
                    w += freq[T.order[li]];
                    T.lpar[li++] = (uint16_t)ni;
                } else {
                    w += T.iw[ii];
                    T.ipar[ii++] = (uint16_t)ni;
                }
            }
            T.iw[ni++] = w;
        }
        int count[33];
        for (int i = 0; i <= 32; ++i) count[i] = 0;
        if (ni > 0) T.idepth[ni - 1] = 0;
        for (int k = ni - 2; k >= 0; --k) T.idepth[k] = (uint16_t)(T.idepth[T.ipar[k]] + 1);
        for (int i = 0; i < nu; ++i) count[min((int)T.idepth[T.lpar[i]] + 1, maxbits)] += 1;
        uint32_t total = 0;
        for (int i = maxbits; i >= 1; --i) total += (uint32_t)count[i] << (maxbits - i);
        while (total > (1u << maxbits)) {
            count[maxbits] -= 1;
            for (int i = maxbits - 1; i >= 1; --i)
                if (count[i]) {
                    count[i] -= 1;
                    count[i + 1] += 2;
                    break;
                }
            total -= 1;
        }
        int j = nu;
        for (int i = 1; i <= maxbits; ++i)
            for (int l = count[i]; l > 0; --l) lens[T.order[--j]] = (uint8_t)i;
    }
    __syncthreads();
}

// Canonical codes of lens[0..n), bit-reversed for deflate's LSB-first packing: code | len << 16.
__device__ void assign_codes(const uint8_t* lens, int n, uint32_t* codes) {
    uint32_t next[17];
    int count[17];
    for (int i = 0; i <= 16; ++i) count[i] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]] += 1;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int i = 1; i <= 16; ++i) {
        code = (code + (uint32_t)count[i - 1]) << 1;
        next[i] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        codes[s] = l ? ((__brev(next[l]++) >> (32 - l)) | ((uint32_t)l << 16)) : 0u;
    }
}

// Bits [pos, pos + nb) of a zeroed LSB-first word array = the low nb <= 32 bits of v.
__device__ __forceinline__ void put_bits(uint32_t* words, uint32_t pos, uint32_t v, int nb) {
    if (nb <= 0) return;
    const uint64_t x = (uint64_t)v << (pos & 31u);
    words[pos >> 5] |= (uint32_t)x;
    if ((pos & 31u) + (uint32_t)nb > 32u) words[(pos >> 5) + 1] |= (uint32_t)(x >> 32);
}

}  // namespace

}  // namespace rr
