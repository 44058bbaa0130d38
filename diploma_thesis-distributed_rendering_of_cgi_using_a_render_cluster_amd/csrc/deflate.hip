// Deflate on the device: LZ77 over three fixed distances and one dynamic-Huffman
// block per band of rows, behind the front end of a format (deflate.hpp
// k_deflate_front; png.hip, png16.hip, exr.hip), so only the compressed bytes
// cross PCIe and the host writes the file around them.
//
// A plan (DeflatePlan: bytes per row, three candidate distances, own_stream)
// describes the bands, not a format's geometry. One-stream plans (PNG) follow
// the container scheme of the host encoder (image_io.cpp encode_png): bands of
// kDeflateBandRows whole rows, each an independent raw deflate piece that ends
// byte-aligned (an empty stored block after a dynamic block; stored pieces are
// aligned by themselves), the last one with the final block; concatenated
// behind 78 01; the bands' Adler-32s are combined on the host. With own_stream
// (EXR chunks) every band is a final stream of its own, and a band that would
// not shrink is left to the front end's owner to write raw.
//
// Per band of n = stride * rows front-end bytes, one launch per stage on the
// frame's stream (no workgroup ever waits for another):
//  - k_deflate_match: match length at every position for the plan's three
//    distances (PNG-8: 1 for zero runs, 4 the pixel period, 4W + 1 the filtered
//    row above): ballots of b[i] == b[i-d] per 64 positions, the run from a
//    position = its trailing ones across the next words, capped at 258. The
//    longest (>= 3) wins.
//  - greedy parse (take the candidate at i, go on at i + len) without a serial
//    walk over the band: k_deflate_exits computes, per 512-position segment,
//    where a parse entering at each of its first 258 positions leaves it (a
//    backward sweep in LDS, one lane per segment); k_deflate_entries chains the
//    segments' exit tables (one lane per band, tables staged in LDS);
//    k_deflate_mark walks every segment from its entry, flags the chosen
//    positions and counts the literal/length and distance symbols per 4096
//    positions.
//  - k_deflate_codes (workgroup per band): length-limited canonical Huffman
//    codes (15 / 15 / 7 bits) from the summed histograms, the exact size of the
//    dynamic block against the stored form (the smaller is taken), the block
//    header, end-of-block and trailer bits, bit offsets per 4096 positions,
//    the band's Adler-32 from the front end's partial sums.
//  - k_deflate_emit: every token ORs its bits (LSB first, codes bit-reversed)
//    at its scanned offset into zeroed words; stored bands are copied.
//  - k_deflate_scan + k_deflate_gather: bands to the prefix of their lengths in
//    pinned host memory, 16-byte stores; total length; per-band table.
// Same bytes in -> same bytes out: integer counts and ORs only, nothing depends
// on the order of arrival.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "deflate.hpp"
#include "device.hpp"
#include "prefix_code.hpp"

namespace rr {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kCodeThreads, "build_lengths strides by the workgroup");
constexpr uint32_t kTile = 16384;               // positions per parse tile (4 subs)
constexpr uint32_t kSeg = 512;                  // positions per parse segment (>= 258)
constexpr uint32_t kSegPerTile = kTile / kSeg;  // 32: one lane each
constexpr uint32_t kEntries = 258;              // a parse enters a segment at one of its first 258 positions
constexpr uint32_t kSegPad = kSeg + 2;          // LDS stride of a segment (uint16): odd in dwords, no bank conflicts
constexpr int kSyms = 320;                      // 0..285 literal/length, 288..317 distance
constexpr int kDistBase = 288;
constexpr uint32_t kChosen = 0x8000u;           // candidate word: len | dsel << 9 | kChosen
constexpr uint32_t kAdlerMod = 65521u;

struct Band {
    uint32_t n;     // filtered bytes
    int row0, rows;
    bool last;
};

__device__ __forceinline__ Band band_of(const DeflatePlan& p, int b) {
    Band r;
    r.row0 = b * kDeflateBandRows;
    r.rows = min(kDeflateBandRows, p.H - r.row0);
    r.n = p.stride * (uint32_t)r.rows;
    r.last = p.own_stream || b + 1 == p.nbands;
    return r;
}

// Exclusive scan of one value per thread over the workgroup; returns the total.
__device__ uint32_t wg_scan(uint32_t& v, uint32_t* lds_waves) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) lds_waves[w] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (int k = 0; k < kThreads / 64; ++k) {
        if (k < w) base += lds_waves[k];
        total += lds_waves[k];
    }
    v = base + inc - v;
    __syncthreads();
    return total;
}

// Deflate length / distance symbols (RFC 1951 §3.2.5).
__device__ __forceinline__ void len_sym(int len, int& sym, int& nb, uint32_t& ext) {
    const int l = len - 3;
    if (len == 258) {
        sym = 285, nb = 0, ext = 0;
    } else if (l < 8) {
        sym = 257 + l, nb = 0, ext = 0;
    } else {
        nb = 29 - __clz(l);
        sym = 257 + 4 * (nb + 1) + ((l >> nb) & 3);
        ext = (uint32_t)l & ((1u << nb) - 1u);
    }
}
__device__ __forceinline__ void dist_sym(uint32_t d, int& sym, int& nb, uint32_t& ext) {
    const uint32_t dd = d - 1;
    if (dd < 4) {
        sym = (int)dd, nb = 0, ext = 0;
    } else {
        nb = 30 - __clz((int)dd);
        sym = 2 * nb + 2 + (int)((dd >> nb) & 1u);
        ext = dd & ((1u << nb) - 1u);
    }
}
__device__ __forceinline__ int extra_bits(int s) {  // of symbol s in the kSyms numbering
    if (s >= kDistBase) return s - kDistBase >= 4 ? ((s - kDistBase) >> 1) - 1 : 0;
    return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0;
}
__device__ __forceinline__ uint32_t dist_of(const DeflatePlan& p, uint32_t dsel) {
    return dsel == 0 ? p.dist[0] : dsel == 1 ? p.dist[1] : p.dist[2];
}

// ------------------------------------------------------------- match ------
constexpr int kMaskWords = kDeflateSub / 64 + 6;  // a run from the tile's last position looks 258 positions ahead

__device__ __forceinline__ int run_from(const uint64_t* m, int g, int l) {
    const uint64_t w = ~(m[g] >> l);
    int r = w ? __builtin_ctzll(w) : 64;
    if (r < 64 - l) return r;
    r = 64 - l;
    for (int k = 1; k <= 5; ++k) {
        const uint64_t x = ~m[g + k];
        const int c = x ? __builtin_ctzll(x) : 64;
        r += c;
        if (c < 64 || r >= 258) break;
    }
    return min(r, 258);
}

__global__ __launch_bounds__(kThreads) void k_deflate_match(const uint8_t* __restrict__ filt, DeflatePlan p,
                                                        uint16_t* __restrict__ cand) {
    __shared__ uint64_t mask[3][kMaskWords];
    const int b = blockIdx.y;
    const Band bd = band_of(p, b);
    const uint32_t c0 = blockIdx.x * kDeflateSub;
    if (c0 >= bd.n) return;
    const uint8_t* f = filt + (size_t)b * p.band_pos;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t d0 = p.dist[0], d1 = p.dist[1], rd = p.dist[2];  // 0: not a candidate (beyond the window)
    for (int g = wv; g < kMaskWords; g += kThreads / 64) {
        const uint32_t j = c0 + (uint32_t)g * 64u + (uint32_t)lane;
        const bool in = j < bd.n;  // a match never runs past the band's end
        const uint32_t v = in ? f[j] : 0u;
        const bool e1 = in && d0 && j >= d0 && f[j - d0] == v;  // ... nor starts before the band
        const bool e4 = in && d1 && j >= d1 && f[j - d1] == v;
        const bool er = in && rd && j >= rd && f[j - rd] == v;
        const uint64_t m1 = __ballot(e1), m4 = __ballot(e4), mr = __ballot(er);
        if (lane == 0) {
            mask[0][g] = m1;
            mask[1][g] = m4;
            mask[2][g] = mr;
        }
    }
    __syncthreads();
    uint16_t* c = cand + (size_t)b * p.band_pos;
    // a 3-byte match further than 4096 costs more than its literals (zlib TOO_FAR)
    const int min0 = d0 > 4096 ? 4 : 3, min1 = d1 > 4096 ? 4 : 3, far_min = rd > 4096 ? 4 : 3;
    for (uint32_t k = threadIdx.x; k < kDeflateSub; k += kThreads) {
        const uint32_t j = c0 + k;
        if (j >= bd.n) break;
        const int g = (int)(k >> 6), l = (int)(k & 63);
        const int l1 = run_from(mask[0], g, l), l4 = run_from(mask[1], g, l), lr = run_from(mask[2], g, l);
        int best = 0, sel = 0;
        if (l1 >= min0) best = l1;
        if (l4 >= min1 && l4 > best) best = l4, sel = 1;
        if (lr >= far_min && lr > best) best = lr, sel = 2;
        c[j] = (uint16_t)(best | (sel << 9));
    }
}

// ------------------------------------------------------------- parse ------
__device__ __forceinline__ uint32_t seg_idx(uint32_t i) { return i + 2u * (i / kSeg); }

// Tile of candidate words into LDS (0 beyond the band's end: literals that no parse reaches).
__device__ __forceinline__ void load_tile(const uint16_t* __restrict__ c, uint32_t t0, uint32_t n, uint16_t* lds) {
    for (uint32_t i = threadIdx.x; i < kTile; i += kThreads) {
        const uint32_t j = t0 + i;
        lds[seg_idx(i)] = j < n ? (uint16_t)(c[j] & 0x7FFu) : (uint16_t)0;
    }
}

// exits[seg][e]: the position, relative to the next segment, at which the parse
// that enters segment seg at position e < 258 leaves it.
__global__ __launch_bounds__(kThreads) void k_deflate_exits(const uint16_t* __restrict__ cand, DeflatePlan p,
                                                        uint16_t* __restrict__ exits) {
    __shared__ uint16_t c[kSegPerTile * kSegPad];
    const int b = blockIdx.y;
    const Band bd = band_of(p, b);
    const uint32_t t0 = blockIdx.x * kTile;
    if (t0 >= bd.n) return;
    load_tile(cand + (size_t)b * p.band_pos, t0, bd.n, c);
    __syncthreads();
    if (threadIdx.x < kSegPerTile) {
        uint16_t* s = c + threadIdx.x * kSegPad;
        for (int i = (int)kSeg - 1; i >= 0; --i) {  // s[i]: candidate word before, exit after
            const int len = s[i] & 0x1FF;
            const int nx = i + (len ? len : 1);
            s[i] = nx >= (int)kSeg ? (uint16_t)(nx - (int)kSeg) : s[nx];
        }
    }
    __syncthreads();
    uint16_t* o = exits + ((size_t)b * p.nseg + (size_t)blockIdx.x * kSegPerTile) * kEntries;
    for (uint32_t i = threadIdx.x; i < kSegPerTile * kEntries; i += kThreads)
        o[i] = c[(i / kEntries) * kSegPad + i % kEntries];
}

// entry[seg]: where the band's parse (from its first byte) enters each segment.
constexpr uint32_t kStage = 64;  // exit tables staged per step
__global__ __launch_bounds__(64) void k_deflate_entries(const uint16_t* __restrict__ exits, DeflatePlan p,
                                                    uint16_t* __restrict__ entry) {
    __shared__ uint32_t ex[kStage * kEntries / 2];
    const int b = blockIdx.x;
    const Band bd = band_of(p, b);
    const uint32_t used = (bd.n + kSeg - 1) / kSeg;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(exits + (size_t)b * p.nseg * kEntries);
    uint16_t* out = entry + (size_t)b * p.nseg;
    uint32_t e = 0;
    for (uint32_t s0 = 0; s0 < used; s0 += kStage) {
        const uint32_t rows = min(kStage, used - s0);
        for (uint32_t i = threadIdx.x; i < rows * (kEntries / 2); i += 64) ex[i] = src[(size_t)s0 * (kEntries / 2) + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint16_t* t = reinterpret_cast<const uint16_t*>(ex);
            for (uint32_t s = 0; s < rows; ++s) {
                out[s0 + s] = (uint16_t)e;
                e = t[s * kEntries + e];
            }
        }
        __syncthreads();
    }
}

// Flags the parse's positions and counts its symbols per kDeflateSub positions.
__global__ __launch_bounds__(kThreads) void k_deflate_mark(const uint8_t* __restrict__ filt, DeflatePlan p,
                                                       uint16_t* __restrict__ cand,
                                                       const uint16_t* __restrict__ entry,
                                                       uint32_t* __restrict__ subhist) {
    __shared__ uint16_t c[kSegPerTile * kSegPad];
    __shared__ uint32_t hist[kTile / kDeflateSub][kSyms];
    const int b = blockIdx.y;
    const Band bd = band_of(p, b);
    const uint32_t t0 = blockIdx.x * kTile;
    if (t0 >= bd.n) return;
    uint16_t* cg = cand + (size_t)b * p.band_pos;
    load_tile(cg, t0, bd.n, c);
    for (uint32_t i = threadIdx.x; i < (kTile / kDeflateSub) * kSyms; i += kThreads) (&hist[0][0])[i] = 0u;
    __syncthreads();
    if (threadIdx.x < kSegPerTile && t0 + threadIdx.x * kSeg < bd.n) {
        uint16_t* s = c + threadIdx.x * kSegPad;
        uint32_t i = entry[(size_t)b * p.nseg + (size_t)blockIdx.x * kSegPerTile + threadIdx.x];
        while (i < kSeg) {
            const uint32_t v = s[i];
            s[i] = (uint16_t)(v | kChosen);
            const uint32_t len = v & 0x1FFu;
            i += len ? len : 1u;
        }
    }
    __syncthreads();
    const uint8_t* f = filt + (size_t)b * p.band_pos;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* h = hist[wv];
    for (uint32_t k = lane; k < kDeflateSub; k += 64) {
        const uint32_t i = wv * kDeflateSub + k, j = t0 + i;
        if (j >= bd.n) break;
        const uint32_t v = c[seg_idx(i)];
        if (!(v & kChosen)) continue;
        cg[j] = (uint16_t)v;
        const int len = (int)(v & 0x1FFu);
        if (len == 0) {
            atomicAdd(&h[f[j]], 1u);
        } else {
            int sym, nb;
            uint32_t ext;
            len_sym(len, sym, nb, ext);
            atomicAdd(&h[sym], 1u);
            dist_sym(dist_of(p, (v >> 9) & 3u), sym, nb, ext);
            atomicAdd(&h[kDistBase + sym], 1u);
        }
    }
    __syncthreads();
    const uint32_t sub0 = blockIdx.x * (kTile / kDeflateSub);
    for (uint32_t i = threadIdx.x; i < (kTile / kDeflateSub) * kSyms; i += kThreads) {
        const uint32_t sub = sub0 + i / kSyms;
        if (sub * kDeflateSub < bd.n) subhist[((size_t)b * p.nsub + sub) * kSyms + i % kSyms] = (&hist[0][0])[i];
    }
}

// ------------------------------------------------------------- codes ------
// (build_lengths, assign_codes, put_bits: prefix_code.hpp)

__device__ __forceinline__ uint32_t stored_bytes(uint32_t n) { return n + 5u * ((n + 65534u) / 65535u); }

__constant__ uint8_t c_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// rec[band]: {mode (0 dynamic, 1 stored), compressed bytes, Adler-32, raw bytes}.
__global__ __launch_bounds__(kThreads) void k_deflate_codes(DeflatePlan p, const uint32_t* __restrict__ subhist,
                                                        const uint32_t* __restrict__ adler_part,
                                                        uint32_t* __restrict__ codes_out,
                                                        uint32_t* __restrict__ sub_off, uint32_t* __restrict__ rec,
                                                        uint32_t* __restrict__ out_words) {
    __shared__ uint32_t freq[kSyms];
    __shared__ uint8_t lens[kSyms];
    __shared__ uint32_t codes[kSyms];
    __shared__ uint8_t cost[kSyms];  // code length + extra bits
    __shared__ TreeLds T;
    __shared__ uint32_t clfreq[19];
    __shared__ uint8_t cllen[19];
    __shared__ uint32_t clcode[19];
    __shared__ uint8_t tok_sym[kSyms], tok_ext[kSyms];
    __shared__ uint32_t s_ntok;
    const int b = blockIdx.x;
    const Band bd = band_of(p, b);
    const uint32_t nsub = (bd.n + kDeflateSub - 1) / kDeflateSub;
    const uint32_t* sh = subhist + (size_t)b * p.nsub * kSyms;
    for (int s = threadIdx.x; s < kSyms; s += kThreads) {
        uint32_t a = 0;
        for (uint32_t q = 0; q < nsub; ++q) a += sh[(size_t)q * kSyms + s];
        freq[s] = a;
        lens[s] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        freq[256] = 1;  // end of block
        // at least two codes per alphabet, so that each is a complete prefix code (zlib does the same)
        int used = 0;
        for (int s = 0; s < 286; ++s) used += freq[s] != 0;
        if (used < 2) freq[freq[0] ? 1 : 0] = 1;
        used = 0;
        for (int s = 0; s < 30; ++s) used += freq[kDistBase + s] != 0;
        for (int s = 0; used < 2; ++s)
            if (!freq[kDistBase + s]) freq[kDistBase + s] = 1, ++used;
    }
    __syncthreads();
    build_lengths(freq, 286, 15, lens, T);
    build_lengths(freq + kDistBase, 30, 15, lens + kDistBase, T);
    if (threadIdx.x == 0) {
        // the 286 + 30 code lengths as one run-length coded sequence (symbols 16 / 17 / 18)
        for (int i = 0; i < 19; ++i) clfreq[i] = 0;
        int nt = 0;
        auto seq = [&](int i) { return (int)lens[i < 286 ? i : kDistBase + i - 286]; };
        auto tok = [&](int sym, int ext) {
            tok_sym[nt] = (uint8_t)sym;
            tok_ext[nt] = (uint8_t)ext;
            ++nt;
            clfreq[sym] += 1;
        };
        for (int i = 0; i < 316;) {
            const int v = seq(i);
            int run = 1;
            while (i + run < 316 && seq(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 3) {
                    const int r = min(run, 138);
                    if (r <= 10) tok(17, r - 3);
                    else tok(18, r - 11);
                    run -= r;
                }
            } else {
                tok(v, 0);
                --run;
                while (run >= 3) {
                    const int r = min(run, 6);
                    tok(16, r - 3);
                    run -= r;
                }
            }
            for (; run > 0; --run) tok(v, 0);
        }
        s_ntok = (uint32_t)nt;
        int used = 0;
        for (int i = 0; i < 19; ++i) used += clfreq[i] != 0;
        for (int i = 0; used < 2; ++i)
            if (!clfreq[i]) clfreq[i] = 1, ++used;
    }
    __syncthreads();
    build_lengths(clfreq, 19, 7, cllen, T);
    if (threadIdx.x == 0) {
        assign_codes(lens, 286, codes);
        assign_codes(lens + kDistBase, 30, codes + kDistBase);
        assign_codes(cllen, 19, clcode);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kSyms; s += kThreads) {
        const bool real = s < 286 || (s >= kDistBase && s < kDistBase + 30);
        cost[s] = real ? (uint8_t)(lens[s] + extra_bits(s)) : (uint8_t)0;
        codes_out[(size_t)b * kSyms + s] = real ? codes[s] : 0u;
    }
    __syncthreads();
    // token bits per kDeflateSub positions (the end-of-block symbol is in no histogram)
    uint32_t* so = sub_off + (size_t)b * p.nsub;
    for (uint32_t q = threadIdx.x >> 6; q < nsub; q += kThreads / 64) {
        uint32_t a = 0;
        for (int s = threadIdx.x & 63; s < kSyms; s += 64) a += sh[(size_t)q * kSyms + s] * cost[s];
        a = wave_sum(a);
        if ((threadIdx.x & 63) == 0) so[q] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nt = s_ntok;
        uint32_t hdr = 3 + 5 + 5 + 4 + 19 * 3;
        for (uint32_t i = 0; i < nt; ++i) {
            const int s = tok_sym[i];
            hdr += cllen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
        uint32_t pos = hdr;
        for (uint32_t q = 0; q < nsub; ++q) {  // exclusive scan in place
            const uint32_t v = so[q];
            so[q] = pos;
            pos += v;
        }
        const uint32_t eob = pos;
        const uint32_t total = eob + lens[256];
        const uint32_t dyn = bd.last ? (total + 7) / 8 : (total + 3 + 7) / 8 + 4;
        // own streams: against the band's raw bytes, less the 6 bytes of zlib framing the host adds
        const uint32_t raw_n = p.raw_stride * (uint32_t)bd.rows;  // bd.n but for PXR24 FLOAT chunks
        const uint32_t sto = p.own_stream ? (raw_n > 6u ? raw_n - 6u : 0u) : stored_bytes(bd.n);
        const uint32_t mode = dyn < sto ? 0u : 1u;
        uint32_t s1 = 1, s2 = 0;  // Adler-32 of the band from the chunk sums
        for (uint32_t q = 0; q < nsub; ++q) {
            const uint32_t m = min(kDeflateSub, bd.n - q * kDeflateSub);
            const uint32_t* a = adler_part + 2 * ((size_t)b * p.nsub + q);
            s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)m * s1 + a[1]) % kAdlerMod);
            s1 = (uint32_t)(((uint64_t)s1 + a[0]) % kAdlerMod);
        }
        uint32_t* r = rec + 4 * (size_t)b;
        r[0] = mode;
        r[1] = mode ? (p.own_stream ? raw_n : sto) : dyn;
        r[2] = (s2 << 16) | s1;
        r[3] = bd.n;
        if (mode == 0) {  // block header, end of block and trailer; the tokens come from k_deflate_emit
            uint32_t* w = out_words + (size_t)b * (p.band_cap / 4);
            uint32_t at = 0;
            auto put = [&](uint32_t v, int nb) {
                put_bits(w, at, v, nb);
                at += (uint32_t)nb;
            };
            put((bd.last ? 1u : 0u) | (2u << 1), 3);  // BFINAL, BTYPE = 10
            put(286 - 257, 5);
            put(30 - 1, 5);
            put(19 - 4, 4);
            for (int i = 0; i < 19; ++i) put(cllen[c_clorder[i]], 3);
            for (uint32_t i = 0; i < nt; ++i) {
                const int s = tok_sym[i];
                put(clcode[s] & 0xFFFFu, (int)(clcode[s] >> 16));
                put(tok_ext[i], s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
            }
            at = eob;
            put(codes[256] & 0xFFFFu, (int)(codes[256] >> 16));
            if (!bd.last) {  // empty stored block: 000, pad to a byte, 00 00 FF FF
                at = (at + 3 + 7) / 8 * 8 + 16;
                put(0xFFFFu, 16);
            }
        }
    }
}

// -------------------------------------------------------------- emit ------
constexpr int kEmitWords = 64 * 48 / 32 + 4;  // 64 tokens of at most 48 bits + alignment

__global__ __launch_bounds__(kThreads) void k_deflate_emit(const uint8_t* __restrict__ filt, DeflatePlan p,
                                                       const uint16_t* __restrict__ cand,
                                                       const uint32_t* __restrict__ codes_in,
                                                       const uint32_t* __restrict__ sub_off,
                                                       const uint32_t* __restrict__ rec, uint8_t* __restrict__ out) {
    __shared__ uint32_t codes[kSyms];
    __shared__ uint32_t words[kThreads / 64][kEmitWords];
    const int b = blockIdx.y;
    const Band bd = band_of(p, b);
    const uint32_t t0 = blockIdx.x * kTile;
    if (t0 >= bd.n) return;
    const uint8_t* f = filt + (size_t)b * p.band_pos;
    uint8_t* ob = out + (size_t)b * p.band_cap;
    if (rec[4 * (size_t)b] != 0u) {  // stored: pieces of at most 65,535 bytes behind 5-byte headers
        if (p.own_stream) return;  // raw band: the front end's owner writes the unprocessed bytes (exr.hip)
        const uint32_t end = min(bd.n, t0 + kTile);
        for (uint32_t j = t0 + threadIdx.x; j < end; j += kThreads) {
            const uint32_t piece = j / 65535u;
            ob[j + 5u * (piece + 1u)] = f[j];
            if (j - piece * 65535u == 0u) {
                const uint32_t len = min(65535u, bd.n - j);
                uint8_t* h = ob + j + 5u * piece;
                h[0] = (bd.last && j + len == bd.n) ? 1 : 0;  // BFINAL, BTYPE = 00
                h[1] = (uint8_t)len;
                h[2] = (uint8_t)(len >> 8);
                h[3] = (uint8_t)~len;
                h[4] = (uint8_t)(~len >> 8);
            }
        }
        return;
    }
    for (int s = threadIdx.x; s < kSyms; s += kThreads) codes[s] = codes_in[(size_t)b * kSyms + s];
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t sub = blockIdx.x * (kTile / kDeflateSub) + wv;
    const uint32_t j0 = sub * kDeflateSub;
    if (j0 >= bd.n) return;
    const uint16_t* c = cand + (size_t)b * p.band_pos;
    uint32_t* lw = words[wv];
    uint32_t* ow = reinterpret_cast<uint32_t*>(ob);
    uint32_t pos = sub_off[(size_t)b * p.nsub + sub];
    for (uint32_t k = 0; k < kDeflateSub && j0 + k < bd.n; k += 64) {
        const uint32_t j = j0 + k + lane;
        const uint32_t v = j < bd.n ? c[j] : 0u;
        uint64_t str = 0;
        int nb = 0;
        if (v & kChosen) {
            const int len = (int)(v & 0x1FFu);
            if (len == 0) {
                const uint32_t e = codes[f[j]];
                str = e & 0xFFFFu;
                nb = (int)(e >> 16);
            } else {
                int sym, xb;
                uint32_t ext;
                len_sym(len, sym, xb, ext);
                uint32_t e = codes[sym];
                str = e & 0xFFFFu;
                nb = (int)(e >> 16);
                str |= (uint64_t)ext << nb;
                nb += xb;
                dist_sym(dist_of(p, (v >> 9) & 3u), sym, xb, ext);
                e = codes[kDistBase + sym];
                str |= (uint64_t)(e & 0xFFFFu) << nb;
                nb += (int)(e >> 16);
                str |= (uint64_t)ext << nb;
                nb += xb;
            }
        }
        uint32_t inc = (uint32_t)nb;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off);
            if ((int)lane >= off) inc += o;
        }
        const uint32_t total = __shfl(inc, 63);
        if (total == 0) continue;
        const uint32_t w0 = pos >> 5;
        const uint32_t nw = ((pos & 31u) + total + 31u) >> 5;
        for (uint32_t i = lane; i < nw; i += 64) lw[i] = 0u;
        __builtin_amdgcn_wave_barrier();
        if (nb > 0) {
            const uint32_t at = (pos & 31u) + inc - (uint32_t)nb;
            const uint32_t w = at >> 5, sh = at & 31u;
            atomicOr(&lw[w], (uint32_t)(str << sh));
            if (sh + (uint32_t)nb > 32u) atomicOr(&lw[w + 1], (uint32_t)((str << sh) >> 32));
            if (sh + (uint32_t)nb > 64u) atomicOr(&lw[w + 2], (uint32_t)(str >> (64u - sh)));
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < nw; i += 64) {  // edge words are shared with the neighbours
            const uint32_t x = lw[i];
            if (i == 0 || i + 1 == nw) atomicOr(&ow[w0 + i], x);
            else ow[w0 + i] = x;
        }
        __builtin_amdgcn_wave_barrier();
        pos += total;
    }
}

// ------------------------------------------------------------ gather ------
// host: [uint64 length][8 B pad][78 01][deflate data]; tab: {Adler-32, raw bytes} per band.
// Own streams: [uint64 length][8 B pad][the bands' pieces]; tab: rec (4 words) per band.
__global__ __launch_bounds__(kThreads) void k_deflate_scan(DeflatePlan p, const uint32_t* __restrict__ rec,
                                                       uint32_t* __restrict__ prefix, uint8_t* __restrict__ host,
                                                       uint32_t* __restrict__ tab) {
    __shared__ uint32_t ws[kThreads / 64];
    uint32_t base = 0;
    for (int b0 = 0; b0 < p.nbands; b0 += kThreads) {
        const int b = b0 + (int)threadIdx.x;
        uint32_t v = b < p.nbands ? rec[4 * (size_t)b + 1] : 0u;
        const uint32_t total = wg_scan(v, ws);
        if (b < p.nbands) {
            prefix[b] = base + v;
            if (p.own_stream) {
                for (int k = 0; k < 4; ++k) tab[4 * (size_t)b + k] = rec[4 * (size_t)b + k];
            } else {
                tab[2 * (size_t)b] = rec[4 * (size_t)b + 2];
                tab[2 * (size_t)b + 1] = rec[4 * (size_t)b + 3];
            }
        }
        base += total;
    }
    if (threadIdx.x == 0) {
        if (p.own_stream) {
            *reinterpret_cast<uint64_t*>(host) = (uint64_t)base;
            return;
        }
        *reinterpret_cast<uint64_t*>(host) = (uint64_t)base + 2u;
        host[16] = 0x78;
        host[17] = 0x01;  // deflate, 32 KB window, no dictionary (as the host encoder)
    }
}

__global__ __launch_bounds__(kThreads) void k_deflate_gather(DeflatePlan p, const uint32_t* __restrict__ rec,
                                                         const uint32_t* __restrict__ prefix,
                                                         const uint8_t* __restrict__ out, uint8_t* __restrict__ host) {
    const int b = blockIdx.y;
    const uint32_t len = rec[4 * (size_t)b + 1];
    const uint8_t* src = out + (size_t)b * p.band_cap;  // 16-byte aligned
    const size_t dst0 = (p.own_stream ? 16 : 18) + (size_t)prefix[b];
    const uint32_t head = min(len, (uint32_t)((16u - (dst0 & 15u)) & 15u));  // bytes before the first aligned chunk
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q == 0)
        for (uint32_t i = 0; i < head; ++i) host[dst0 + i] = src[i];
    const uint64_t o = (uint64_t)head + 16ull * q;  // this thread's chunk, as an offset into the band
    if (o >= len) return;
    if (o + 16 <= len) {
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(src + (o & ~3ull));
        const uint32_t sh = 8u * (uint32_t)(o & 3ull);
        uint32_t w[5];
        for (int i = 0; i < 5; ++i) w[i] = sw[i];  // w[4]: within the band's slack
        uint4 v;
        v.x = sh ? (w[0] >> sh) | (w[1] << (32u - sh)) : w[0];
        v.y = sh ? (w[1] >> sh) | (w[2] << (32u - sh)) : w[1];
        v.z = sh ? (w[2] >> sh) | (w[3] << (32u - sh)) : w[2];
        v.w = sh ? (w[3] >> sh) | (w[4] << (32u - sh)) : w[3];
        *reinterpret_cast<uint4*>(host + dst0 + o) = v;
    } else {
        for (uint64_t i = o; i < len; ++i) host[dst0 + i] = src[i];
    }
}

inline uint32_t host_stored_bytes(uint32_t n) { return n + 5u * ((n + 65534u) / 65535u); }

}  // namespace

bool deflate_plan(int W, int H, uint32_t stride, DeflatePlan& p, uint32_t raw_stride) {
    p = DeflatePlan{};
    p.W = W;
    p.H = H;
    p.stride = stride;
    p.raw_stride = raw_stride ? raw_stride : stride;
    p.nbands = (H + kDeflateBandRows - 1) / kDeflateBandRows;
    p.band_full = p.stride * (uint32_t)std::min(H, kDeflateBandRows);
    p.band_pos = (p.band_full + kTile - 1) / kTile * kTile;
    p.nsub = p.band_pos / kDeflateSub;
    p.nseg = p.band_pos / kSeg;
    const uint32_t raw_full = p.raw_stride * (uint32_t)std::min(H, kDeflateBandRows);
    p.band_cap = (std::max(host_stored_bytes(p.band_full), raw_full) + 15u) / 16u * 16u + 32u;
    return (uint64_t)p.nbands * p.band_cap < (1ull << 31);  // band offsets in the stream are 32-bit
}

size_t deflate_stream_max_bytes(const DeflatePlan& p) {
    const uint32_t last = p.stride * (uint32_t)(p.H - (p.nbands - 1) * kDeflateBandRows);
    return 2 + (size_t)(p.nbands - 1) * host_stored_bytes(p.band_full) + host_stored_bytes(last) + 4;
}

DeflateBufs deflate_carve(const DeflatePlan& p, uint32_t* base) {
    DeflateBufs c{};
    size_t at = 0;  // in 32-bit words; every part starts 16-byte aligned
    auto take = [&](size_t bytes) {
        uint32_t* r = base ? base + at : nullptr;
        at += (bytes + 15) / 16 * 4;
        return r;
    };
    const size_t nb = (size_t)p.nbands;
    c.out = reinterpret_cast<uint8_t*>(take(nb * p.band_cap));
    c.filt = reinterpret_cast<uint8_t*>(take(nb * p.band_pos));
    c.cand = reinterpret_cast<uint16_t*>(take(nb * p.band_pos * 2));
    c.exits = reinterpret_cast<uint16_t*>(take(nb * p.nseg * kEntries * 2));
    c.entry = reinterpret_cast<uint16_t*>(take(nb * p.nseg * 2));
    c.adler_part = take(nb * p.nsub * 8);
    c.subhist = take(nb * p.nsub * kSyms * 4);
    c.codes = take(nb * kSyms * 4);
    c.sub_off = take(nb * p.nsub * 4);
    c.rec = take(nb * 16);
    c.prefix = take(nb * 4);
    c.words = at;
    return c;
}

size_t deflate_scratch_words(const DeflatePlan& p) { return deflate_carve(p, nullptr).words; }

void deflate_bands_device(const DeflatePlan& p, const DeflateBufs& c, hipStream_t st) {
    const dim3 subs(p.nsub, p.nbands), tiles(p.band_pos / kTile, p.nbands);
    RR_HIP(hipMemsetAsync(c.out, 0, (size_t)p.nbands * p.band_cap, st));
    k_deflate_match<<<subs, kThreads, 0, st>>>(c.filt, p, c.cand);
    k_deflate_exits<<<tiles, kThreads, 0, st>>>(c.cand, p, c.exits);
    k_deflate_entries<<<p.nbands, 64, 0, st>>>(c.exits, p, c.entry);
    k_deflate_mark<<<tiles, kThreads, 0, st>>>(c.filt, p, c.cand, c.entry, c.subhist);
    k_deflate_codes<<<p.nbands, kThreads, 0, st>>>(p, c.subhist, c.adler_part, c.codes, c.sub_off, c.rec,
                                               reinterpret_cast<uint32_t*>(c.out));
    k_deflate_emit<<<tiles, kThreads, 0, st>>>(c.filt, p, c.cand, c.codes, c.sub_off, c.rec, c.out);
    RR_HIP(hipGetLastError());
}

void deflate_gather_device(const DeflatePlan& p, const DeflateBufs& c, uint8_t* host_out, uint32_t* host_tab,
                           hipStream_t st) {
    k_deflate_scan<<<1, kThreads, 0, st>>>(p, c.rec, c.prefix, host_out, host_tab);
    k_deflate_gather<<<dim3((p.band_cap / 16 + 1 + kThreads - 1) / kThreads, p.nbands), kThreads, 0, st>>>(
        p, c.rec, c.prefix, c.out, host_out);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
