// The device deflate coder (deflate.hip) and the seam its front ends plug into.
//
// An image is cut into bands of kDeflateBandRows rows of `stride` bytes. A
// front end (png.hip, png16.hip, exr.hip) is a byte function: k_deflate_front
// calls it for every position of every band and keeps the Adler sums; the
// stages of deflate.hip (match, parse, codes, emit) turn each band into a
// deflate piece, and scan + gather write the pieces to pinned host memory as
// [uint64 length][8 B pad][bytes] plus a table per band for the host's file
// wrapper (image_io png_wrap_stream / exr_wrap_stream). The band height is
// fixed, so a file's bytes depend on the image alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rr {

constexpr int kDeflateBandRows = 16;
constexpr uint32_t kDeflateSub = 4096;  // positions per Adler chunk / histogram / emit wave

struct DeflatePlan {
    int W, H, nbands;
    uint32_t stride;     // front-end bytes per row (PNG: filtered, 4W + 1 or 8W + 1; EXR: 8W)
    uint32_t band_full;  // front-end bytes of a full band
    uint32_t band_pos;   // positions reserved per band (whole parse tiles)
    uint32_t nsub, nseg; // per band: kDeflateSub-position chunks, 512-position parse segments
    uint32_t band_cap;   // bytes reserved per band's deflate piece (>= its stored form)
    // the three match distances tried at every position, 0 = none (beyond the 32 KB window)
    uint32_t dist[3];
    // 0: the bands are the pieces of one zlib stream (78 01 in front, a stored
    // band where the dynamic block would be longer); the host table holds
    // {Adler-32, front-end bytes} per band, 2 words.
    // 1: every band is a deflate stream of its own (EXR chunks): its dynamic
    // block is final and ends the piece; the alternative is not the stored form
    // but the band's raw bytes, written by the front end's owner, and the host
    // table holds {mode (0 dynamic, 1 raw), bytes, Adler-32, front-end bytes}
    // per band, 4 words.
    int own_stream;
    // own streams: the bytes of a row in a raw band, which the codes stage
    // compares a band's stream with. The front end's own (stride) but for PXR24
    // FLOAT chunks, which code 3 bytes of a sample's 4. band_cap holds either.
    uint32_t raw_stride;
};

struct DeflateBufs {
    uint8_t *filt, *out;  // filt: band b's front-end bytes at b * band_pos; out: its piece at b * band_cap
    uint16_t *cand, *exits, *entry;
    // adler_part: per kDeflateSub-byte chunk of m bytes {sum of bytes, sum of
    // (m - k) * byte k} at 2 * (b * nsub + chunk): k_deflate_front writes it,
    // the codes stage folds the chunks into the band's Adler-32.
    uint32_t* adler_part;
    uint32_t *subhist, *codes, *sub_off, *rec, *prefix;  // rec: 4 words per band (k_deflate_codes)
    size_t words;
};

// No distance of the plan twice: a repeated one becomes 0 (none). The plans of
// the four-channel files keep their lists as they were.
inline void deflate_distinct(DeflatePlan& p) {
    for (int a = 1; a < 3; ++a)
        for (int b = 0; b < a; ++b)
            if (p.dist[a] == p.dist[b]) p.dist[a] = 0u;
}

// Everything of the plan but dist and own_stream; false: a stream of 2 GB and
// more. raw_stride 0: the stride.
bool deflate_plan(int W, int H, uint32_t stride, DeflatePlan& p, uint32_t raw_stride = 0);
DeflateBufs deflate_carve(const DeflatePlan& p, uint32_t* base);  // base nullptr: only `words`
size_t deflate_scratch_words(const DeflatePlan& p);
size_t deflate_stream_max_bytes(const DeflatePlan& p);  // one zlib stream with every band stored
void deflate_bands_device(const DeflatePlan& p, const DeflateBufs& c, hipStream_t st);  // match ... emit
void deflate_gather_device(const DeflatePlan& p, const DeflateBufs& c, uint8_t* host_out, uint32_t* host_tab,
                           hipStream_t st);

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// The front end of every format: f(p, row0, n, j) is byte j of the band of n
// bytes that starts at image row row0, a pure function of the frame (no lane
// waits for another). Workgroup (chunk, band) stores its chunk's bytes and
// their Adler partial sums (DeflateBufs::adler_part).
template <class Front>
__global__ __launch_bounds__(256) void k_deflate_front(Front f, DeflatePlan p, uint8_t* __restrict__ filt,
                                                       uint32_t* __restrict__ adler_part) {
    constexpr int kThreads = 256;
    __shared__ uint32_t red[2][kThreads / 64];
    const int b = blockIdx.y;
    const int row0 = b * kDeflateBandRows;
    const uint32_t n = p.stride * (uint32_t)min(kDeflateBandRows, p.H - row0);
    const uint32_t c0 = blockIdx.x * kDeflateSub;
    if (c0 >= n) return;
    const uint32_t m = min(kDeflateSub, n - c0);
    uint8_t* out = filt + (size_t)b * p.band_pos;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t k = threadIdx.x; k < m; k += kThreads) {
        const uint32_t j = c0 + k;
        const uint32_t v = f(p, row0, n, j);
        out[j] = (uint8_t)v;
        s1 += v;
        s2 += (m - k) * v;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s1;
        red[1][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, c = 0;
        for (int w = 0; w < kThreads / 64; ++w) a += red[0][w], c += red[1][w];
        uint32_t* o = adler_part + 2 * ((size_t)b * p.nsub + blockIdx.x);
        o[0] = a;  // < 2^32: <= 4096 * 255
        o[1] = c;  // < 2^32: <= 255 * 4096 * 4097 / 2
    }
}
#endif

}  // namespace rr
