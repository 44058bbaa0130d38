// The film reduction kernel of reduced outputs. See reduce.hpp and reduce_rule.h.
//
// One thread per output pixel, consecutive lanes on consecutive output pixels
// of a row. A lane reads its block row by row, K float4 (16 K bytes, contiguous)
// a row. At K = 2 a wave's load instruction covers 64 x 32 B of one input row
// with half of each 32-byte piece, and the next instruction the other half; at
// K = 8 a lane owns a whole 128-byte line of the row, so one instruction touches
// 64 different lines (stride 128 B) and takes 16 bytes of each, and the lane's
// following seven loads of that row hit the lines it has just brought in. Every
// byte of the film is still fetched from memory once (33 MB at 1080p); what the
// strided shape costs is requests per byte at the L1, not traffic. The writes
// are one float4 a lane, contiguous. profiles/multi_output.md has the times.
//
// The additions of a block are a chain (reduce_rule.h fixes their order), so
// lanes cannot share a block; staging rows through LDS would change who loads,
// not who adds.
#pragma clang fp contract(off)

#include "reduce.hpp"

#include <stdexcept>

namespace rr {

namespace {

template <int K>
__global__ __launch_bounds__(256) void k_film_reduce(const float4* __restrict__ film, int W, int H, int OW, int OH,
                                                     float4* __restrict__ out) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    out[(size_t)oy * (size_t)OW + ox] = reduce_block(film, W, H, K, ox, oy);
}

template <int K>
void launch(const float4* film, int W, int H, float4* out, hipStream_t st) {
    const int OW = reduced_size(W, K), OH = reduced_size(H, K);
    const dim3 grid((unsigned)((OW + 63) / 64), (unsigned)((OH + 3) / 4));
    k_film_reduce<K><<<grid, 256, 0, st>>>(film, W, H, OW, OH, out);
}

struct HostPx {
    float x, y, z, w;
};

}  // namespace

void film_reduce_device(const float4* film, int W, int H, int K, float4* out, hipStream_t st) {
    if (!film || !out || W <= 0 || H <= 0) throw std::runtime_error("film reduction of an empty image");
    // (the grid's second dimension holds 65535 blocks of 4 rows: any height a frame can have)
    if (reduced_size(H, K < 1 ? 1 : K) > 4 * 65535) throw std::runtime_error("film reduction: image too tall");
    switch (K) {
    case 1: launch<1>(film, W, H, out, st); break;  // the rule at K = 1 (inspection only)
    case 2: launch<2>(film, W, H, out, st); break;
    case 4: launch<4>(film, W, H, out, st); break;
    case 8: launch<8>(film, W, H, out, st); break;
    default: throw std::runtime_error("film reduction factor must be 1, 2, 4 or 8");
    }
    if (hipGetLastError() != hipSuccess) throw std::runtime_error("k_film_reduce launch failed");
}

void film_reduce_host(const float* rgba, int W, int H, int K, float* out) {
    const HostPx* in = reinterpret_cast<const HostPx*>(rgba);
    HostPx* o = reinterpret_cast<HostPx*>(out);
    const int OW = reduced_size(W, K), OH = reduced_size(H, K);
    for (int oy = 0; oy < OH; ++oy)
        for (int ox = 0; ox < OW; ++ox) o[(size_t)oy * OW + ox] = reduce_block(in, W, H, K, ox, oy);
}

}  // namespace rr
