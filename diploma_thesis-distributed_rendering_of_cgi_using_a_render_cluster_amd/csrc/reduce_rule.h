// The box mean a reduced output is made with (rr_frame_output.reduce), shared
// by the device kernel (reduce.hip k_film_reduce) and the host entry point's
// restatement (reduce_film_host): a W x H image of four float channels becomes
// one of ceil(W / K) x ceil(H / K).
//
// Output pixel (ox, oy) covers the block of input pixels x in [K ox, min(K ox +
// K, W)), y in [K oy, min(K oy + K, H)). Every channel of it is
//   s = 0; for y, then for x, both ascending: s = s + in[y][x]    (float32, round to nearest)
//   out = s / (float)count                                        (float32, round to nearest)
// where count is the number of pixels in the block: K K inside the image, fewer
// in the partial blocks of the right and bottom edges. No operation is fused
// and the order is fixed, so host and device agree bit for bit. The film holds
// sums over samples and so does its reduction: inv_spp applies afterwards.
//
// Host code includes this without any HIP header.
#pragma once

#include <stddef.h>

#if defined(__HIP__)
#define RR_REDUCE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_REDUCE_HD inline
#endif

namespace rr {

constexpr bool reduce_factor_valid(int k) { return k == 1 || k == 2 || k == 4 || k == 8; }
// The size of the reduced image along an axis of n pixels.
constexpr int reduced_size(int n, int k) { return (n + k - 1) / k; }

RR_REDUCE_HD float reduce_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

RR_REDUCE_HD float reduce_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// Output pixel (ox, oy) of the W x H image `in` at factor K. Px: four floats x, y, z, w.
template <class Px>
RR_REDUCE_HD Px reduce_block(const Px* in, int W, int H, int K, int ox, int oy) {
    const int x0 = ox * K, y0 = oy * K;
    const int x1 = x0 + K < W ? x0 + K : W, y1 = y0 + K < H ? y0 + K : H;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int y = y0; y < y1; ++y) {
        const Px* row = in + (size_t)y * (size_t)W;
        for (int x = x0; x < x1; ++x) {
            const Px p = row[x];
            s0 = reduce_add(s0, p.x);
            s1 = reduce_add(s1, p.y);
            s2 = reduce_add(s2, p.z);
            s3 = reduce_add(s3, p.w);
        }
    }
    const float n = (float)((x1 - x0) * (y1 - y0));
    Px o;
    o.x = reduce_div(s0, n);
    o.y = reduce_div(s1, n);
    o.z = reduce_div(s2, n);
    o.w = reduce_div(s3, n);
    return o;
}

}  // namespace rr
