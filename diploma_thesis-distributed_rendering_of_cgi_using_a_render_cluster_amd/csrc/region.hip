// The windowed film of a region frame. See region.hpp. Pure data movement: one
// float4 (16 bytes) in and out per thread, no arithmetic on the colour sums, so
// a region's values are the full frame's own bits.
#include "region.hpp"

#include <stdexcept>

namespace rr {

namespace {

constexpr int kWindowBlock = 256;

// Thread i = output pixel i (row-major in the output image, ow pixels a row).
// kCrop: output (ox, oy) is film (x0 + ox, y0 + oy). Else the output is the
// frame: inside [x0, x1) x [y0, y1) the film's pixel, outside zeros.
template <bool kCrop>
__global__ __launch_bounds__(kWindowBlock) void k_film_window(const float4* __restrict__ film, int W, int ow,
                                                              unsigned n_out, int x0, int y0, int x1, int y1,
                                                              float alpha_sum, float4* __restrict__ out) {
    const unsigned i = blockIdx.x * (unsigned)kWindowBlock + threadIdx.x;
    if (i >= n_out) return;
    const int oy = (int)(i / (unsigned)ow), ox = (int)(i - (unsigned)oy * (unsigned)ow);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (kCrop) {
        v = film[(size_t)(y0 + oy) * (size_t)W + (size_t)(x0 + ox)];
        v.w = alpha_sum;
    } else if (ox >= x0 && ox < x1 && oy >= y0 && oy < y1) {
        v = film[i];
        v.w = alpha_sum;
    }
    out[i] = v;
}

__global__ __launch_bounds__(kWindowBlock) void k_window_mask8(uint32_t* __restrict__ rgba8, int W, unsigned npix, int x0,
                                                               int y0, int x1, int y1) {
    const unsigned i = blockIdx.x * (unsigned)kWindowBlock + threadIdx.x;
    if (i >= npix) return;
    const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
    if (!(x >= x0 && x < x1 && y >= y0 && y < y1)) rgba8[i] = 0u;
}

void check_rect(int W, int H, const RegionRect& r) {
    if (W <= 0 || H <= 0 || (long long)W * H > 0x7fffffffll || r.empty() || r.x0 < 0 || r.y0 < 0 || r.x1 > W || r.y1 > H)
        throw std::runtime_error("film window: the region must lie inside the frame");
}

}  // namespace

void film_window_device(const float4* film, int W, int H, RegionRect r, bool crop, float alpha_sum, float4* out,
                        hipStream_t st) {
    check_rect(W, H, r);
    const int ow = crop ? r.w() : W, oh = crop ? r.h() : H;
    const unsigned n = (unsigned)ow * (unsigned)oh;
    const unsigned grid = (n + kWindowBlock - 1) / kWindowBlock;
    if (crop) k_film_window<true><<<grid, kWindowBlock, 0, st>>>(film, W, ow, n, r.x0, r.y0, r.x1, r.y1, alpha_sum, out);
    else k_film_window<false><<<grid, kWindowBlock, 0, st>>>(film, W, ow, n, r.x0, r.y0, r.x1, r.y1, alpha_sum, out);
    if (hipGetLastError() != hipSuccess) throw std::runtime_error("k_film_window launch failed");
}

void window_mask8_device(uint8_t* rgba8, int W, int H, RegionRect r, hipStream_t st) {
    check_rect(W, H, r);
    const unsigned n = (unsigned)W * (unsigned)H;
    k_window_mask8<<<(n + kWindowBlock - 1) / kWindowBlock, kWindowBlock, 0, st>>>(reinterpret_cast<uint32_t*>(rgba8), W,
                                                                                   n, r.x0, r.y0, r.x1, r.y1);
    if (hipGetLastError() != hipSuccess) throw std::runtime_error("k_window_mask8 launch failed");
}

}  // namespace rr
