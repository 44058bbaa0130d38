// The Filmic family's chain per pixel (device) and the display gamma (host and
// device): see view.hpp for the chain and where it comes from. Shared by
// k_view (view.hip, 8-bit) and Png16Sub (png16.hip, 16-bit): both quantise the
// float result of filmic_display / display_gamma. The float operations of the
// base chain are written in the order oracle/rr_oracle.c orc_filmic uses,
// contraction off, so the 8-bit output is bit-identical to the oracle's
// (tests/test_gpu_view.py); tests/view_settings.py restates every mode in
// numpy float32 (tests/test_gpu_view_settings.py).
#pragma once
#pragma clang fp contract(off)

#include "device.hpp"

namespace rr {

// log2 for normal positive x without libm: x = 2^e m, m in [1, 2) folded
// into [sqrt(1/2), sqrt(2)); log2 m = 2/ln 2 atanh(t), t = (m - 1)/(m + 1),
// by its odd series to t^9 (|t| < 0.172: truncation < 4e-10).
RR_HD float log2_fixed(float x) {
    const int bits = f2i(x);
    int e = ((bits >> 23) & 0xff) - 127;
    float m = i2f((bits & 0x007fffff) | 0x3f800000);
    if (m > 1.41421356f) {
        m = m * 0.5f;
        e = e + 1;
    }
    const float t = (m - 1.0f) / (m + 1.0f);
    const float t2 = t * t;
    const float p = ((((t2 * 0.111111112f + 0.142857149f) * t2 + 0.2f) * t2 + 0.333333343f) * t2 + 1.0f) * t;
    return (float)e + p * 2.88539004f;
}

// 2^x without libm, written like log2_fixed: x = n + f, n the nearest integer
// (f in [-1/2, 1/2]), 2^f = e^u with u = f ln 2 by its series to u^7
// (|u| < 0.347: truncation < 6e-9), 2^n added to the exponent field. 0 below
// 2^-125, 2^127 from there up.
RR_HD float exp2_fixed(float x) {
    if (x < -125.0f) return 0.0f;
    if (x >= 127.0f) return 1.70141183e38f;
    const float h = x + 0.5f;
    int n = (int)h;
    if ((float)n > h) n = n - 1;
    const float f = x - (float)n;
    const float u = f * 0.693147182f;
    const float p = ((((((u * 1.98412701e-4f + 1.38888892e-3f) * u + 8.33333377e-3f) * u + 4.16666679e-2f) * u +
                       0.166666672f) * u + 0.5f) * u + 1.0f) * u + 1.0f;
    return i2f(f2i(p) + n * 8388608);
}

// Display gamma g on a display-referred value d: d^(1/g), 0 for d <= 0
// (inv_g = 1.0f / g; callers skip the step for g = 1).
RR_HD float display_gamma(float d, float inv_g) {
    if (d <= 0.0f) return 0.0f;
    return exp2_fixed(log2_fixed(d) * inv_g);
}

RR_HD float sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// OCIO Lut1D, linear interpolation over the domain [lo, hi] (clamped).
RR_D float lut1d(const float* __restrict__ t, int n, int comps, int c, float lo, float hi, float x) {
    float f = (x - lo) / (hi - lo) * (float)(n - 1);
    f = fminf(fmaxf(f, 0.0f), (float)(n - 1));
    const int i = (int)f;
    if (i >= n - 1) return t[(n - 1) * comps + c];
    const float fr = f - (float)i;
    const float a = t[i * comps + c], b = t[(i + 1) * comps + c];
    return a + (b - a) * fr;
}

RR_D float3 ld3(const float4* __restrict__ cube, int i) {
    const float4 v = cube[i];
    return make_float3(v.x, v.y, v.z);
}

// OCIO Lut3D tetrahedral interpolation; input clamped to [0, 1].
RR_D float3 lut3d_tetra(const float4* __restrict__ cube, int n, float r, float g, float b) {
    const float s = (float)(n - 1);
    float fr = sat(r) * s, fg = sat(g) * s, fb = sat(b) * s;
    const int ir = min((int)fr, n - 2), ig = min((int)fg, n - 2), ib = min((int)fb, n - 2);
    fr = fr - (float)ir;
    fg = fg - (float)ig;
    fb = fb - (float)ib;
    auto at = [&](int di, int dj, int dk) { return ld3(cube, ((ir + di) * n + (ig + dj)) * n + (ib + dk)); };
    const float3 c000 = at(0, 0, 0), c111 = at(1, 1, 1);
    float3 c1, c2;
    float w0, w1, w2, w3;
    if (fr > fg) {
        if (fg > fb) {  // r > g > b
            c1 = at(1, 0, 0); c2 = at(1, 1, 0);
            w0 = 1.0f - fr; w1 = fr - fg; w2 = fg - fb; w3 = fb;
        } else if (fr > fb) {  // r > b >= g
            c1 = at(1, 0, 0); c2 = at(1, 0, 1);
            w0 = 1.0f - fr; w1 = fr - fb; w2 = fb - fg; w3 = fg;
        } else {  // b >= r > g
            c1 = at(0, 0, 1); c2 = at(1, 0, 1);
            w0 = 1.0f - fb; w1 = fb - fr; w2 = fr - fg; w3 = fg;
        }
    } else {
        if (fb > fg) {  // b > g >= r
            c1 = at(0, 0, 1); c2 = at(0, 1, 1);
            w0 = 1.0f - fb; w1 = fb - fg; w2 = fg - fr; w3 = fr;
        } else if (fb > fr) {  // g >= b > r
            c1 = at(0, 1, 0); c2 = at(0, 1, 1);
            w0 = 1.0f - fg; w1 = fg - fb; w2 = fb - fr; w3 = fr;
        } else {  // g >= r >= b
            c1 = at(0, 1, 0); c2 = at(1, 1, 0);
            w0 = 1.0f - fg; w1 = fg - fr; w2 = fr - fb; w3 = fb;
        }
    }
    return make_float3(((w0 * c000.x + w1 * c1.x) + w2 * c2.x) + w3 * c111.x,
                       ((w0 * c000.y + w1 * c1.y) + w2 * c2.y) + w3 * c111.y,
                       ((w0 * c000.z + w1 * c1.z) + w2 * c2.z) + w3 * c111.z);
}

// Scene-linear c (the film's mean times the exposure scale) -> Filmic Log: the
// cube's output over its allocation [0, 0.66].
RR_D void filmic_log(const FilmicArgs& f, const float c[3], float L[3]) {
    float a[3];
    for (int k = 0; k < 3; ++k) a[k] = (log2_fixed(fmaxf(c[k], 1.17549435e-38f)) + 12.473931188f) / 25.0f;
    const float3 b = lut3d_tetra(f.cube, f.n3, a[0], a[1], a[2]);
    L[0] = b.x / 0.66f;
    L[1] = b.y / 0.66f;
    L[2] = b.z / 0.66f;
}

// Scene-linear c -> display-referred values of a view of the Filmic family,
// before display gamma and quantisation.
//   RR_VIEW_FILMIC:      the 1D curve of f (the base curve, or the look's in
//                        its place) of Filmic Log
//   RR_VIEW_FILMIC_LOG:  Filmic Log itself
//   RR_VIEW_FALSE_COLOR: the false-colour cube at Filmic Log's luminance
RR_D void filmic_display(const FilmicArgs& f, int view, const float c[3], float d[3]) {
    float L[3];
    filmic_log(f, c, L);
    if (view == RR_VIEW_FILMIC_LOG) {
        for (int k = 0; k < 3; ++k) d[k] = L[k];
    } else if (view == RR_VIEW_FALSE_COLOR) {
        const float pr = 0.2126729f * L[0], pg = 0.7151521f * L[1], pb = 0.0721750f * L[2];
        const float s = pr + pg;
        const float y = s + pb;
        const float3 v = lut3d_tetra(f.fcube, f.nf, y, y, y);
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
    } else {
        for (int k = 0; k < 3; ++k) d[k] = lut1d(f.lut1, f.n1, f.comps, f.comps == 3 ? k : 0, f.lo1, f.hi1, L[k]);
    }
}

}  // namespace rr
