// View settings: OCIO LUT parsing (host) and the per-pixel second pass over
// the film (device). See view.hpp for the chain and where it comes from. The
// float operations of the base chain are written in the order
// oracle/rr_oracle.c orc_filmic uses, so its 8-bit output is bit-identical to
// the oracle's (tests/test_gpu_view.py).
#pragma clang fp contract(off)

#include "view.hpp"
#include "dither.h"
#include "view_filmic.h"

#include <cstring>
#include <fstream>
#include <sstream>

namespace rr {

namespace {

// 8-bit sRGB table intervals of the render kernels' tonemap (paths.hpp kSrgbN)
constexpr int kViewSrgbN = 4096;

// The view pass: VIEW, GAMMA and DITHER are compile-time, so Filmic at gamma 1
// keeps the instructions it had before there were other settings. Standard and
// Raw (here for their display gamma or the dither) repeat paths.hpp tonemap up
// to the quantiser. DITHER adds dither.h's noise of the pixel, scaled by
// f.dither, to the three display-referred values before they are quantised.
template <int VIEW, bool GAMMA, bool DITHER>
__global__ __launch_bounds__(256) void k_view(FrameConsts fc, FilmicArgs f, const float* __restrict__ srgb,
                                              const float4* __restrict__ film, uchar4* __restrict__ out) {
    float inv_w = 0.0f, inv_h = 0.0f;
    if constexpr (DITHER) {
        inv_w = 1.0f / (float)fc.W;
        inv_h = 1.0f / (float)fc.H;
    }
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < fc.npix; pix += gridDim.x * 256) {
        const float4 acc = film[pix];
        const float c[3] = {acc.x * fc.inv_spp * fc.exposure_scale, acc.y * fc.inv_spp * fc.exposure_scale,
                            acc.z * fc.inv_spp * fc.exposure_scale};
        float d[3];
        if constexpr (VIEW >= RR_VIEW_FILMIC) {
            filmic_display(f, VIEW, c, d);
        } else {
            for (int k = 0; k < 3; ++k) {
                float v = fminf(fmaxf(c[k], 0.0f), 1.0f);
                if (VIEW == RR_VIEW_STANDARD) v = srgb_oetf(v, srgb, kViewSrgbN);
                d[k] = v;
            }
        }
        if constexpr (GAMMA)
            for (int k = 0; k < 3; ++k) d[k] = display_gamma(d[k], f.inv_gamma);
        if constexpr (DITHER) {
            // rows run top to bottom here, Blender's bottom-up
            const int row = (int)fc.div_w.div((uint32_t)pix), x = pix - row * fc.W;
            const float dv = dither_noise(x, fc.H - 1 - row, inv_w, inv_h) * kDitherScale * f.dither;
            for (int k = 0; k < 3; ++k) d[k] = d[k] + dv;
        }
        uint8_t q[3];
        for (int k = 0; k < 3; ++k) q[k] = quantize8(d[k]);
        out[pix] = make_uchar4(q[0], q[1], q[2], 255);
    }
}

template <int VIEW>
void launch_view(bool gamma, bool dither, int grid, hipStream_t st, const FrameConsts& fc, const FilmicArgs& a,
                 const float* srgb, const float4* film, uchar4* out) {
    if (dither) {
        if (gamma) k_view<VIEW, true, true><<<grid, 256, 0, st>>>(fc, a, srgb, film, out);
        else k_view<VIEW, false, true><<<grid, 256, 0, st>>>(fc, a, srgb, film, out);
    } else {
        if (gamma) k_view<VIEW, true, false><<<grid, 256, 0, st>>>(fc, a, srgb, film, out);
        else k_view<VIEW, false, false><<<grid, 256, 0, st>>>(fc, a, srgb, film, out);
    }
}

bool read_lines(const std::string& path, std::vector<std::string>& lines, std::string& err) {
    std::ifstream in(path);
    if (!in) {
        err = "cannot open " + path;
        return false;
    }
    std::string l;
    while (std::getline(in, l)) {
        if (!l.empty() && l.back() == '\r') l.pop_back();
        lines.push_back(l);
    }
    return true;
}

}  // namespace

// OCIO's .spi3d (Sony Pictures Imageworks): "SPILUT 1.0", "3 3", "N N N",
// then one line "i j k r g b" per cube entry (i indexes red).
bool parse_spi3d(const std::string& path, int& n3, std::vector<float>& cube, std::string& err) {
    std::vector<std::string> L;
    if (!read_lines(path, L, err)) return false;
    if (L.size() < 3 || L[0].rfind("SPILUT", 0) != 0) {
        err = path + ": not an SPILUT file";
        return false;
    }
    int na = 0, nb = 0, nc = 0;
    {
        std::istringstream s(L[2]);
        if (!(s >> na >> nb >> nc) || na != nb || na != nc || na < 2 || na > 256) {
            err = path + ": bad cube size line '" + L[2] + "'";
            return false;
        }
    }
    const int n = na;
    n3 = n;
    cube.assign((size_t)n * n * n * 3, 0.f);
    std::vector<char> seen((size_t)n * n * n, 0);
    size_t count = 0;
    for (size_t li = 3; li < L.size(); ++li) {
        std::istringstream s(L[li]);
        int i, j, k;
        double r, g, b;  // decimal -> double -> float, as the oracle's reader rounds
        if (!(s >> i)) continue;  // blank line
        if (!(s >> j >> k >> r >> g >> b) || i < 0 || j < 0 || k < 0 || i >= n || j >= n || k >= n) {
            err = path + ": bad entry line " + std::to_string(li + 1);
            return false;
        }
        const size_t e = ((size_t)i * n + j) * n + k;
        if (!seen[e]) ++count;
        seen[e] = 1;
        cube[3 * e] = (float)r;
        cube[3 * e + 1] = (float)g;
        cube[3 * e + 2] = (float)b;
    }
    if (count != (size_t)n * n * n) {
        err = path + ": " + std::to_string(count) + " of " + std::to_string((size_t)n * n * n) + " cube entries";
        return false;
    }
    return true;
}

// OCIO's .spi1d: "Version 1", "From lo hi", "Length N", "Components C",
// "{", N lines of C values, "}".
bool parse_spi1d(const std::string& path, Curve1& out, std::string& err) {
    std::vector<std::string> L;
    if (!read_lines(path, L, err)) return false;
    int n = -1, comps = -1;
    double lo = 0.0, hi = 1.0;
    size_t li = 0;
    for (; li < L.size(); ++li) {
        std::istringstream s(L[li]);
        std::string key;
        if (!(s >> key)) continue;
        if (key == "Version") continue;
        if (key == "From") {
            if (!(s >> lo >> hi) || !(hi > lo)) {
                err = path + ": bad From line";
                return false;
            }
        } else if (key == "Length") {
            s >> n;
        } else if (key == "Components") {
            s >> comps;
        } else if (key == "{") {
            ++li;
            break;
        } else {
            err = path + ": unexpected '" + key + "'";
            return false;
        }
    }
    if (n < 2 || n > (1 << 20) || (comps != 1 && comps != 3)) {
        err = path + ": bad Length/Components";
        return false;
    }
    out.n = n;
    out.comps = comps;
    out.lo = (float)lo;
    out.hi = (float)hi;
    out.v.clear();
    for (; li < L.size(); ++li) {
        std::istringstream s(L[li]);
        std::string tok;
        while (s >> tok) {
            if (tok == "}") goto done;
            out.v.push_back((float)std::stod(tok));
        }
    }
done:
    if (out.v.size() != (size_t)n * comps) {
        err = path + ": " + std::to_string(out.v.size()) + " values, expected " + std::to_string((size_t)n * comps);
        return false;
    }
    return true;
}

namespace {

// dir/luts/name or dir/name, "" if neither is there
std::string find_lut(const std::string& dir, const char* name) {
    for (const std::string& sub : {std::string("/luts/"), std::string("/")}) {
        const std::string p = dir + sub + name;
        if (std::ifstream(p)) return p;
    }
    return "";
}

}  // namespace

bool load_filmic_luts(const std::string& dir, FilmicLuts& out, std::string& err) {
    const char* names[2] = {"filmic_desat65cube.spi3d", "filmic_to_0-70_1-03.spi1d"};
    std::string paths[2];
    for (int k = 0; k < 2; ++k) {
        paths[k] = find_lut(dir, names[k]);
        if (paths[k].empty()) {
            err = std::string("no ") + names[k] + " under " + dir + " (or its luts/)";
            return false;
        }
    }
    if (!parse_spi3d(paths[0], out.n3, out.cube, err) || !parse_spi1d(paths[1], out.base, err)) return false;
    // optional: a look's curve, the false-colour cube
    for (int id = 0; id < kNumLooks; ++id) {
        out.look[id] = Curve1{};
        if (!kLooks[id].file) continue;
        const std::string p = find_lut(dir, kLooks[id].file);
        if (!p.empty() && !parse_spi1d(p, out.look[id], err)) return false;
    }
    out.nf = 0;
    out.fcube.clear();
    const std::string p = find_lut(dir, kFalseColorFile);
    if (!p.empty() && !parse_spi3d(p, out.nf, out.fcube, err)) return false;
    return true;
}

namespace {

void upload_cube(const std::vector<float>& src, int n, DevBuf<float4>& dst) {
    const size_t nc = (size_t)n * n * n;
    if (nc == 0) return;
    std::vector<float4> c(nc);
    for (size_t i = 0; i < nc; ++i) c[i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.f);
    dst.ensure(nc);
    RR_HIP(hipMemcpy(dst.ptr, c.data(), nc * sizeof(float4), hipMemcpyHostToDevice));
}

}  // namespace

void Curve1Dev::upload(const Curve1& c) {
    n = 0;  // an absent curve leaves none behind
    if (c.n == 0) return;
    v.ensure(c.v.size());
    RR_HIP(hipMemcpy(v.ptr, c.v.data(), c.v.size() * sizeof(float), hipMemcpyHostToDevice));
    n = c.n;
    comps = c.comps;
    lo = c.lo;
    hi = c.hi;
}

void FilmicDev::upload(const FilmicLuts& l, const std::string& from) {
    upload_cube(l.cube, l.n3, cube);
    n3 = l.n3;
    base.upload(l.base);
    for (int id = 0; id < kNumLooks; ++id) look[id].upload(l.look[id]);
    nf = 0;
    upload_cube(l.fcube, l.nf, fcube);
    nf = l.nf;
    dir = from;
    ready = true;
}

void FilmicDev::release() {
    cube.release();
    base.v.release();
    base.n = 0;
    for (auto& c : look) {
        c.v.release();
        c.n = 0;
    }
    fcube.release();
    nf = 0;
    ready = false;
    dir.clear();
}

void view_device(const FilmicArgs& a, const FrameConsts& fc, const float* srgb, const float4* film, uchar4* out,
                 hipStream_t st) {
    const int view = fc.view_transform;
    if (view >= RR_VIEW_FILMIC && (!a.cube || (view == RR_VIEW_FILMIC && !a.lut1) ||
                                   (view == RR_VIEW_FALSE_COLOR && !a.fcube)))
        throw std::runtime_error(std::string(view_name(view)) + " view transform without its LUTs");
    if (view == RR_VIEW_STANDARD && !srgb) throw std::runtime_error("Standard view transform without its table");
    const bool gamma = a.inv_gamma != 0.0f, dither = a.dither > 0.0f;
    if (dither && (fc.W <= 0 || fc.H <= 0 || (long long)fc.W * fc.H != fc.npix))
        throw std::runtime_error("dither needs the frame's width and height");
    const int grid = std::max(1, std::min((fc.npix + 255) / 256, 4096));
    switch (view) {
    case RR_VIEW_STANDARD: launch_view<RR_VIEW_STANDARD>(gamma, dither, grid, st, fc, a, srgb, film, out); break;
    case RR_VIEW_RAW: launch_view<RR_VIEW_RAW>(gamma, dither, grid, st, fc, a, srgb, film, out); break;
    case RR_VIEW_FILMIC: launch_view<RR_VIEW_FILMIC>(gamma, dither, grid, st, fc, a, srgb, film, out); break;
    case RR_VIEW_FILMIC_LOG: launch_view<RR_VIEW_FILMIC_LOG>(gamma, dither, grid, st, fc, a, srgb, film, out); break;
    case RR_VIEW_FALSE_COLOR: launch_view<RR_VIEW_FALSE_COLOR>(gamma, dither, grid, st, fc, a, srgb, film, out); break;
    default: throw std::runtime_error("unsupported view transform");
    }
    RR_HIP(hipGetLastError());
}

void display_gamma_host(const float* in, size_t n, float g, float* out) {
    const float inv = 1.0f / g;
    for (size_t i = 0; i < n; ++i) out[i] = display_gamma(in[i], inv);
}

void sin_fixed_host(const float* in, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = sin_fixed(in[i]);
}

void dither_noise_host(int w, int h, float* out) {
    const float inv_w = 1.0f / (float)w, inv_h = 1.0f / (float)h;
    for (int r = 0; r < h; ++r)
        for (int x = 0; x < w; ++x) out[(size_t)r * w + x] = dither_noise(x, h - 1 - r, inv_w, inv_h);
}

}  // namespace rr

