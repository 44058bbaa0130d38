// Filmic view transform: OCIO LUT parsing (host) and the per-pixel chain
// (device). See view.hpp for the chain and where it comes from. The float
// operations are written in the order oracle/rr_oracle.c orc_filmic uses, so
// the 8-bit output is bit-identical to the oracle's (tests/test_gpu_view.py).
#pragma clang fp contract(off)

#include "view.hpp"
#include "view_filmic.h"

#include <fstream>
#include <sstream>

namespace rr {

namespace {

__global__ __launch_bounds__(256) void k_view_filmic(FrameConsts fc, FilmicArgs f, const float4* __restrict__ film,
                                                     uchar4* __restrict__ out) {
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < fc.npix; pix += gridDim.x * 256) {
        const float4 acc = film[pix];
        const float c[3] = {acc.x * fc.inv_spp * fc.exposure_scale, acc.y * fc.inv_spp * fc.exposure_scale,
                            acc.z * fc.inv_spp * fc.exposure_scale};
        float d[3];
        filmic_display(f, c, d);
        uint8_t q[3];
        for (int k = 0; k < 3; ++k) q[k] = quantize8(d[k]);
        out[pix] = make_uchar4(q[0], q[1], q[2], 255);
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
bool parse_spi3d(const std::string& path, FilmicLuts& out, std::string& err) {
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
    out.n3 = n;
    out.cube.assign((size_t)n * n * n * 3, 0.f);
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
        out.cube[3 * e] = (float)r;
        out.cube[3 * e + 1] = (float)g;
        out.cube[3 * e + 2] = (float)b;
    }
    if (count != (size_t)n * n * n) {
        err = path + ": " + std::to_string(count) + " of " + std::to_string((size_t)n * n * n) + " cube entries";
        return false;
    }
    return true;
}

// OCIO's .spi1d: "Version 1", "From lo hi", "Length N", "Components C",
// "{", N lines of C values, "}".
bool parse_spi1d(const std::string& path, FilmicLuts& out, std::string& err) {
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
    out.n1 = n;
    out.comps = comps;
    out.lo1 = (float)lo;
    out.hi1 = (float)hi;
    out.lut1.clear();
    for (; li < L.size(); ++li) {
        std::istringstream s(L[li]);
        std::string tok;
        while (s >> tok) {
            if (tok == "}") goto done;
            out.lut1.push_back((float)std::stod(tok));
        }
    }
done:
    if (out.lut1.size() != (size_t)n * comps) {
        err = path + ": " + std::to_string(out.lut1.size()) + " values, expected " + std::to_string((size_t)n * comps);
        return false;
    }
    return true;
}

bool load_filmic_luts(const std::string& dir, FilmicLuts& out, std::string& err) {
    const char* names[2] = {"filmic_desat65cube.spi3d", "filmic_to_0-70_1-03.spi1d"};
    std::string paths[2];
    for (int k = 0; k < 2; ++k) {
        for (const std::string& sub : {std::string("/luts/"), std::string("/")}) {
            const std::string p = dir + sub + names[k];
            if (std::ifstream(p)) {
                paths[k] = p;
                break;
            }
        }
        if (paths[k].empty()) {
            err = std::string("no ") + names[k] + " under " + dir + " (or its luts/)";
            return false;
        }
    }
    return parse_spi3d(paths[0], out, err) && parse_spi1d(paths[1], out, err);
}

void FilmicDev::upload(const FilmicLuts& l, const std::string& from) {
    const size_t n3c = (size_t)l.n3 * l.n3 * l.n3;
    std::vector<float4> c(n3c);
    for (size_t i = 0; i < n3c; ++i) c[i] = make_float4(l.cube[3 * i], l.cube[3 * i + 1], l.cube[3 * i + 2], 0.f);
    cube.ensure(n3c);
    lut1.ensure(l.lut1.size());
    RR_HIP(hipMemcpy(cube.ptr, c.data(), n3c * sizeof(float4), hipMemcpyHostToDevice));
    RR_HIP(hipMemcpy(lut1.ptr, l.lut1.data(), l.lut1.size() * sizeof(float), hipMemcpyHostToDevice));
    n3 = l.n3;
    n1 = l.n1;
    comps = l.comps;
    lo1 = l.lo1;
    hi1 = l.hi1;
    dir = from;
    ready = true;
}

void FilmicDev::release() {
    cube.release();
    lut1.release();
    ready = false;
    dir.clear();
}

void view_filmic_device(const FilmicDev& f, const FrameConsts& fc, const float4* film, uchar4* out,
                        hipStream_t st) {
    if (!f.ready) throw std::runtime_error("Filmic view transform without LUTs");
    const FilmicArgs a = f.args();
    const int grid = std::max(1, std::min((fc.npix + 255) / 256, 4096));
    k_view_filmic<<<grid, 256, 0, st>>>(fc, a, film, out);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
