// The view settings of Blender 3.6's colour management applied after the
// render: the Filmic family of view transforms (RR_VIEW_FILMIC with its looks,
// RR_VIEW_FILMIC_LOG, RR_VIEW_FALSE_COLOR) through the OCIO LUTs of a Blender
// colour-management directory, and the display gamma of every view (DESIGN.md
// §4, "View transforms").
//
// The reference renders 01_simple-animation with Blender 3.6's "Filmic" view
// (the .blend's view settings), which Blender applies through
// OpenColorIO with its bundled config (datafiles/colormanagement/config.ocio,
// third-party, not in the reference tree). For display "sRGB", view "Filmic",
// look "None" that config's chain is, per channel unless noted:
//   1. AllocationTransform lg2 [-12.473931188, 12.526068812]:
//        a = (log2(max(x, FLT_MIN)) + 12.473931188) / 25
//   2. FileTransform filmic_desat65cube.spi3d, interpolation best
//        (tetrahedral, RGB -> RGB, input clamped to the cube)
//   3. AllocationTransform uniform [0, 0.66]:  L = b / 0.66   ("Filmic Log")
//   4. FileTransform filmic_to_0-70_1-03.spi1d, interpolation linear
//        (display-referred sRGB code values)
// The other settings, from the same config:
//   - a look is "contrast curve, then the inverse base curve" in Filmic Log,
//     and the display's base curve follows: the pair cancels, so the look's
//     curve (kLooks) takes the place of step 4;
//   - view "Filmic Log" ends after step 3;
//   - view "False Color" takes L's luminance (Rec.709 weights 0.2126729,
//     0.7151521, 0.0721750) through filmic_false_color.spi3d;
//   - the display gamma g is an exponent 1 / g on the display-referred value
//     (ExponentTransform after the view; view_filmic.h display_gamma).
// The constants, file names and the look table are restated from that config
// (not present here); Blender's LUT files are not in the image either, so the
// chain is tested bit-exact against the oracle and a numpy restatement on
// synthetic LUTs written in the same formats, and its parity with Blender's
// own output stays unpinned.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device.hpp"
#include "looks.hpp"

namespace rr {

// The looks table (kLooks, look_id), view_name, kFalseColorFile, kGammaMax and
// kDitherMax are host data of their own: looks.hpp.

// A 1D LUT as parsed from its file (host).
struct Curve1 {
    int n = 0, comps = 1;      // length (0: not loaded), components (1: one curve for every channel)
    std::vector<float> v;      // n x comps
    float lo = 0.f, hi = 1.f;  // input domain ("From")
};

// LUTs as parsed from the files (host).
struct FilmicLuts {
    int n3 = 0;                // cube edge
    std::vector<float> cube;   // n3^3 x (r, g, b); entry (i, j, k) at (i * n3 + j) * n3 + k
    Curve1 base;               // filmic_to_0-70_1-03.spi1d
    Curve1 look[kNumLooks];    // by look id, where kLooks names a file and the file is there
    int nf = 0;                // false-colour cube edge (0: not loaded)
    std::vector<float> fcube;  // as cube
};

// Parse an OCIO .spi3d / .spi1d file. false + err on failure.
bool parse_spi3d(const std::string& path, int& n3, std::vector<float>& cube, std::string& err);
bool parse_spi1d(const std::string& path, Curve1& out, std::string& err);

// Find and parse Blender's Filmic LUTs under `dir` (dir/luts/ or dir/): the
// desaturation cube and the base curve are required, the looks' curves and the
// false-colour cube are taken when present (a malformed one fails the load).
bool load_filmic_luts(const std::string& dir, FilmicLuts& out, std::string& err);

// The LUTs on one device.
struct Curve1Dev {
    DevBuf<float> v;
    int n = 0, comps = 1;
    float lo = 0.f, hi = 1.f;
    void upload(const Curve1& c);
};
struct FilmicDev {
    DevBuf<float4> cube;  // n3^3, (r, g, b, 0)
    int n3 = 0;
    Curve1Dev base, look[kNumLooks];
    DevBuf<float4> fcube;
    int nf = 0;
    bool ready = false;  // the two base LUTs are loaded
    std::string dir;
    void upload(const FilmicLuts& l, const std::string& from);
    void release();
    // whether a frame can be given this look / the False Color view
    bool has_look(int id) const { return ready && (kLooks[id].file == nullptr || look[id].n > 0); }
    bool has_false_color() const { return ready && nf > 0; }
    // the arguments of a Filmic-family frame with look `id` (has_look holds)
    FilmicArgs args(int id = 0) const {
        const Curve1Dev& c = kLooks[id].file ? look[id] : base;
        return FilmicArgs{cube.ptr, c.v.ptr, n3, c.n, c.comps, c.lo, c.hi, 0.0f, fcube.ptr, nf, 0.0f};
    }
};

// FilmicArgs::inv_gamma of a display gamma g in (0, kGammaMax].
inline float inv_gamma_of(float g) { return g == 1.0f ? 0.0f : 1.0f / g; }

// Whether a frame's rgba8 comes from view_device (the second pass over the
// film) and not from the render kernels' own tonemap (paths.hpp: Standard and
// Raw at gamma 1 without dither).
inline bool view_needs_pass(int view_transform, float gamma, float dither) {
    return view_transform >= RR_VIEW_FILMIC || gamma != 1.0f || dither > 0.0f;
}

// rgba8 = quantize8(view(film sums * inv_spp * exposure_scale)) for every
// pixel: fc.view_transform with a's LUTs and display gamma. srgb: the 8-bit
// path's sRGB table (DevPaths::srgb_lut; Standard only). a.dither > 0: the
// dither of dither.h before the quantiser, which needs fc.W, fc.H (W H = npix)
// and fc.div_w.
void view_device(const FilmicArgs& a, const FrameConsts& fc, const float* srgb, const float4* film, uchar4* out,
                 hipStream_t st);

// out[i] = display_gamma(in[i], 1 / g) on the host, g != 1 (rr_debug_display_gamma).
void display_gamma_host(const float* in, size_t n, float g, float* out);

// dither.h on the host: out[i] = sin_fixed(in[i]) (rr_debug_sin_fixed), and the
// noise n of every pixel of a w x h image, rows top to bottom
// (rr_debug_dither_noise).
void sin_fixed_host(const float* in, size_t n, float* out);
void dither_noise_host(int w, int h, float* out);

}  // namespace rr
