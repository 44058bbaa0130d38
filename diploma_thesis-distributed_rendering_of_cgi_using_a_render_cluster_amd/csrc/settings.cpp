// Output settings: their ranges, their environment spellings, and the file a
// frame gets from them. See settings.hpp.
#include "settings.hpp"

#include <algorithm>
#include <cstdlib>

#include "looks.hpp"
#include "scene.hpp"

namespace rr {

bool set_png_depth(OutputSettings& s, int depth, std::string& err) {
    if (depth != 0 && depth != 8 && depth != 16) {
        err = "PNG depth must be 0 (the scene's), 8 or 16";
        return false;
    }
    s.png_depth = depth;
    return true;
}

bool set_exr_depth(OutputSettings& s, int depth, std::string& err) {
    if (depth != 0 && depth != 16 && depth != 32) {
        err = "EXR depth must be 0 (the scene's), 16 or 32";
        return false;
    }
    s.exr_depth = depth;
    return true;
}

bool set_exr_codec(OutputSettings& s, int codec, std::string& err) {
    if (codec < RR_EXR_CODEC_SCENE || codec > RR_EXR_CODEC_DWAB) {
        err = "EXR codec must be RR_EXR_CODEC_SCENE (0) or one of RR_EXR_CODEC_NONE (1) .. RR_EXR_CODEC_DWAB (10)";
        return false;
    }
    s.exr_codec = codec;
    return true;
}

bool valid_color_mode(int mode) {
    return mode == RR_COLOR_SCENE || mode == RR_COLOR_BW || mode == RR_COLOR_RGB || mode == RR_COLOR_RGBA;
}

bool set_color_mode(OutputSettings& s, int mode, std::string& err) {
    if (!valid_color_mode(mode)) {
        err = "colour mode must be RR_COLOR_SCENE (0), RR_COLOR_BW (1), RR_COLOR_RGB (3) or RR_COLOR_RGBA (4)";
        return false;
    }
    s.color_mode = mode;
    return true;
}

bool set_look(OutputSettings& s, const char* name, std::string& err) {
    const int id = (name && *name) ? look_id(name) : -1;
    if (name && *name && id < 0) {
        err = std::string("unknown look '") + name + "'";
        return false;
    }
    s.look = id;
    return true;
}

bool set_display_gamma(OutputSettings& s, double gamma, std::string& err) {
    if (!(gamma >= 0.0) || gamma > (double)kGammaMax) {
        err = "display gamma must be 0 (the scene's) or above 0 and at most 5";
        return false;
    }
    s.gamma = (float)gamma;
    return true;
}

bool set_dither(OutputSettings& s, double intensity, std::string& err) {
    if (intensity != (double)RR_DITHER_SCENE && (!(intensity >= 0.0) || intensity > (double)kDitherMax)) {
        err = "dither intensity must be in [0, 2], or RR_DITHER_SCENE (the scene's)";
        return false;
    }
    s.dither = (float)intensity;
    return true;
}

bool valid_png_compression(int v) { return v >= RR_PNG_COMPRESSION_SCENE && v <= 100; }

bool set_png_compression(OutputSettings& s, int percent, std::string& err) {
    if (!valid_png_compression(percent)) {
        err = "PNG compression must be 0 .. 100, RR_PNG_COMPRESSION_LEGACY or RR_PNG_COMPRESSION_SCENE";
        return false;
    }
    s.png_compression = percent;
    return true;
}

bool set_extra_outputs(OutputSettings& s, const char* spec, std::string& err) {
    std::vector<ExtraOutput> list;
    const std::string text(spec ? spec : "");
    for (size_t at = 0; !text.empty() && at <= text.size();) {
        const size_t end = std::min(text.find(',', at), text.size());
        const std::string entry = text.substr(at, end - at);
        at = end + 1;
        const size_t colon = entry.find(':');
        const std::string name = entry.substr(0, colon), factor = colon == std::string::npos ? "1" : entry.substr(colon + 1);
        ExtraOutput e;
        e.format = find_format(name.c_str());
        if (!e.format) {
            err = "extra output '" + entry + "': " + unsupported_format(name);
            return false;
        }
        if (factor != "1" && factor != "2" && factor != "4" && factor != "8") {
            err = "extra output '" + entry + "': the factor must be 1, 2, 4 or 8";
            return false;
        }
        e.reduce = factor[0] - '0';
        for (const ExtraOutput& o : list)
            if (o.reduce == e.reduce && std::string(o.format->ext) == e.format->ext) {
                err = "extra output '" + entry + "' would write the same file as '" + o.format->name + "'";
                return false;
            }
        if ((int)list.size() == RR_MAX_FRAME_OUTPUTS - 1) {
            err = "at most " + std::to_string(RR_MAX_FRAME_OUTPUTS - 1) + " extra outputs (a frame writes " +
                  std::to_string(RR_MAX_FRAME_OUTPUTS) + " files at most)";
            return false;
        }
        list.push_back(e);
    }
    s.extra_outputs = list;
    return true;
}

bool set_region(OutputSettings& s, int x0, int y0, int x1, int y1, bool crop, std::string& err) {
    constexpr int kMax = 1 << 30;
    const bool in_range = x0 >= -kMax && y0 >= -kMax && x1 <= kMax && y1 <= kMax;
    if (!in_range || x0 >= x1 || y0 >= y1) {
        err = "region (" + std::to_string(x0) + ", " + std::to_string(y0) + ", " + std::to_string(x1) + ", " +
              std::to_string(y1) + ") must have x0 < x1 and y0 < y1, each within +-2^30";
        return false;
    }
    s.region_on = true;
    s.region = RegionRect{x0, y0, x1, y1};
    s.region_crop = crop;
    return true;
}

bool resolve_region(const OutputSettings& s, const RenderDesc& r, int W, int H, FrameRegion& out, std::string& err) {
    out = FrameRegion{};
    RegionRect asked;
    if (s.region_from_scene && r.has_border) {
        asked = region_of_border(r.border_min_x, r.border_max_x, r.border_min_y, r.border_max_y, W, H);
        out.crop = r.border_crop;
    } else if (s.region_on) {
        asked = s.region;
        out.crop = s.region_crop;
    } else {
        return true;
    }
    out.r = region_clamp(asked, W, H);
    if (out.r.empty()) {
        err = "region (" + std::to_string(asked.x0) + ", " + std::to_string(asked.y0) + ", " +
              std::to_string(asked.x1) + ", " + std::to_string(asked.y1) + ") is empty inside the " +
              std::to_string(W) + " x " + std::to_string(H) + " frame";
        return false;
    }
    out.on = !(out.r.w() == W && out.r.h() == H);
    return true;
}

namespace {

// A whole text as one number, as strtol / strtod read it.
bool whole_long(const char* t, long& v) {
    char* end = nullptr;
    v = std::strtol(t, &end, 10);
    return end != t && !*end;
}
bool whole_double(const char* t, double& v) {
    char* end = nullptr;
    v = std::strtod(t, &end);
    return end != t && !*end;
}

// The text of one variable through its setter. The spellings: "" is the
// setting's default; a depth is "0", "8", "16", "32" and no other way of
// writing those numbers; a colour mode is its Blender name; the values that
// rr.h gives a negative constant are spelled "scene" (and LEGACY ""), never as
// that number.
bool apply_text(OutputSettings& s, const std::string& var, const char* t, std::string& err) {
    const std::string v(t);
    long n = 0;
    double x = 0.0;
    if (var == "RR_DEVICE_PNG") {
        set_device_png(s, v == "1");
        return true;
    }
    if (var == "RR_PNG_DEPTH" || var == "RR_EXR_DEPTH") {
        if (v.empty()) n = 0;
        else if (!whole_long(t, n) || std::to_string(n) != v) {
            err = "not a depth";
            return false;
        }
        const int d = n == (long)(int)n ? (int)n : -1;
        return var == "RR_PNG_DEPTH" ? set_png_depth(s, d, err) : set_exr_depth(s, d, err);
    }
    if (var == "RR_EXR_CODEC") {
        if (v.empty()) return set_exr_codec(s, RR_EXR_CODEC_SCENE, err);
        const int k = exr_codec_of_name(t);
        if (k < 0) {
            err = "EXR codec must be NONE, RLE, ZIPS, ZIP, PIZ, PXR24, B44, B44A, DWAA or DWAB";
            return false;
        }
        return set_exr_codec(s, k, err);
    }
    if (var == "RR_COLOR_MODE") {
        if (v.empty()) return set_color_mode(s, RR_COLOR_SCENE, err);
        if (v == "BW") return set_color_mode(s, RR_COLOR_BW, err);
        if (v == "RGB") return set_color_mode(s, RR_COLOR_RGB, err);
        if (v == "RGBA") return set_color_mode(s, RR_COLOR_RGBA, err);
        err = "colour mode must be BW, RGB or RGBA";
        return false;
    }
    if (var == "RR_LOOK") return set_look(s, t, err);
    if (var == "RR_DISPLAY_GAMMA") {
        if (v.empty()) return set_display_gamma(s, 0.0, err);
        if (!whole_double(t, x)) {
            err = "not a number";
            return false;
        }
        return set_display_gamma(s, x, err);
    }
    if (var == "RR_DITHER") {
        if (v.empty()) return set_dither(s, 0.0, err);
        if (v == "scene") return set_dither(s, (double)RR_DITHER_SCENE, err);
        if (!whole_double(t, x) || x == (double)RR_DITHER_SCENE) {
            err = "not a number in [0, 2] or 'scene'";
            return false;
        }
        return set_dither(s, x, err);
    }
    if (var == "RR_PNG_COMPRESSION") {
        if (v.empty()) return true;  // the context's own (LEGACY on a new one)
        if (v == "scene") return set_png_compression(s, RR_PNG_COMPRESSION_SCENE, err);
        if (!whole_long(t, n) || n != (long)(int)n || n == RR_PNG_COMPRESSION_LEGACY || n == RR_PNG_COMPRESSION_SCENE) {
            err = "not a number in 0 .. 100 or 'scene'";
            return false;
        }
        return set_png_compression(s, (int)n, err);
    }
    if (var == "RR_EXTRA_OUTPUTS") return set_extra_outputs(s, t, err);
    if (var == "RR_REGION") {
        if (v.empty()) {
            set_region_off(s);
            set_region_from_scene(s, false);
            return true;
        }
        if (v == "scene") {
            set_region_from_scene(s, true);
            return true;
        }
        long f[5] = {0, 0, 0, 0, 0};
        int nf = 0;
        for (size_t at = 0; at <= v.size(); ++nf) {
            const size_t end = std::min(v.find(',', at), v.size());
            const std::string field = v.substr(at, end - at);
            at = end + 1;
            if (nf == 5 || !whole_long(field.c_str(), f[nf]) || std::to_string(f[nf]) != field ||
                f[nf] != (long)(int)f[nf]) {
                nf = -1;
                break;
            }
        }
        if (nf < 4 || (nf == 5 && f[4] != 0 && f[4] != 1)) {
            err = "not 'x0,y0,x1,y1[,crop]' (whole numbers, crop 0 or 1) or 'scene'";
            return false;
        }
        return set_region(s, (int)f[0], (int)f[1], (int)f[2], (int)f[3], f[4] == 1, err);
    }
    err = "not an output setting";
    return false;
}

constexpr const char* kEnvVars[] = {"RR_PNG_DEPTH",     "RR_EXR_DEPTH",       "RR_EXR_CODEC", "RR_COLOR_MODE", "RR_LOOK",
                                    "RR_DISPLAY_GAMMA", "RR_PNG_COMPRESSION", "RR_DITHER",    "RR_DEVICE_PNG",
                                    "RR_EXTRA_OUTPUTS", "RR_REGION"};

}  // namespace

bool setting_from_text(OutputSettings& s, const std::string& var, const char* text, std::string& err) {
    std::string why;
    if (apply_text(s, var, text, why)) return true;
    err = var + "='" + text + "': " + why;
    return false;
}

bool settings_from_env(OutputSettings& s, std::string& err) {
    OutputSettings t = s;
    for (const char* var : kEnvVars)
        if (const char* text = std::getenv(var))
            if (!setting_from_text(t, var, text, err)) return false;
    s = t;
    return true;
}

const char* coder_ext(Coder k) {
    if (k == Coder::HostRgba) k = Coder::Png8;  // the host's file of the same format
    for (const Format& f : kFormats)
        if (f.coder == k || (f.deep_depth && f.deep == k)) return f.ext;
    return "";
}

// kFormats' names as a refusal lists them, "A, B and C". film: 1 the formats
// that need the float film, 0 those of an RGBA8 image, -1 all.
static std::string format_names(int film) {
    std::string s, last;
    for (const Format& f : kFormats) {
        if (film >= 0 && coder_info(f.coder).film != (film != 0)) continue;
        if (!last.empty()) s += (s.empty() ? "" : ", ") + last;
        last = f.name;
    }
    return s.empty() ? last : s + " and " + last;
}

std::string unsupported_format(const std::string& format, bool rgba8) {
    const std::string head = "unsupported output format '" + format + "'";
    if (!rgba8) return head + " (" + format_names(-1) + " are supported)";
    if (known_format(format.c_str()))
        return head + " for an RGBA8 image: it needs the float film (" + format_names(0) + " are supported here)";
    return head + " (" + format_names(0) + " are supported here; " + format_names(1) + " need the float film)";
}

int resolve_color_mode(int mode, bool no_alpha) {
    if (mode == 0) return no_alpha ? RR_COLOR_RGB : RR_COLOR_RGBA;
    return (no_alpha && mode == RR_COLOR_RGBA) ? RR_COLOR_RGB : mode;
}

FrameOutput resolve_output(const OutputSettings& s, const RenderDesc& r, const char* format, bool has_path,
                           int jpeg_quality) {
    const Format* f = has_path ? find_format(format) : nullptr;
    FrameOutput o;
    if (f) {
        // the context's depth, at 0 the scene's: HALF or FLOAT channels, 8 or 16 bits per sample
        const int depth = f->coder == Coder::Exr ? (s.exr_depth ? s.exr_depth : r.exr_depth)
                                                 : (s.png_depth ? s.png_depth : r.color_depth);
        o.coder = format_coder(*f, depth);
        // 8 bits: the host coder unless the context asks (16 has no host coder)
        if (o.coder == Coder::Png8 && !s.device_png) o.coder = Coder::HostRgba;
        o.tga_raw = f->tga_raw;
    }
    // the context's mode, at 0 the scene's, at 0 again the format's own layout
    o.color_mode = resolve_color_mode(s.color_mode ? s.color_mode : r.color_mode, f && f->no_alpha);
    // the context's setting, at SCENE the scene's (-1, legacy, where it has no field)
    o.png_compression = s.png_compression == RR_PNG_COMPRESSION_SCENE ? r.png_compression : s.png_compression;
    // the context's codec, at SCENE the scene's (ZIP where it has no field)
    o.exr_codec = s.exr_codec != RR_EXR_CODEC_SCENE ? s.exr_codec : r.exr_codec;
    o.quality = jpeg_quality;
    return o;
}

std::string extra_output_path(const std::string& path, int reduce) {
    return reduce == 1 ? path : path + ".r" + std::to_string(reduce);
}

void add_extra_outputs(const OutputSettings& s, const RenderDesc& r, std::vector<OutputRequest>& list) {
    if (list.empty()) return;
    const OutputRequest own = list[0];
    for (const ExtraOutput& e : s.extra_outputs)
        list.push_back({extra_output_path(own.path, e.reduce), e.format->name, own.quality, e.reduce});
    if (s.extra_outputs.empty() && r.use_preview && own.format == "OPEN_EXR")
        list.push_back({own.path, "JPEG", own.quality, 1});
}

int check_outputs(const std::vector<OutputRequest>& list, std::string& err) {
    if (list.empty() || (int)list.size() > RR_MAX_FRAME_OUTPUTS) {
        err = "a frame writes 1 .. " + std::to_string(RR_MAX_FRAME_OUTPUTS) + " files, not " + std::to_string(list.size());
        return RR_EINVAL;
    }
    std::vector<std::string> files;
    for (const OutputRequest& o : list) {
        if (!(o.reduce == 1 || o.reduce == 2 || o.reduce == 4 || o.reduce == 8)) {
            err = "output reduce must be 1, 2, 4 or 8, got " + std::to_string(o.reduce);
            return RR_EINVAL;
        }
        const Format* f = find_format(o.format.c_str());
        if (!f) {
            err = unsupported_format(o.format);
            return RR_ENOTSUP;
        }
        if (f->coder == Coder::Jpeg && (o.quality < 1 || o.quality > 100)) {
            err = "jpeg_quality must be 1..100";
            return RR_EINVAL;
        }
        files.push_back(o.path + f->ext);
    }
    for (size_t i = 0; i < files.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (files[i] == files[j]) {
                err = "two outputs of one frame would write " + files[i];
                return RR_EINVAL;
            }
    return RR_OK;
}

int png_compression_of(const OutputSettings& s) {
    return s.png_compression >= 0 ? s.png_compression : RR_PNG_COMPRESSION_LEGACY;
}

int exr_codec_of(const OutputSettings& s) {
    return s.exr_codec != RR_EXR_CODEC_SCENE ? s.exr_codec : RR_EXR_CODEC_ZIP;
}

std::string exr_codec_warning(const FrameOutput& fo) {
    if ((fo.coder != Coder::Exr && fo.coder != Coder::Exr32) || exr_codec_built(fo.exr_codec)) return "";
    return std::string("OPEN_EXR with codec ") + exr_codec_name(fo.exr_codec) +
           ": that codec is not built, the file is ZIP (lossless, 16 scanlines a chunk)";
}

float dither_of(const OutputSettings& s) { return s.dither > 0.f ? s.dither : 0.f; }

}  // namespace rr
