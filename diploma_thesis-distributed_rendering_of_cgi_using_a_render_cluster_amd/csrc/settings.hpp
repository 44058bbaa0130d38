// The output settings of a context (rr_set_* / the RR_* environment variables)
// and what file they give a frame. Host code only, no HIP header: the checks
// of tests/cpp/settings_check.cpp link settings.cpp and nothing else.
//
// A setting's valid values are stated once, in its setter. rr_set_* calls the
// setter; settings_from_env parses a variable's text and calls the same one.
#pragma once

#include <string>
#include <vector>

#include "formats.hpp"
#include "region_rule.h"
#include "rr.h"

namespace rr {

struct RenderDesc;  // scene.hpp

// One entry of rr_set_extra_outputs' list: a format of kFormats and the factor
// its file is reduced by (1, 2, 4 or 8).
struct ExtraOutput {
    const Format* format = nullptr;
    int reduce = 1;
};

struct OutputSettings {
    // 8-bit "PNG" frames are coded on the device (rr_set_device_png / RR_DEVICE_PNG)
    bool device_png = false;
    // bit depth of "PNG" frames (rr_set_png_depth / RR_PNG_DEPTH): 0 the scene's, 8, 16
    int png_depth = 0;
    // channel type of "OPEN_EXR" frames (rr_set_exr_depth / RR_EXR_DEPTH): 0 the scene's, 16 HALF, 32 FLOAT
    int exr_depth = 0;
    // compression of "OPEN_EXR" frames (rr_set_exr_codec / RR_EXR_CODEC): an RR_EXR_CODEC_* value, SCENE the scene's
    int exr_codec = RR_EXR_CODEC_SCENE;
    // colour mode of the files (rr_set_color_mode / RR_COLOR_MODE): 0 the scene's, else RR_COLOR_BW / RGB / RGBA
    int color_mode = 0;
    // look of Filmic frames (rr_set_look / RR_LOOK): a looks.hpp kLooks id, -1 the scene's
    int look = -1;
    // compression of "PNG" files (rr_set_png_compression / RR_PNG_COMPRESSION): LEGACY, SCENE or 0 .. 100
    int png_compression = RR_PNG_COMPRESSION_LEGACY;
    // display gamma (rr_set_display_gamma / RR_DISPLAY_GAMMA): 0 the scene's
    float gamma = 0.f;
    // dither of the 8-bit image (rr_set_dither / RR_DITHER): an intensity in [0, 2], RR_DITHER_SCENE the scene's
    float dither = 0.f;
    // files every frame with a path writes beside its own (rr_set_extra_outputs / RR_EXTRA_OUTPUTS)
    std::vector<ExtraOutput> extra_outputs;
    // the render region (rr_set_region / rr_set_region_off / RR_REGION): off on a new context
    bool region_on = false;
    RegionRect region;         // full-frame pixels, rows top first, half open; clamped when a frame is resolved
    bool region_crop = false;  // the outputs are the region's pixels alone; else the full frame, (0, 0, 0, 0) outside
    // a scene's render.border gives the region (rr_set_region_from_scene / RR_REGION=scene); comes before `region`
    bool region_from_scene = false;
};

// The setters. false + err for a value outside the setting's range, which
// changes nothing. Settings are read when a frame is submitted; frames in
// flight keep theirs.
inline void set_device_png(OutputSettings& s, bool on) { s.device_png = on; }
bool set_png_depth(OutputSettings& s, int depth, std::string& err);
bool set_exr_depth(OutputSettings& s, int depth, std::string& err);
bool set_exr_codec(OutputSettings& s, int codec, std::string& err);
bool set_color_mode(OutputSettings& s, int mode, std::string& err);
bool set_look(OutputSettings& s, const char* name, std::string& err);  // NULL or "": the scene's
bool set_display_gamma(OutputSettings& s, double gamma, std::string& err);
bool set_dither(OutputSettings& s, double intensity, std::string& err);
bool set_png_compression(OutputSettings& s, int percent, std::string& err);
// spec: "FORMAT[:K]" entries joined by commas, e.g. "JPEG:4,PNG": a name of
// kFormats and a factor 1 (also when left out), 2, 4 or 8; at most
// RR_MAX_FRAME_OUTPUTS - 1 entries, no two of which would write the same file.
// NULL or "": none.
bool set_extra_outputs(OutputSettings& s, const char* spec, std::string& err);
// The region: x0 < x1 and y0 < y1 (an inverted or empty rectangle is refused), each within +-2^30; beyond
// the frame is allowed and clamped when a frame is resolved.
bool set_region(OutputSettings& s, int x0, int y0, int x1, int y1, bool crop, std::string& err);
inline void set_region_off(OutputSettings& s) { s.region_on = false; }
inline void set_region_from_scene(OutputSettings& s, bool on) { s.region_from_scene = on; }

bool valid_color_mode(int mode);

// Blender's names of the OpenEXR codecs, by RR_EXR_CODEC_* value ("" for SCENE
// and anything else), and the value of a name (-1: no codec's name).
inline const char* exr_codec_name(int codec) {
    constexpr const char* names[] = {"", "NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};
    static_assert(sizeof names / sizeof *names == RR_EXR_CODEC_DWAB + 1, "a name for every value");
    return codec > RR_EXR_CODEC_SCENE && codec <= RR_EXR_CODEC_DWAB ? names[codec] : "";
}
inline int exr_codec_of_name(const std::string& name) {
    for (int k = RR_EXR_CODEC_SCENE + 1; k <= RR_EXR_CODEC_DWAB; ++k)
        if (name == exr_codec_name(k)) return k;
    return -1;
}
// The codecs that are built: a frame that asks for another is written as ZIP
// and flagged (exr_codec_warning).
inline bool exr_codec_built(int codec) {
    return codec == RR_EXR_CODEC_NONE || codec == RR_EXR_CODEC_RLE || codec == RR_EXR_CODEC_ZIP ||
           codec == RR_EXR_CODEC_PXR24;
}
// rr_set_png_compression's values: LEGACY, SCENE or a percentage.
bool valid_png_compression(int v);

// One variable's text (RR_PNG_DEPTH, RR_EXR_DEPTH, RR_EXR_CODEC, RR_COLOR_MODE, RR_LOOK,
// RR_DISPLAY_GAMMA, RR_PNG_COMPRESSION, RR_DITHER, RR_DEVICE_PNG, RR_EXTRA_OUTPUTS, RR_REGION) through its
// setter. RR_REGION: "x0,y0,x1,y1[,crop]" (crop 0 or 1), "scene" (the scene's border), "" off. A refusal's err names the variable and quotes the text.
bool setting_from_text(OutputSettings& s, const std::string& var, const char* text, std::string& err);
// Every variable that is set, in the order above. false + err: s is unchanged.
bool settings_from_env(OutputSettings& s, std::string& err);

// The coders' families (formats.hpp). A slot coder reads only its slot's rgba8 /
// film and writes slot buffers only: the next frame waits for such a frame's
// image, not for its coder.
inline bool device_deflate(Coder k) { return coder_info(k).family == Family::Deflate; }
inline bool device_body(Coder k) { return coder_info(k).family == Family::Body; }
inline bool slot_coder(Coder k) { return device_deflate(k) || device_body(k); }

// The formats a frame can be submitted with (kFormats), and the extension of a coder's files.
inline bool known_format(const char* format) { return find_format(format) != nullptr; }
const char* coder_ext(Coder k);

// What a format that is not written is refused with, listing those that are:
// a frame's (rr_frame_submit), or with rgba8 an RGBA8 image's (do_encode), for
// which the formats of the float film are not written either.
std::string unsupported_format(const std::string& format, bool rgba8 = false);

// The channels a frame's file holds (rr_set_color_mode), which is also the
// resolved mode's value: RR_COLOR_BW 1, RR_COLOR_RGB 3, RR_COLOR_RGBA 4. mode 0:
// the format's layout before there was a setting (JPEG three components, the
// others four channels). A format without alpha (Format::no_alpha):
// RGBA resolves to RGB, as in Blender, and mode 0 is RGB.
int resolve_color_mode(int mode, bool no_alpha);

// The file of one frame, resolved when the frame is submitted.
struct FrameOutput {
    Coder coder = Coder::None;
    int color_mode = RR_COLOR_RGBA;                    // the file's channels (resolve_color_mode)
    int png_compression = RR_PNG_COMPRESSION_LEGACY;   // LEGACY, or 0 .. 100
    int quality = 0;                                   // JPEG
    bool tga_raw = false;                              // Coder::Tga: no run-length packets (Format::tga_raw)
    int exr_codec = RR_EXR_CODEC_ZIP;                  // Coder::Exr, Exr32: the codec asked for, never SCENE
};

// The codec fo's OPEN_EXR file is written with: the one asked for where it is
// built, else ZIP. And what rr_last_warning says of such a file ("" for a file
// of another format or of a codec that is built).
inline int exr_codec_written(const FrameOutput& fo) { return exr_codec_built(fo.exr_codec) ? fo.exr_codec : RR_EXR_CODEC_ZIP; }
std::string exr_codec_warning(const FrameOutput& fo);

// What a frame of a scene with render settings r is written as on a context
// with settings s. format: a name of kFormats (known_format, checked by the
// caller); without a path there is no file (Coder::None).
FrameOutput resolve_output(const OutputSettings& s, const RenderDesc& r, const char* format, bool has_path,
                           int jpeg_quality);

// The region a W x H frame of a scene with render settings r renders on a context with settings s.
struct FrameRegion {
    bool on = false;    // false: the whole frame, and nothing of the region code runs
    bool crop = false;
    RegionRect r;       // clamped to the frame, never empty when on
    // the size of the frame's files and of rr_render_frame_to_memory's image
    int out_w(int W) const { return on && crop ? r.w() : W; }
    int out_h(int H) const { return on && crop ? r.h() : H; }
};
// The scene's border where the context asks for it and the scene has one, else the context's own region,
// clamped. A region that covers the whole frame resolves to off: such a frame is the frame without a region.
// false + err (naming the region and the frame size): nothing of the region lies inside the frame.
bool resolve_region(const OutputSettings& s, const RenderDesc& r, int W, int H, FrameRegion& out, std::string& err);

// One file a frame is asked to write: rr_frame_output with its strings owned.
struct OutputRequest {
    std::string path, format;
    int quality = 0, reduce = 1;
};

// Where an entry of rr_set_extra_outputs writes for a frame submitted with
// `path`: "<path>" at factor 1, "<path>.r<K>" at K > 1 (the extension follows).
std::string extra_output_path(const std::string& path, int reduce);

// Appends what the context and the scene add to a frame's own files, list[0]
// giving the path and the quality: the context's extra outputs; with none of
// those, a scene with render.use_preview whose frame is "OPEN_EXR" adds
// "<path>.jpg", JPEG at factor 1 (Blender's image_settings.use_preview). An
// empty list (a frame without a file) stays empty.
void add_extra_outputs(const OutputSettings& s, const RenderDesc& r, std::vector<OutputRequest>& list);

// What a list of 1 or more files is refused for, before anything is planned:
// RR_OK, or RR_EINVAL (more than RR_MAX_FRAME_OUTPUTS files; no path or format;
// a factor that is not 1, 2, 4 or 8; a JPEG quality outside 1 .. 100; two
// files of one name, which err names) or RR_ENOTSUP (a format nobody writes:
// unsupported_format's text) with err.
int check_outputs(const std::vector<OutputRequest>& list, std::string& err);

// The PNG compression of an image that comes with no scene (the inspection
// entry points): the context's, SCENE meaning legacy.
int png_compression_of(const OutputSettings& s);
// The OpenEXR codec of such an image: the context's, SCENE meaning ZIP.
int exr_codec_of(const OutputSettings& s);
// The dither of such an image: the context's; none where it leaves the
// intensity to a scene.
float dither_of(const OutputSettings& s);

}  // namespace rr
