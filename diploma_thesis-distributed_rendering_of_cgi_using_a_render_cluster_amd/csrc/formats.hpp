// The output formats and their coders, each fact stated once. Everything that
// chooses, names or refuses a file looks here (settings.cpp, coders.cpp, the
// entry points, the shim). Host code only: no HIP header, nothing to link.
#pragma once

#include <cstring>

namespace rr {

// Who codes a frame's output. None: no file. HostRgba: the 8-bit image comes
// back to the host (rr_render_frame_to_memory; a "PNG" file from the host's
// zlib threads where a path is given). The others code on the device, the file
// written from the slot's pinned stream.
enum class Coder { None, HostRgba, Jpeg, Png8, Png16, Exr, Exr32, Tga, Hdr, Iris, Webp };

// Host: no device coder. Jpeg: jpeg.hip. Deflate: the front ends of deflate.hip
// (png.hip, png16.hip, exr.hip). Body: tga.hip, hdr.hip, iris.hip and webp.hip,
// which form a dense body in the slot's scratch and gather it into the stream.
enum class Family { Host, Jpeg, Deflate, Body };

struct CoderInfo {
    Family family;
    bool film;          // reads the float film (W x H float4); else the 8-bit image rgba8
    int depth;          // bits a sample: with 0, the depth rr_debug_encode_device takes for it
    const char* name;   // in messages
    const char* range;  // what an image size outside the coder's range is refused with
};

constexpr CoderInfo kCoders[] = {  // indexed by Coder
    {Family::Host, false, 0, "", ""},
    {Family::Host, false, 8, "PNG", ""},
    {Family::Jpeg, false, 8, "JPEG", "image size outside the JPEG format's range"},
    {Family::Deflate, false, 8, "PNG", "image size outside the device PNG encoder's range"},
    {Family::Deflate, true, 16, "16-bit PNG", "image size outside the device 16-bit PNG encoder's range"},
    {Family::Deflate, true, 16, "EXR", "image size outside the device EXR encoder's range"},  // HALF channels
    {Family::Deflate, true, 32, "32-bit EXR", "image size outside the device 32-bit EXR encoder's range"},  // FLOAT
    {Family::Body, false, 8, "TARGA", "image size outside the TARGA format's range (65535 x 65535, a body below 2 GB)"},
    {Family::Body, true, 32, "HDR", "image size outside the HDR coder's range (a body bound below 2 GB)"},
    {Family::Body, false, 8, "IRIS",
     "image size outside the IRIS format's range (65535 x 65535, a body bound below 2 GB)"},
    {Family::Body, false, 8, "WEBP",
     "image size outside the WEBP format's range (16384 x 16384, a payload bound below 2 GB)"},
};
inline const CoderInfo& coder_info(Coder k) { return kCoders[(int)k]; }

// A format a frame can be submitted with. Its files come from `coder` whatever
// the depth settings say (8 bits a channel; HDR: RGBE quads of the film's
// means), except that "PNG" and "OPEN_EXR" at deep_depth come from `deep`.
// no_alpha: RGBA resolves to RGB, as in Blender. tga_raw: no run-length packets.
struct Format {
    const char* name;
    const char* ext;
    bool no_alpha;
    Coder coder;
    int deep_depth;  // 0: one coder
    Coder deep;
    bool tga_raw;
};

constexpr Format kFormats[] = {  // in the order the refusals list them
    {"JPEG", ".jpg", true, Coder::Jpeg, 0, Coder::None, false},
    {"PNG", ".png", false, Coder::Png8, 16, Coder::Png16, false},  // 8 bits: HostRgba without rr_set_device_png
    {"OPEN_EXR", ".exr", false, Coder::Exr, 32, Coder::Exr32, false},
    {"TARGA", ".tga", false, Coder::Tga, 0, Coder::None, false},
    {"TARGA_RAW", ".tga", false, Coder::Tga, 0, Coder::None, true},
    {"HDR", ".hdr", true, Coder::Hdr, 0, Coder::None, false},
    {"IRIS", ".rgb", false, Coder::Iris, 0, Coder::None, false},
    {"WEBP", ".webp", false, Coder::Webp, 0, Coder::None, false},  // lossless at every quality
};

// The row of a name; nullptr for a name nobody writes, and for NULL.
inline const Format* find_format(const char* name) {
    for (const Format& f : kFormats)
        if (name && std::strcmp(f.name, name) == 0) return &f;
    return nullptr;
}
inline Coder format_coder(const Format& f, int depth) { return f.deep_depth && depth == f.deep_depth ? f.deep : f.coder; }

}  // namespace rr
