// Stand-alone checks of csrc/settings.cpp (no GPU, no HIP): the environment
// spellings, the setters' ranges, the file resolve_output gives a frame, and
// the format table of csrc/formats.hpp with the refusal texts made from it.
// Built with the system compiler and -fsanitize=address,undefined and run as a
// child process by tests/test_settings.py. Exit status 0 and "settings_check:
// ok" when every check holds; every failed check is printed.
//
// The expected values are written out here from the behaviour the C ABI has
// had since each setting was added (rr_set_* and rr_create's RR_* variables,
// rr_frame_submit's choice of coder); none is computed by the code under test.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "looks.hpp"
#include "scene.hpp"
#include "settings.hpp"

using namespace rr;

static int g_failed = 0, g_checked = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        ++g_checked;                                       \
        if (!(cond)) {                                     \
            ++g_failed;                                    \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

static bool same(const OutputSettings& a, const OutputSettings& b) {
    return a.device_png == b.device_png && a.png_depth == b.png_depth && a.exr_depth == b.exr_depth &&
           a.color_mode == b.color_mode && a.look == b.look && a.png_compression == b.png_compression &&
           a.gamma == b.gamma && a.dither == b.dither;
}

// ---- environment text ------------------------------------------------------

struct EnvCase {
    const char* var;
    const char* text;
    bool accepted;
};

// every text the GPU tests give a variable, and the result it has always had
static const EnvCase kEnv[] = {
    {"RR_PNG_DEPTH", "", true},       {"RR_PNG_DEPTH", "0", true},      {"RR_PNG_DEPTH", "8", true},
    {"RR_PNG_DEPTH", "16", true},     {"RR_PNG_DEPTH", "12", false},
    {"RR_EXR_DEPTH", "16", true},     {"RR_EXR_DEPTH", "32", true},     {"RR_EXR_DEPTH", "24", false},
    {"RR_COLOR_MODE", "BW", true},    {"RR_COLOR_MODE", "RGB", true},   {"RR_COLOR_MODE", "RGBA", true},
    {"RR_COLOR_MODE", "", true},      {"RR_COLOR_MODE", "GREY", false},
    {"RR_LOOK", "Very High Contrast", true}, {"RR_LOOK", "Filmic - Low Contrast", true}, {"RR_LOOK", "", true},
    {"RR_LOOK", "Punchy", false},
    {"RR_DISPLAY_GAMMA", "0.7", true}, {"RR_DISPLAY_GAMMA", "", true},  {"RR_DISPLAY_GAMMA", "5", true},
    {"RR_DISPLAY_GAMMA", "7", false},  {"RR_DISPLAY_GAMMA", "two", false}, {"RR_DISPLAY_GAMMA", "-1", false},
    {"RR_DISPLAY_GAMMA", "nan", false},
    {"RR_DITHER", "0.5", true},       {"RR_DITHER", "scene", true},     {"RR_DITHER", "", true},
    {"RR_DITHER", "2", true},         {"RR_DITHER", "2.5", false},      {"RR_DITHER", "-1", false},
    {"RR_DITHER", "x", false},
    {"RR_PNG_COMPRESSION", "15", true},   {"RR_PNG_COMPRESSION", "0", true},    {"RR_PNG_COMPRESSION", "100", true},
    {"RR_PNG_COMPRESSION", "scene", true}, {"RR_PNG_COMPRESSION", "", true},
    {"RR_PNG_COMPRESSION", "101", false}, {"RR_PNG_COMPRESSION", "-3", false},  {"RR_PNG_COMPRESSION", "-1", false},
    {"RR_PNG_COMPRESSION", "fast", false}, {"RR_PNG_COMPRESSION", "15%", false}, {"RR_PNG_COMPRESSION", "1.5", false},
    // spellings of a number that were never a depth
    {"RR_PNG_DEPTH", "016", false},   {"RR_PNG_DEPTH", " 8", false},    {"RR_EXR_DEPTH", "8", false},
    {"RR_EXR_DEPTH", "", true},       {"RR_EXR_DEPTH", "0", true},
    {"RR_DEVICE_PNG", "1", true},     {"RR_DEVICE_PNG", "0", true},     {"RR_DEVICE_PNG", "yes", true},
};

static void check_env() {
    for (const EnvCase& e : kEnv) {
        OutputSettings s, before;
        // start from a changed struct, so that "unchanged" is not "default"
        s.png_depth = 16; s.exr_depth = 32; s.color_mode = RR_COLOR_RGB; s.look = 2; s.png_compression = 40;
        s.gamma = 2.2f; s.dither = 1.0f; s.device_png = true;
        before = s;
        std::string err;
        const bool ok = setting_from_text(s, e.var, e.text, err);
        CHECK(ok == e.accepted, "%s='%s' %s", e.var, e.text, ok ? "accepted" : "refused");
        if (!ok) {
            CHECK(same(s, before), "%s='%s' refused but changed the settings", e.var, e.text);
            CHECK(err.find(e.var) != std::string::npos, "%s='%s': message '%s' lacks the variable", e.var, e.text,
                  err.c_str());
            CHECK(err.find(std::string("'") + e.text + "'") != std::string::npos,
                  "%s='%s': message '%s' does not quote the text", e.var, e.text, err.c_str());
        }
    }
    // the values the accepted texts give
    auto from = [](const char* var, const char* text) {
        OutputSettings s;
        std::string err;
        CHECK(setting_from_text(s, var, text, err), "%s='%s': %s", var, text, err.c_str());
        return s;
    };
    CHECK(from("RR_PNG_DEPTH", "").png_depth == 0 && from("RR_PNG_DEPTH", "0").png_depth == 0, "png depth 0");
    CHECK(from("RR_PNG_DEPTH", "8").png_depth == 8 && from("RR_PNG_DEPTH", "16").png_depth == 16, "png depth");
    CHECK(from("RR_EXR_DEPTH", "16").exr_depth == 16 && from("RR_EXR_DEPTH", "32").exr_depth == 32, "exr depth");
    CHECK(from("RR_COLOR_MODE", "BW").color_mode == RR_COLOR_BW, "BW");
    CHECK(from("RR_COLOR_MODE", "RGB").color_mode == RR_COLOR_RGB, "RGB");
    CHECK(from("RR_COLOR_MODE", "RGBA").color_mode == RR_COLOR_RGBA, "RGBA");
    CHECK(from("RR_COLOR_MODE", "").color_mode == RR_COLOR_SCENE, "colour mode ''");
    CHECK(from("RR_LOOK", "Very High Contrast").look == 1, "look 1");
    CHECK(from("RR_LOOK", "Filmic - Low Contrast").look == 6, "look 6");
    CHECK(from("RR_LOOK", "").look == -1, "look ''");
    CHECK(from("RR_DISPLAY_GAMMA", "0.7").gamma == 0.7f && from("RR_DISPLAY_GAMMA", "5").gamma == 5.0f, "gamma");
    CHECK(from("RR_DISPLAY_GAMMA", "").gamma == 0.0f, "gamma ''");
    CHECK(from("RR_DITHER", "0.5").dither == 0.5f && from("RR_DITHER", "2").dither == 2.0f, "dither");
    CHECK(from("RR_DITHER", "scene").dither == RR_DITHER_SCENE && from("RR_DITHER", "").dither == 0.0f, "dither words");
    CHECK(from("RR_PNG_COMPRESSION", "15").png_compression == 15 && from("RR_PNG_COMPRESSION", "0").png_compression == 0 &&
              from("RR_PNG_COMPRESSION", "100").png_compression == 100,
          "compression");
    CHECK(from("RR_PNG_COMPRESSION", "scene").png_compression == RR_PNG_COMPRESSION_SCENE, "compression scene");
    CHECK(from("RR_PNG_COMPRESSION", "").png_compression == RR_PNG_COMPRESSION_LEGACY, "compression ''");
    CHECK(from("RR_DEVICE_PNG", "1").device_png && !from("RR_DEVICE_PNG", "0").device_png &&
              !from("RR_DEVICE_PNG", "yes").device_png,
          "RR_DEVICE_PNG is == \"1\"");
    // the defaults are rr_create's
    OutputSettings d;
    CHECK(!d.device_png && d.png_depth == 0 && d.exr_depth == 0 && d.color_mode == 0 && d.look == -1 &&
              d.png_compression == RR_PNG_COMPRESSION_LEGACY && d.gamma == 0.f && d.dither == 0.f,
          "defaults");
}

// ---- setters ---------------------------------------------------------------

static void check_setters() {
    std::string err;
    // integers: the accepted set, and for every value the same answer from the variable's text
    for (int v = -40; v <= 140; ++v) {
        const std::string t = std::to_string(v);
        OutputSettings a, b;
        const bool png = v == 0 || v == 8 || v == 16;
        CHECK(set_png_depth(a, v, err) == png, "set_png_depth(%d)", v);
        CHECK(a.png_depth == (png ? v : 0), "set_png_depth(%d) left %d", v, a.png_depth);
        CHECK(setting_from_text(b, "RR_PNG_DEPTH", t.c_str(), err) == png, "RR_PNG_DEPTH=%d", v);
        const bool exr = v == 0 || v == 16 || v == 32;
        CHECK(set_exr_depth(a, v, err) == exr, "set_exr_depth(%d)", v);
        CHECK(a.exr_depth == (exr ? v : 0), "set_exr_depth(%d) left %d", v, a.exr_depth);
        CHECK(setting_from_text(b, "RR_EXR_DEPTH", t.c_str(), err) == exr, "RR_EXR_DEPTH=%d", v);
        const bool mode = v == 0 || v == 1 || v == 3 || v == 4;
        CHECK(set_color_mode(a, v, err) == mode, "set_color_mode(%d)", v);
        CHECK(valid_color_mode(v) == mode, "valid_color_mode(%d)", v);
        // RR_PNG_COMPRESSION_SCENE (-2), LEGACY (-1), 0 .. 100; the variable spells the two constants as words
        const bool comp = v >= -2 && v <= 100;
        OutputSettings c;
        CHECK(set_png_compression(c, v, err) == comp, "set_png_compression(%d)", v);
        CHECK(c.png_compression == (comp ? v : RR_PNG_COMPRESSION_LEGACY), "set_png_compression(%d) left %d", v,
              c.png_compression);
        CHECK(valid_png_compression(v) == comp, "valid_png_compression(%d)", v);
        CHECK(setting_from_text(b, "RR_PNG_COMPRESSION", t.c_str(), err) == (comp && v >= 0), "RR_PNG_COMPRESSION=%d", v);
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    struct F {
        float v;
        bool ok;
    };
    // display gamma: 0 (the scene's) or (0, 5]
    const F gammas[] = {{0.f, true}, {1e-6f, true}, {1.f, true}, {2.2f, true}, {5.f, true},
                        {std::nextafter(5.f, 6.f), false}, {5.5f, false}, {-1.f, false}, {-1e-6f, false},
                        {nan, false}, {inf, false}, {-inf, false}};
    for (const F& g : gammas) {
        OutputSettings a, b;
        a.gamma = 1.5f;
        CHECK(set_display_gamma(a, g.v, err) == g.ok, "set_display_gamma(%g)", g.v);
        CHECK(a.gamma == (g.ok ? g.v : 1.5f), "set_display_gamma(%g) left %g", g.v, a.gamma);
        char t[64];
        std::snprintf(t, sizeof t, "%.9g", g.v);
        CHECK(setting_from_text(b, "RR_DISPLAY_GAMMA", t, err) == g.ok, "RR_DISPLAY_GAMMA=%s", t);
    }
    // dither: [0, 2], or RR_DITHER_SCENE (-1), which the variable spells "scene"
    const F dithers[] = {{0.f, true}, {0.5f, true}, {2.f, true}, {RR_DITHER_SCENE, true},
                         {std::nextafter(2.f, 3.f), false}, {2.5f, false}, {-0.5f, false}, {-2.f, false},
                         {std::nextafter(-1.f, 0.f), false}, {nan, false}, {inf, false}};
    for (const F& d : dithers) {
        OutputSettings a, b;
        a.dither = 1.5f;
        CHECK(set_dither(a, d.v, err) == d.ok, "set_dither(%g)", d.v);
        CHECK(a.dither == (d.ok ? d.v : 1.5f), "set_dither(%g) left %g", d.v, a.dither);
        char t[64];
        std::snprintf(t, sizeof t, "%.9g", d.v);
        CHECK(setting_from_text(b, "RR_DITHER", t, err) == (d.ok && d.v != RR_DITHER_SCENE), "RR_DITHER=%s", t);
    }
    // looks: NULL and "" the scene's; a name with or without Blender's prefix
    OutputSettings l;
    CHECK(set_look(l, "High Contrast", err) && l.look == 2, "look by name");
    CHECK(set_look(l, "Filmic - Very Low Contrast", err) && l.look == 7, "look with prefix");
    CHECK(set_look(l, "None", err) && l.look == 0, "look None");
    for (const char* bad : {"Punchy", "Filmic - ", "high contrast"}) {
        l.look = 3;
        CHECK(!set_look(l, bad, err) && l.look == 3, "set_look('%s')", bad);
        OutputSettings b;
        CHECK(!setting_from_text(b, "RR_LOOK", bad, err), "RR_LOOK='%s'", bad);
    }
    CHECK(set_look(l, nullptr, err) && l.look == -1, "look NULL");
    l.look = 3;
    CHECK(set_look(l, "", err) && l.look == -1, "look ''");
    for (int id = 0; id < kNumLooks; ++id) {
        OutputSettings a, b;
        CHECK(set_look(a, kLooks[id].name, err) && a.look == id, "set_look(%s)", kLooks[id].name);
        CHECK(setting_from_text(b, "RR_LOOK", kLooks[id].name, err) && b.look == id, "RR_LOOK=%s", kLooks[id].name);
    }
    // inspection calls: SCENE compression means legacy, a scene's dither means none
    OutputSettings s;
    s.png_compression = RR_PNG_COMPRESSION_SCENE;
    CHECK(png_compression_of(s) == RR_PNG_COMPRESSION_LEGACY, "png_compression_of(SCENE)");
    s.png_compression = 40;
    CHECK(png_compression_of(s) == 40, "png_compression_of(40)");
    s.dither = RR_DITHER_SCENE;
    CHECK(dither_of(s) == 0.f, "dither_of(SCENE)");
    s.dither = 0.75f;
    CHECK(dither_of(s) == 0.75f, "dither_of(0.75)");
}

// ---- resolve_output --------------------------------------------------------

enum Fmt { NONE, JPEG, PNG, EXR };
static const char* kFmtName[] = {nullptr, "JPEG", "PNG", "OPEN_EXR"};
// a depth "level": 0 none (the context leaves it to the scene), 1 the format's
// low depth (PNG 8, EXR 16), 2 its high one (PNG 16, EXR 32)
static const int kPngDepth[] = {0, 8, 16}, kExrDepth[] = {0, 16, 32};

struct CoderRow {
    Fmt fmt;
    int ctx_level, scene_level;  // scene_level 1 or 2
    bool device_png;
    Coder want;
};
// the context's depth before the scene's; "PNG" at 16 bits is Png16 whatever
// device_png says, at 8 bits HostRgba without device_png; no path, no coder
static const CoderRow kCoder[] = {
    {NONE, 0, 1, false, Coder::None}, {NONE, 0, 1, true, Coder::None}, {NONE, 0, 2, false, Coder::None},
    {NONE, 0, 2, true, Coder::None},  {NONE, 1, 1, false, Coder::None}, {NONE, 1, 1, true, Coder::None},
    {NONE, 1, 2, false, Coder::None}, {NONE, 1, 2, true, Coder::None}, {NONE, 2, 1, false, Coder::None},
    {NONE, 2, 1, true, Coder::None},  {NONE, 2, 2, false, Coder::None}, {NONE, 2, 2, true, Coder::None},
    {JPEG, 0, 1, false, Coder::Jpeg}, {JPEG, 0, 1, true, Coder::Jpeg}, {JPEG, 0, 2, false, Coder::Jpeg},
    {JPEG, 0, 2, true, Coder::Jpeg},  {JPEG, 1, 1, false, Coder::Jpeg}, {JPEG, 1, 1, true, Coder::Jpeg},
    {JPEG, 1, 2, false, Coder::Jpeg}, {JPEG, 1, 2, true, Coder::Jpeg}, {JPEG, 2, 1, false, Coder::Jpeg},
    {JPEG, 2, 1, true, Coder::Jpeg},  {JPEG, 2, 2, false, Coder::Jpeg}, {JPEG, 2, 2, true, Coder::Jpeg},
    {PNG, 0, 1, false, Coder::HostRgba}, {PNG, 0, 1, true, Coder::Png8},
    {PNG, 0, 2, false, Coder::Png16},    {PNG, 0, 2, true, Coder::Png16},
    {PNG, 1, 1, false, Coder::HostRgba}, {PNG, 1, 1, true, Coder::Png8},
    {PNG, 1, 2, false, Coder::HostRgba}, {PNG, 1, 2, true, Coder::Png8},
    {PNG, 2, 1, false, Coder::Png16},    {PNG, 2, 1, true, Coder::Png16},
    {PNG, 2, 2, false, Coder::Png16},    {PNG, 2, 2, true, Coder::Png16},
    {EXR, 0, 1, false, Coder::Exr},   {EXR, 0, 1, true, Coder::Exr},
    {EXR, 0, 2, false, Coder::Exr32}, {EXR, 0, 2, true, Coder::Exr32},
    {EXR, 1, 1, false, Coder::Exr},   {EXR, 1, 1, true, Coder::Exr},
    {EXR, 1, 2, false, Coder::Exr},   {EXR, 1, 2, true, Coder::Exr},
    {EXR, 2, 1, false, Coder::Exr32}, {EXR, 2, 1, true, Coder::Exr32},
    {EXR, 2, 2, false, Coder::Exr32}, {EXR, 2, 2, true, Coder::Exr32},
};

struct ModeRow {
    bool jpeg;
    int ctx_mode, scene_mode, want;
};
// the context's mode, at 0 the scene's, at 0 again the format's own layout
// (JPEG three components, the others four); JPEG has no alpha: RGBA gives RGB
static const ModeRow kMode[] = {
    {false, 0, 0, 4}, {false, 0, 1, 1}, {false, 0, 3, 3}, {false, 0, 4, 4},
    {false, 1, 0, 1}, {false, 1, 1, 1}, {false, 1, 3, 1}, {false, 1, 4, 1},
    {false, 3, 0, 3}, {false, 3, 1, 3}, {false, 3, 3, 3}, {false, 3, 4, 3},
    {false, 4, 0, 4}, {false, 4, 1, 4}, {false, 4, 3, 4}, {false, 4, 4, 4},
    {true, 0, 0, 3},  {true, 0, 1, 1},  {true, 0, 3, 3},  {true, 0, 4, 3},
    {true, 1, 0, 1},  {true, 1, 1, 1},  {true, 1, 3, 1},  {true, 1, 4, 1},
    {true, 3, 0, 3},  {true, 3, 1, 3},  {true, 3, 3, 3},  {true, 3, 4, 3},
    {true, 4, 0, 3},  {true, 4, 1, 3},  {true, 4, 3, 3},  {true, 4, 4, 3},
};

struct CompRow {
    int ctx_comp, scene_comp, want;
};
// the context's setting, at SCENE the scene's, which is -1 (legacy) where the scene has no field
static const CompRow kComp[] = {
    {RR_PNG_COMPRESSION_LEGACY, -1, RR_PNG_COMPRESSION_LEGACY}, {RR_PNG_COMPRESSION_LEGACY, 40, RR_PNG_COMPRESSION_LEGACY},
    {RR_PNG_COMPRESSION_SCENE, -1, RR_PNG_COMPRESSION_LEGACY},  {RR_PNG_COMPRESSION_SCENE, 40, 40},
    {15, -1, 15},                                                {15, 40, 15},
};

static void check_resolve_output() {
    int combos = 0;
    for (const CoderRow& k : kCoder)
        for (const ModeRow& m : kMode) {
            if (m.jpeg != (k.fmt == JPEG)) continue;
            for (const CompRow& p : kComp) {
                OutputSettings s;
                s.device_png = k.device_png;
                s.png_depth = kPngDepth[k.ctx_level];
                s.exr_depth = kExrDepth[k.ctx_level];
                s.color_mode = m.ctx_mode;
                s.png_compression = p.ctx_comp;
                RenderDesc r;
                r.color_depth = kPngDepth[k.scene_level];
                r.exr_depth = kExrDepth[k.scene_level];
                r.color_mode = m.scene_mode;
                r.png_compression = p.scene_comp;
                const FrameOutput o = resolve_output(s, r, kFmtName[k.fmt], k.fmt != NONE, 77);
                ++combos;
                CHECK(o.coder == k.want, "coder %d, want %d: format %d depth %d/%d device_png %d", (int)o.coder,
                      (int)k.want, (int)k.fmt, k.ctx_level, k.scene_level, (int)k.device_png);
                CHECK(o.color_mode == m.want, "colour mode %d, want %d: format %d modes %d/%d", o.color_mode, m.want,
                      (int)k.fmt, m.ctx_mode, m.scene_mode);
                CHECK(o.png_compression == p.want, "compression %d, want %d: %d/%d", o.png_compression, p.want,
                      p.ctx_comp, p.scene_comp);
                CHECK(o.quality == 77, "quality %d", o.quality);
            }
        }
    // 4 formats x 3 context depths x 2 scene depths x 2 device_png x 16 colour modes x 6 compressions
    CHECK(combos == 4 * 3 * 2 * 2 * 16 * 6, "%d combinations", combos);
    // a format given without a path is still no file
    OutputSettings s;
    RenderDesc r;
    CHECK(resolve_output(s, r, "JPEG", false, 90).coder == Coder::None, "no path, no coder");
    CHECK(resolve_output(s, r, "JPEG", false, 90).color_mode == RR_COLOR_RGBA, "no path: not a JPEG's layout");
    CHECK(std::strcmp(coder_ext(Coder::Jpeg), ".jpg") == 0 && std::strcmp(coder_ext(Coder::Exr), ".exr") == 0 &&
              std::strcmp(coder_ext(Coder::Exr32), ".exr") == 0 && std::strcmp(coder_ext(Coder::Png8), ".png") == 0 &&
              std::strcmp(coder_ext(Coder::Png16), ".png") == 0 && std::strcmp(coder_ext(Coder::HostRgba), ".png") == 0,
          "extensions");
}

// ---- the format table (formats.hpp) ----------------------------------------

static const Coder J = Coder::Jpeg, HOST = Coder::HostRgba, P8 = Coder::Png8, P16 = Coder::Png16, X16 = Coder::Exr,
                   X32 = Coder::Exr32, TG = Coder::Tga, HD = Coder::Hdr, IR = Coder::Iris, WP = Coder::Webp;

struct FormatRow {
    const char* name;
    const char* ext;
    bool no_alpha, tga_raw;
    // the coder of a frame with a path, by the depth levels above: [context level 0, 1, 2][scene level 1, 2]
    // [device_png off, on]
    Coder at[3][2][2];
};
// what a frame of each name has been written as since the format was added
static const FormatRow kFormatRows[] = {
    {"JPEG", ".jpg", true, false, {{{J, J}, {J, J}}, {{J, J}, {J, J}}, {{J, J}, {J, J}}}},
    {"PNG", ".png", false, false,
     {{{HOST, P8}, {P16, P16}}, {{HOST, P8}, {HOST, P8}}, {{P16, P16}, {P16, P16}}}},
    {"OPEN_EXR", ".exr", false, false,
     {{{X16, X16}, {X32, X32}}, {{X16, X16}, {X16, X16}}, {{X32, X32}, {X32, X32}}}},
    {"TARGA", ".tga", false, false, {{{TG, TG}, {TG, TG}}, {{TG, TG}, {TG, TG}}, {{TG, TG}, {TG, TG}}}},
    {"TARGA_RAW", ".tga", false, true, {{{TG, TG}, {TG, TG}}, {{TG, TG}, {TG, TG}}, {{TG, TG}, {TG, TG}}}},
    {"HDR", ".hdr", true, false, {{{HD, HD}, {HD, HD}}, {{HD, HD}, {HD, HD}}, {{HD, HD}, {HD, HD}}}},
    {"IRIS", ".rgb", false, false, {{{IR, IR}, {IR, IR}}, {{IR, IR}, {IR, IR}}, {{IR, IR}, {IR, IR}}}},
    {"WEBP", ".webp", false, false, {{{WP, WP}, {WP, WP}}, {{WP, WP}, {WP, WP}}, {{WP, WP}, {WP, WP}}}},
};

struct CoderRowFacts {
    Coder k;
    Family family;
    bool film;  // reads the float film, else the 8-bit image
    const char* ext;
    const char* range;
};
static const CoderRowFacts kCoderFacts[] = {
    {Coder::None, Family::Host, false, "", ""},
    {Coder::HostRgba, Family::Host, false, ".png", ""},
    {Coder::Jpeg, Family::Jpeg, false, ".jpg", "image size outside the JPEG format's range"},
    {Coder::Png8, Family::Deflate, false, ".png", "image size outside the device PNG encoder's range"},
    {Coder::Png16, Family::Deflate, true, ".png", "image size outside the device 16-bit PNG encoder's range"},
    {Coder::Exr, Family::Deflate, true, ".exr", "image size outside the device EXR encoder's range"},
    {Coder::Exr32, Family::Deflate, true, ".exr", "image size outside the device 32-bit EXR encoder's range"},
    {Coder::Tga, Family::Body, false, ".tga",
     "image size outside the TARGA format's range (65535 x 65535, a body below 2 GB)"},
    {Coder::Hdr, Family::Body, true, ".hdr", "image size outside the HDR coder's range (a body bound below 2 GB)"},
    {Coder::Iris, Family::Body, false, ".rgb",
     "image size outside the IRIS format's range (65535 x 65535, a body bound below 2 GB)"},
    {Coder::Webp, Family::Body, false, ".webp",
     "image size outside the WEBP format's range (16384 x 16384, a payload bound below 2 GB)"},
};

static void check_formats() {
    CHECK(sizeof kFormats / sizeof kFormats[0] == 8, "eight formats");
    size_t row = 0;
    for (const FormatRow& w : kFormatRows) {
        const Format* f = find_format(w.name);
        CHECK(f && known_format(w.name), "%s is a format", w.name);
        if (!f) continue;
        CHECK(f == &kFormats[row++], "%s: the table's order is the refusals'", w.name);
        CHECK(std::strcmp(f->ext, w.ext) == 0, "%s: extension %s, want %s", w.name, f->ext, w.ext);
        CHECK(f->no_alpha == w.no_alpha, "%s: no_alpha %d", w.name, (int)f->no_alpha);
        CHECK(f->tga_raw == w.tga_raw, "%s: tga_raw %d", w.name, (int)f->tga_raw);
        for (int ctx = 0; ctx < 3; ++ctx)
            for (int scene = 1; scene <= 2; ++scene)
                for (int dev = 0; dev < 2; ++dev) {
                    OutputSettings s;
                    s.device_png = dev != 0;
                    s.png_depth = kPngDepth[ctx];
                    s.exr_depth = kExrDepth[ctx];
                    RenderDesc r;
                    r.color_depth = kPngDepth[scene];
                    r.exr_depth = kExrDepth[scene];
                    const FrameOutput o = resolve_output(s, r, w.name, true, 90);
                    const Coder want = w.at[ctx][scene - 1][dev];
                    CHECK(o.coder == want, "%s depth %d/%d device_png %d: coder %d, want %d", w.name, ctx, scene, dev,
                          (int)o.coder, (int)want);
                    CHECK(o.tga_raw == w.tga_raw, "%s: the frame's tga_raw %d", w.name, (int)o.tga_raw);
                    // no setting: the format's own layout; RGBA asked of a format without alpha is RGB
                    CHECK(o.color_mode == (w.no_alpha ? RR_COLOR_RGB : RR_COLOR_RGBA), "%s: layout %d", w.name,
                          o.color_mode);
                    s.color_mode = RR_COLOR_RGBA;
                    CHECK(resolve_output(s, r, w.name, true, 90).color_mode == (w.no_alpha ? RR_COLOR_RGB : RR_COLOR_RGBA),
                          "%s: RGBA", w.name);
                    CHECK(resolve_output(s, r, w.name, false, 90).coder == Coder::None, "%s: no path, no coder", w.name);
                }
    }
    for (const char* bad : {"TIFF", "BMP", "jpeg", "PNG ", "", "TARGA_"})
        CHECK(!known_format(bad) && !find_format(bad), "'%s' is no format", bad);
    CHECK(!known_format(nullptr), "NULL is no format");

    CHECK(sizeof kCoders / sizeof kCoders[0] == 11, "a row for every Coder");
    for (const CoderRowFacts& w : kCoderFacts) {
        const CoderInfo& ci = coder_info(w.k);
        CHECK(ci.family == w.family, "coder %d: family %d", (int)w.k, (int)ci.family);
        CHECK(ci.film == w.film, "coder %d: film %d", (int)w.k, (int)ci.film);
        CHECK(std::strcmp(coder_ext(w.k), w.ext) == 0, "coder %d: extension %s", (int)w.k, coder_ext(w.k));
        CHECK(std::strcmp(ci.range, w.range) == 0, "coder %d: range refusal '%s'", (int)w.k, ci.range);
        CHECK(device_deflate(w.k) == (w.family == Family::Deflate) && device_body(w.k) == (w.family == Family::Body) &&
                  slot_coder(w.k) == (w.family == Family::Deflate || w.family == Family::Body),
              "coder %d: the family predicates", (int)w.k);
    }
    // the depth rr_debug_encode_device takes for a coder besides 0, and the names its messages use
    CHECK(coder_info(J).depth == 8 && coder_info(P8).depth == 8 && coder_info(TG).depth == 8 &&
              coder_info(IR).depth == 8 && coder_info(WP).depth == 8 && coder_info(P16).depth == 16 &&
              coder_info(X16).depth == 16 && coder_info(X32).depth == 32 && coder_info(HD).depth == 32,
          "coder depths");
    CHECK(std::string(coder_info(J).name) == "JPEG" && std::string(coder_info(TG).name) == "TARGA" &&
              std::string(coder_info(HD).name) == "HDR" && std::string(coder_info(IR).name) == "IRIS" &&
              std::string(coder_info(WP).name) == "WEBP",
          "coder names");

    // the refusals that list the formats, as rr_frame_submit and the host coders have worded them
    CHECK(unsupported_format("TIFF") ==
              "unsupported output format 'TIFF' (JPEG, PNG, OPEN_EXR, TARGA, TARGA_RAW, HDR, IRIS and WEBP are supported)",
          "'%s'", unsupported_format("TIFF").c_str());
    CHECK(unsupported_format("HDR", true) ==
              "unsupported output format 'HDR' for an RGBA8 image: it needs the float film (JPEG, PNG, TARGA, "
              "TARGA_RAW, IRIS and WEBP are supported here)",
          "'%s'", unsupported_format("HDR", true).c_str());
    CHECK(unsupported_format("OPEN_EXR", true) ==
              "unsupported output format 'OPEN_EXR' for an RGBA8 image: it needs the float film (JPEG, PNG, TARGA, "
              "TARGA_RAW, IRIS and WEBP are supported here)",
          "'%s'", unsupported_format("OPEN_EXR", true).c_str());
    CHECK(unsupported_format("TIFF", true) ==
              "unsupported output format 'TIFF' (JPEG, PNG, TARGA, TARGA_RAW, IRIS and WEBP are supported here; "
              "OPEN_EXR and HDR need the float film)",
          "'%s'", unsupported_format("TIFF", true).c_str());
}

// `settings_check --formats`: the table's "name extension" lines, for tests/test_settings.py to hold the
// package's Python copy (naming.py EXTENSIONS) to.
int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--formats") == 0) {
        for (const Format& f : kFormats) std::printf("%s %s\n", f.name, f.ext);
        return 0;
    }
    check_env();
    check_setters();
    check_resolve_output();
    check_formats();
    if (g_failed) {
        std::printf("settings_check: %d of %d checks FAILED\n", g_failed, g_checked);
        return 1;
    }
    std::printf("settings_check: ok (%d checks)\n", g_checked);
    return 0;
}
