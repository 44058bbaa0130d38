// The OpenEXR codec setting without a GPU: links csrc/settings.cpp alone (host
// code, no HIP header). Checks every spelling of RR_EXR_CODEC, the setter's
// range, resolve_output's precedence (context over scene over ZIP), which
// codecs fall back to ZIP and what they are flagged with, and the host side of
// the rule headers exr_rle_rule.h and pxr24_rule.h. Built with the system C++
// compiler under AddressSanitizer and UBSan by tests/test_exr_codec_format.py;
// exits 0 when everything holds.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "exr_rle_rule.h"
#include "pxr24_rule.h"
#include "scene.hpp"
#include "settings.hpp"

using namespace rr;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

int main() {
    const char* const names[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};
    const int values[] = {RR_EXR_CODEC_NONE, RR_EXR_CODEC_RLE,  RR_EXR_CODEC_ZIPS, RR_EXR_CODEC_ZIP,  RR_EXR_CODEC_PIZ,
                          RR_EXR_CODEC_PXR24, RR_EXR_CODEC_B44, RR_EXR_CODEC_B44A, RR_EXR_CODEC_DWAA, RR_EXR_CODEC_DWAB};
    std::string err;
    // the constants are the ABI's
    CHECK(RR_EXR_CODEC_SCENE == 0 && RR_EXR_CODEC_NONE == 1 && RR_EXR_CODEC_DWAB == 10);
    // every good spelling, and the names both ways
    for (int k = 0; k < 10; ++k) {
        OutputSettings s;
        CHECK(s.exr_codec == RR_EXR_CODEC_SCENE);
        CHECK(setting_from_text(s, "RR_EXR_CODEC", names[k], err));
        CHECK(s.exr_codec == values[k]);
        CHECK(std::string(exr_codec_name(values[k])) == names[k]);
        CHECK(exr_codec_of_name(names[k]) == values[k]);
    }
    {  // empty: the scene's, also after another value
        OutputSettings s;
        CHECK(setting_from_text(s, "RR_EXR_CODEC", "RLE", err));
        CHECK(setting_from_text(s, "RR_EXR_CODEC", "", err));
        CHECK(s.exr_codec == RR_EXR_CODEC_SCENE);
    }
    // bad spellings change nothing and name the variable and the text
    for (const char* bad : {"none", "Zip", "zip", " ZIP", "ZIP ", "4", "0", "SCENE", "scene", "PXR", "PXR24 ", "DWA",
                            "B44B", "ZIP16", "-1"}) {
        OutputSettings s;
        s.exr_codec = RR_EXR_CODEC_PIZ;
        err.clear();
        CHECK(!setting_from_text(s, "RR_EXR_CODEC", bad, err));
        CHECK(s.exr_codec == RR_EXR_CODEC_PIZ);
        CHECK(err.find("RR_EXR_CODEC") != std::string::npos && err.find(std::string("'") + bad + "'") != std::string::npos);
    }
    {  // the environment
        OutputSettings s;
        setenv("RR_EXR_CODEC", "PXR24", 1);
        CHECK(settings_from_env(s, err) && s.exr_codec == RR_EXR_CODEC_PXR24);
        setenv("RR_EXR_CODEC", "pxr24", 1);
        OutputSettings t;
        CHECK(!settings_from_env(t, err) && t.exr_codec == RR_EXR_CODEC_SCENE);
        unsetenv("RR_EXR_CODEC");
    }
    {  // the setter's range
        OutputSettings s;
        for (int v = -3; v <= 99; ++v) {
            const bool ok = v >= RR_EXR_CODEC_SCENE && v <= RR_EXR_CODEC_DWAB;
            CHECK(set_exr_codec(s, v, err) == ok);
            if (ok) CHECK(s.exr_codec == v);
        }
        CHECK(exr_codec_name(0)[0] == 0 && exr_codec_name(11)[0] == 0 && exr_codec_name(-1)[0] == 0);
        CHECK(exr_codec_of_name("") == -1 && exr_codec_of_name("TIFF") == -1);
    }
    // resolve_output: the context's, else the scene's, else ZIP; at both depths
    for (int depth : {16, 32}) {
        RenderDesc r;
        r.exr_depth = depth;
        OutputSettings s;
        FrameOutput o = resolve_output(s, r, "OPEN_EXR", true, 90);
        CHECK(o.coder == (depth == 32 ? Coder::Exr32 : Coder::Exr));
        CHECK(o.exr_codec == RR_EXR_CODEC_ZIP && exr_codec_written(o) == RR_EXR_CODEC_ZIP && exr_codec_warning(o).empty());
        r.exr_codec = RR_EXR_CODEC_RLE;
        o = resolve_output(s, r, "OPEN_EXR", true, 90);
        CHECK(o.exr_codec == RR_EXR_CODEC_RLE && exr_codec_written(o) == RR_EXR_CODEC_RLE);
        CHECK(set_exr_codec(s, RR_EXR_CODEC_NONE, err));
        o = resolve_output(s, r, "OPEN_EXR", true, 90);
        CHECK(o.exr_codec == RR_EXR_CODEC_NONE && exr_codec_warning(o).empty());
        CHECK(set_exr_codec(s, RR_EXR_CODEC_ZIP, err));  // ZIP on the context beats the scene's RLE
        o = resolve_output(s, r, "OPEN_EXR", true, 90);
        CHECK(o.exr_codec == RR_EXR_CODEC_ZIP);
        CHECK(set_exr_codec(s, RR_EXR_CODEC_SCENE, err));
        o = resolve_output(s, r, "OPEN_EXR", true, 90);
        CHECK(o.exr_codec == RR_EXR_CODEC_RLE);
    }
    // the codecs not built are written as ZIP and flagged by name; never for another format
    for (int k = 0; k < 10; ++k) {
        RenderDesc r;
        OutputSettings s;
        CHECK(set_exr_codec(s, values[k], err));
        const FrameOutput o = resolve_output(s, r, "OPEN_EXR", true, 90);
        const bool built = values[k] == RR_EXR_CODEC_NONE || values[k] == RR_EXR_CODEC_RLE ||
                           values[k] == RR_EXR_CODEC_ZIP || values[k] == RR_EXR_CODEC_PXR24;
        CHECK(exr_codec_built(values[k]) == built);
        CHECK(exr_codec_written(o) == (built ? values[k] : RR_EXR_CODEC_ZIP));
        const std::string w = exr_codec_warning(o);
        CHECK(w.empty() == built);
        if (!built) CHECK(w.find(std::string("codec ") + names[k] + ":") != std::string::npos && w.find("ZIP") != std::string::npos);
        const FrameOutput j = resolve_output(s, r, "JPEG", true, 90);
        CHECK(exr_codec_warning(j).empty());
    }
    // the RLE packets' header bytes and bound
    CHECK(ExrRle::header(true, 1) == 0 && ExrRle::header(true, 128) == 127);
    CHECK(ExrRle::header(false, 1) == 255 && ExrRle::header(false, 127) == 129);
    CHECK(exr_rle_row_max_bytes(127) == 128 && exr_rle_row_max_bytes(128) == 130 && exr_rle_row_max_bytes(1) == 2);
    // the 24-bit rule at its edges
    CHECK(float24_bits(0x00000000u) == 0x000000u && float24_bits(0x80000000u) == 0x800000u);
    CHECK(float24_bits(0x3F800000u) == 0x3F8000u);
    CHECK(float24_bits(0x3F80007Fu) == 0x3F8000u && float24_bits(0x3F800080u) == 0x3F8001u &&
          float24_bits(0x3F800081u) == 0x3F8001u);
    CHECK(float24_bits(0x7F7FFFFFu) == 0x7F7FFFu);  // the largest finite float truncates
    CHECK(float24_bits(0xFF7FFFFFu) == 0xFF7FFFu);
    CHECK(float24_bits(0x7F800000u) == 0x7F8000u && float24_bits(0xFF800000u) == 0xFF8000u);
    CHECK(float24_bits(0x7F800001u) == 0x7F8001u);  // a NaN with payload in the low byte stays a NaN
    CHECK(float24_bits(0x7FC00000u) == 0x7FC000u);
    CHECK(float24_bits(0x00000001u) == 0x000000u && float24_bits(0x00000080u) == 0x000001u);
    if (g_failed) {
        std::printf("exr_codec_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("exr_codec_check: ok\n");
    return 0;
}
