// Several files from one frame, without a GPU: links csrc/settings.cpp alone
// (host code, no HIP header). Checks every spelling of RR_EXTRA_OUTPUTS, the
// paths its entries derive, what a context and a scene add to a frame's own
// file, the list's refusals (count, factor, format, JPEG quality, collisions),
// that every output resolves on its own, and the host side of reduce_rule.h on
// hand-worked blocks. Built with the system C++ compiler under AddressSanitizer
// and UBSan by tests/test_multi_output_format.py; exits 0 when everything holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "reduce_rule.h"
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

struct Px {
    float x, y, z, w;
};

static bool has(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

int main() {
    std::string err;
    CHECK(RR_MAX_FRAME_OUTPUTS == 4 && RR_ABI_VERSION == 8);
    {  // good specs
        OutputSettings s;
        CHECK(s.extra_outputs.empty());
        CHECK(setting_from_text(s, "RR_EXTRA_OUTPUTS", "JPEG:4,PNG", err));
        CHECK(s.extra_outputs.size() == 2);
        CHECK(std::string(s.extra_outputs[0].format->name) == "JPEG" && s.extra_outputs[0].reduce == 4);
        CHECK(std::string(s.extra_outputs[1].format->name) == "PNG" && s.extra_outputs[1].reduce == 1);
        CHECK(set_extra_outputs(s, "OPEN_EXR:1,WEBP:8,TARGA_RAW:2", err) && s.extra_outputs.size() == 3);
        CHECK(s.extra_outputs[2].format->tga_raw && s.extra_outputs[2].reduce == 2);
        CHECK(set_extra_outputs(s, "JPEG:2,JPEG:4,JPEG", err) && s.extra_outputs.size() == 3);  // three files
        CHECK(set_extra_outputs(s, "", err) && s.extra_outputs.empty());
        CHECK(set_extra_outputs(s, "HDR:8", err) && s.extra_outputs.size() == 1);
        CHECK(set_extra_outputs(s, nullptr, err) && s.extra_outputs.empty());
    }
    // bad specs change nothing and name the variable and the text
    for (const char* bad : {"jpeg", "JPEG:3", "JPEG:0", "JPEG:16", "JPEG:", "JPEG:2:2", "JPEG,", ",JPEG", "JPEG,,PNG",
                            " JPEG", "JPEG :2", "JPEG: 2", "JPEG:02", "TIFF", "JPEG:2,TIFF:2", "JPEG:2,JPEG:2",
                            "TARGA,TARGA_RAW", "JPEG,PNG,HDR,WEBP", ":", "JPEG:-2", "JPEG:2.0"}) {
        OutputSettings s;
        CHECK(set_extra_outputs(s, "HDR:8", err));
        err.clear();
        CHECK(!setting_from_text(s, "RR_EXTRA_OUTPUTS", bad, err));
        CHECK(s.extra_outputs.size() == 1 && s.extra_outputs[0].reduce == 8);
        CHECK(has(err, "RR_EXTRA_OUTPUTS") && has(err, std::string("'") + bad + "'"));
    }
    {  // a format nobody writes: the text a frame's refusal has; a collision names both
        OutputSettings s;
        CHECK(!set_extra_outputs(s, "TIFF:2", err) && has(err, unsupported_format("TIFF")));
        CHECK(!set_extra_outputs(s, "TARGA,TARGA_RAW", err) && has(err, "same file") && has(err, "TARGA"));
        CHECK(!set_extra_outputs(s, "JPEG,PNG,HDR,WEBP", err) && has(err, "at most 3"));
    }
    {  // the environment
        OutputSettings s;
        setenv("RR_EXTRA_OUTPUTS", "JPEG:2", 1);
        CHECK(settings_from_env(s, err) && s.extra_outputs.size() == 1 && s.extra_outputs[0].reduce == 2);
        setenv("RR_EXTRA_OUTPUTS", "JPEG:5", 1);
        OutputSettings t;
        err.clear();
        CHECK(!settings_from_env(t, err) && t.extra_outputs.empty());
        CHECK(has(err, "RR_EXTRA_OUTPUTS='JPEG:5'"));
        setenv("RR_EXTRA_OUTPUTS", "", 1);
        CHECK(settings_from_env(s, err) && s.extra_outputs.empty());
        unsetenv("RR_EXTRA_OUTPUTS");
    }
    // derived paths
    CHECK(extra_output_path("/o/f0001", 1) == "/o/f0001");
    CHECK(extra_output_path("/o/f0001", 2) == "/o/f0001.r2");
    CHECK(extra_output_path("/o/f0001", 4) == "/o/f0001.r4");
    CHECK(extra_output_path("f", 8) == "f.r8");
    {  // what a context adds: behind the frame's own, its path and quality
        OutputSettings s;
        RenderDesc r;
        CHECK(set_extra_outputs(s, "JPEG:4,PNG", err));
        std::vector<OutputRequest> list = {{"/o/f", "OPEN_EXR", 77, 1}};
        add_extra_outputs(s, r, list);
        CHECK(list.size() == 3);
        CHECK(list[1].path == "/o/f.r4" && list[1].format == "JPEG" && list[1].quality == 77 && list[1].reduce == 4);
        CHECK(list[2].path == "/o/f" && list[2].format == "PNG" && list[2].quality == 77 && list[2].reduce == 1);
        CHECK(check_outputs(list, err) == RR_OK);
        std::vector<OutputRequest> none;  // a frame without a file stays without
        add_extra_outputs(s, r, none);
        CHECK(none.empty());
        // a collision with the frame's own file
        std::vector<OutputRequest> own = {{"/o/f", "PNG", 90, 1}};
        add_extra_outputs(s, r, own);
        CHECK(check_outputs(own, err) == RR_EINVAL && has(err, "/o/f.png"));
        // the count includes what is added
        std::vector<OutputRequest> three = {{"a", "JPEG", 90, 1}, {"b", "JPEG", 90, 1}, {"c", "JPEG", 90, 1}};
        add_extra_outputs(s, r, three);
        CHECK(three.size() == 5 && check_outputs(three, err) == RR_EINVAL && has(err, "1 .. 4"));
    }
    {  // render.use_preview: OPEN_EXR frames only, and only without extra outputs of the context
        OutputSettings s;
        RenderDesc r;
        CHECK(!r.use_preview);
        std::vector<OutputRequest> a = {{"/o/f", "OPEN_EXR", 80, 1}};
        add_extra_outputs(s, r, a);
        CHECK(a.size() == 1);
        r.use_preview = true;
        add_extra_outputs(s, r, a);
        CHECK(a.size() == 2 && a[1].path == "/o/f" && a[1].format == "JPEG" && a[1].quality == 80 && a[1].reduce == 1);
        CHECK(check_outputs(a, err) == RR_OK);
        std::vector<OutputRequest> b = {{"/o/f", "PNG", 80, 1}};
        add_extra_outputs(s, r, b);
        CHECK(b.size() == 1);
        CHECK(set_extra_outputs(s, "WEBP:2", err));
        std::vector<OutputRequest> c = {{"/o/f", "OPEN_EXR", 80, 1}};
        add_extra_outputs(s, r, c);
        CHECK(c.size() == 2 && c[1].format == "WEBP");
        // each output resolves on its own: the preview has three components beside the master's four
        const FrameOutput exr = resolve_output(OutputSettings{}, r, "OPEN_EXR", true, 80);
        const FrameOutput jpg = resolve_output(OutputSettings{}, r, "JPEG", true, 80);
        CHECK(exr.coder == Coder::Exr && exr.color_mode == RR_COLOR_RGBA);
        CHECK(jpg.coder == Coder::Jpeg && jpg.color_mode == RR_COLOR_RGB && jpg.quality == 80);
        OutputSettings deep;
        CHECK(set_exr_depth(deep, 32, err) && set_png_depth(deep, 16, err));
        CHECK(resolve_output(deep, r, "OPEN_EXR", true, 80).coder == Coder::Exr32);
        CHECK(resolve_output(deep, r, "PNG", true, 80).coder == Coder::Png16);
        CHECK(resolve_output(deep, r, "JPEG", true, 80).coder == Coder::Jpeg);
    }
    {  // the list's refusals
        auto one = [](const char* p, const char* f, int q, int k) { return OutputRequest{p, f, q, k}; };
        std::vector<OutputRequest> l;
        CHECK(check_outputs(l, err) == RR_EINVAL && has(err, "1 .. 4"));
        for (int k : {1, 2, 4, 8}) {
            l = {one("a", "JPEG", 90, k)};
            CHECK(check_outputs(l, err) == RR_OK);
        }
        for (int k : {0, -1, 3, 5, 6, 7, 9, 16, 1 << 30}) {
            l = {one("a", "JPEG", 90, k)};
            CHECK(check_outputs(l, err) == RR_EINVAL && has(err, "1, 2, 4 or 8"));
        }
        l = {one("a", "JPEG", 90, 1), one("a", "TIFF", 90, 1)};
        CHECK(check_outputs(l, err) == RR_ENOTSUP && err == unsupported_format("TIFF"));
        l = {one("a", "PNG", 0, 1), one("b", "JPEG", 0, 2)};
        CHECK(check_outputs(l, err) == RR_EINVAL && has(err, "jpeg_quality"));
        l = {one("a", "PNG", 0, 1), one("b", "WEBP", 0, 2)};  // a quality only JPEG reads
        CHECK(check_outputs(l, err) == RR_OK);
        l = {one("a", "JPEG", 90, 1), one("a", "JPEG", 50, 2)};  // one name whatever the factor
        CHECK(check_outputs(l, err) == RR_EINVAL && has(err, "a.jpg"));
        l = {one("a", "TARGA", 90, 1), one("b", "PNG", 90, 1), one("a", "TARGA_RAW", 90, 1)};
        CHECK(check_outputs(l, err) == RR_EINVAL && has(err, "a.tga"));
        l = {one("a", "JPEG", 90, 1), one("a.r2", "JPEG", 90, 2), one("a", "PNG", 90, 1), one("b", "JPEG", 90, 1)};
        CHECK(check_outputs(l, err) == RR_OK);
        l.push_back(one("c", "JPEG", 90, 1));
        CHECK(check_outputs(l, err) == RR_EINVAL);
    }
    {  // reduce_rule.h on the host: sizes, full and partial blocks, the order of the sum
        CHECK(reduced_size(1, 8) == 1 && reduced_size(8, 8) == 1 && reduced_size(9, 8) == 2 && reduced_size(67, 4) == 17 &&
              reduced_size(45, 4) == 12 && reduced_size(5, 1) == 5);
        CHECK(reduce_factor_valid(1) && reduce_factor_valid(8) && !reduce_factor_valid(3) && !reduce_factor_valid(0) &&
              !reduce_factor_valid(16));
        const int W = 3, H = 3;
        std::vector<Px> img((size_t)W * H);
        for (int i = 0; i < W * H; ++i) img[i] = {(float)(i + 1), -(float)(i + 1), 0.5f, 1.0f};
        const Px a = reduce_block(img.data(), W, H, 2, 0, 0);  // 1 2 / 4 5
        CHECK(a.x == 3.0f && a.y == -3.0f && a.z == 0.5f && a.w == 1.0f);
        const Px b = reduce_block(img.data(), W, H, 2, 1, 0);  // 3 / 6: two pixels
        CHECK(b.x == 4.5f && b.w == 1.0f);
        const Px c = reduce_block(img.data(), W, H, 2, 1, 1);  // 9: one pixel
        CHECK(c.x == 9.0f && c.y == -9.0f);
        const Px d = reduce_block(img.data(), W, H, 8, 0, 0);  // everything: 45 / 9
        CHECK(d.x == 5.0f && d.z == 0.5f);
        // the order: (((0 + 1e8) + 1) + -1e8) + 1 is 1 in float32, not 2 and not 0
        const Px row[4] = {{1e8f, 0, 0, 0}, {1.0f, 0, 0, 0}, {-1e8f, 0, 0, 0}, {1.0f, 0, 0, 0}};
        CHECK(reduce_block(row, 4, 1, 4, 0, 0).x == 0.25f);
        const Px col = reduce_block(row, 2, 2, 2, 0, 0);  // the same values as rows of two: the same order
        CHECK(col.x == 0.25f);
    }
    if (g_failed) {
        std::printf("multi_output_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("multi_output_check: ok\n");
    return 0;
}
