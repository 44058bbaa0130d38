// The render region without a GPU: links csrc/settings.cpp alone (host code,
// no HIP header). Checks the setter's range, every spelling of RR_REGION, the
// fraction-to-pixel rule of region_rule.h at its edges, the clamp, what a frame
// resolves to with and without the scene's border, and the refusal of a region
// that is empty inside the frame. Built with the system C++ compiler under
// AddressSanitizer and UBSan by tests/test_region_format.py; exits 0 when
// everything holds.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "region_rule.h"
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

static bool has(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }
static bool is(const RegionRect& r, int x0, int y0, int x1, int y1) {
    return r.x0 == x0 && r.y0 == y0 && r.x1 == x1 && r.y1 == y1;
}

int main() {
    std::string err;
    CHECK(RR_ABI_VERSION == 8);
    {  // off by default; the setter's range
        OutputSettings s;
        CHECK(!s.region_on && !s.region_from_scene && !s.region_crop);
        CHECK(set_region(s, 3, 5, 61, 44, true, err) && s.region_on && s.region_crop && is(s.region, 3, 5, 61, 44));
        CHECK(set_region(s, -5, -5, 1 << 30, 1 << 30, false, err) && !s.region_crop);  // beyond a frame: allowed
        CHECK(set_region(s, 0, 0, 1, 1, false, err));
        const int bad[][4] = {{10, 10, 10, 20}, {10, 10, 20, 10}, {20, 5, 10, 9}, {5, 20, 9, 10}, {0, 0, 0, 0},
                              {0, 0, (1 << 30) + 1, 1}, {-(1 << 30) - 1, 0, 1, 1}, {0, 0, 1, (1 << 30) + 1}};
        for (const auto& b : bad) {
            err.clear();
            CHECK(!set_region(s, b[0], b[1], b[2], b[3], true, err));
            CHECK(has(err, "x0 < x1 and y0 < y1"));
            CHECK(s.region_on && !s.region_crop && is(s.region, 0, 0, 1, 1));  // a refusal changes nothing
        }
        set_region_off(s);
        CHECK(!s.region_on);
    }
    {  // RR_REGION, good
        OutputSettings s;
        CHECK(setting_from_text(s, "RR_REGION", "3,5,61,44,1", err) && s.region_on && s.region_crop);
        CHECK(is(s.region, 3, 5, 61, 44));
        CHECK(setting_from_text(s, "RR_REGION", "0,0,70,45", err) && !s.region_crop && is(s.region, 0, 0, 70, 45));
        CHECK(setting_from_text(s, "RR_REGION", "-4,-4,7,9,0", err) && !s.region_crop && is(s.region, -4, -4, 7, 9));
        CHECK(setting_from_text(s, "RR_REGION", "scene", err) && s.region_from_scene && s.region_on);
        CHECK(setting_from_text(s, "RR_REGION", "", err) && !s.region_from_scene && !s.region_on);
    }
    // RR_REGION, malformed: refused with the variable and the text, nothing changed
    for (const char* bad : {"3,5,61", "3,5,61,44,2", "3,5,61,44,1,0", "3,5,61,44,", ",3,5,61,44", "3,,5,61,44",
                            " 3,5,61,44", "3, 5,61,44", "3,5,61,44 ", "a,b,c,d", "3.0,5,61,44", "03,5,61,44", "+3,5,61,44",
                            "3;5;61;44", "Scene", "off", "61,5,3,44", "3,44,61,5", "3,5,3,44", "99999999999,0,1,1",
                            "3,5,61,44,-1", "0x3,5,61,44", ","}) {
        OutputSettings s;
        CHECK(set_region(s, 1, 2, 3, 4, true, err));
        err.clear();
        CHECK(!setting_from_text(s, "RR_REGION", bad, err));
        CHECK(has(err, std::string("RR_REGION='") + bad + "'"));
        CHECK(s.region_on && s.region_crop && is(s.region, 1, 2, 3, 4) && !s.region_from_scene);
    }
    {  // settings_from_env reads it, and a bad text leaves the settings alone
        OutputSettings s;
        setenv("RR_REGION", "8,8,24,16,1", 1);
        CHECK(settings_from_env(s, err) && s.region_on && s.region_crop && is(s.region, 8, 8, 24, 16));
        setenv("RR_REGION", "8,8,24", 1);
        CHECK(!settings_from_env(s, err) && has(err, "RR_REGION='8,8,24'") && is(s.region, 8, 8, 24, 16));
        unsetenv("RR_REGION");
    }
    {  // the pixel rule: x = (int)(fraction * n) in float32, y from the bottom
        CHECK(border_pixel(0.0, 70) == 0 && border_pixel(1.0, 70) == 70 && border_pixel(1.0, 1) == 1);
        CHECK(border_pixel(0.5, 70) == 35 && border_pixel(0.5, 45) == 22);  // 22.5 truncates
        CHECK(border_pixel(0.1, 70) == 7 && border_pixel(0.2, 45) == 9 && border_pixel(0.3, 10) == 3);  // whole products
        CHECK(border_pixel(0.7, 10) == 7 && border_pixel(0.6, 5) == 3 && border_pixel(0.9, 10) == 9);
        CHECK(border_pixel(0.999, 70) == 69 && border_pixel(0.0142, 70) == 0 && border_pixel(0.0143, 70) == 1);
        CHECK(is(region_of_border(0.0, 1.0, 0.0, 1.0, 70, 45), 0, 0, 70, 45));
        // the bottom fifth of the frame is its last rows
        CHECK(is(region_of_border(0.1, 0.5, 0.0, 0.2, 70, 45), 7, 36, 35, 45));
        CHECK(is(region_of_border(0.1, 0.5, 0.8, 1.0, 70, 45), 7, 0, 35, 9));
        CHECK(region_of_border(0.3, 0.3, 0.0, 1.0, 70, 45).empty());  // min == max
        CHECK(region_of_border(0.0, 1.0, 0.4, 0.4, 70, 45).empty());
        CHECK(region_of_border(0.30, 0.31, 0.0, 1.0, 10, 10).empty());  // both truncate to 3
        CHECK(is(region_clamp(RegionRect{-5, -5, 500, 400}, 70, 45), 0, 0, 70, 45));
        CHECK(region_clamp(RegionRect{70, 0, 90, 45}, 70, 45).empty());
        CHECK(is(region_clamp(RegionRect{60, 40, 500, 400}, 70, 45), 60, 40, 70, 45));
    }
    {  // what a frame resolves to
        OutputSettings s;
        RenderDesc r;
        FrameRegion f;
        CHECK(resolve_region(s, r, 70, 45, f, err) && !f.on && f.out_w(70) == 70 && f.out_h(45) == 45);
        CHECK(set_region(s, 3, 5, 61, 44, true, err));
        CHECK(resolve_region(s, r, 70, 45, f, err) && f.on && f.crop && is(f.r, 3, 5, 61, 44));
        CHECK(f.out_w(70) == 58 && f.out_h(45) == 39);
        CHECK(set_region(s, 3, 5, 61, 44, false, err));
        CHECK(resolve_region(s, r, 70, 45, f, err) && f.on && !f.crop && f.out_w(70) == 70 && f.out_h(45) == 45);
        CHECK(set_region(s, 60, 40, 500, 400, true, err));  // clamped, not refused
        CHECK(resolve_region(s, r, 70, 45, f, err) && f.on && is(f.r, 60, 40, 70, 45) && f.out_w(70) == 10);
        CHECK(set_region(s, -5, -5, 500, 400, true, err));  // the whole frame: the frame without a region
        CHECK(resolve_region(s, r, 70, 45, f, err) && !f.on && f.out_w(70) == 70);
        CHECK(set_region(s, 70, 0, 90, 45, true, err));  // nothing inside: refused, naming both
        err.clear();
        CHECK(!resolve_region(s, r, 70, 45, f, err));
        CHECK(has(err, "(70, 0, 90, 45)") && has(err, "70 x 45"));
        CHECK(resolve_region(s, r, 128, 45, f, err) && f.on && is(f.r, 70, 0, 90, 45));  // judged per frame
        // the scene's border: ignored without the opt-in, first with it
        r.has_border = true;
        r.border_min_x = 0.1;
        r.border_max_x = 0.5;
        r.border_min_y = 0.0;
        r.border_max_y = 0.2;
        r.border_crop = true;
        set_region_off(s);
        CHECK(resolve_region(s, r, 70, 45, f, err) && !f.on);
        CHECK(set_region(s, 3, 5, 61, 44, false, err));
        CHECK(resolve_region(s, r, 70, 45, f, err) && f.on && !f.crop && is(f.r, 3, 5, 61, 44));
        set_region_from_scene(s, true);
        CHECK(resolve_region(s, r, 70, 45, f, err) && f.on && f.crop && is(f.r, 7, 36, 35, 45));
        r.has_border = false;  // a scene without one leaves the context's in force
        CHECK(resolve_region(s, r, 70, 45, f, err) && f.on && !f.crop && is(f.r, 3, 5, 61, 44));
        r.has_border = true;
        r.border_max_x = 0.1;  // min == max: empty, refused
        err.clear();
        CHECK(!resolve_region(s, r, 70, 45, f, err) && has(err, "70 x 45"));
    }
    if (g_failed) {
        std::printf("region_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("region_check: ok\n");
    return 0;
}
