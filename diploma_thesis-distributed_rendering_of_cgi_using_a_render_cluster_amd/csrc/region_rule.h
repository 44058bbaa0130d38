// The render region (rr_set_region; Blender's render border): which pixels of
// a W x H frame it covers. Stated once, for the settings (settings.cpp
// resolve_region) and the checks of tests/cpp/region_check.cpp.
//
// A region is a half-open rectangle of full-frame pixels, rows top first:
// x0 <= x < x1, y0 <= y < y1. region_clamp cuts it to the frame; what is left
// may be empty (x0 >= x1 or y0 >= y1), which refuses the frame.
//
// A scene's border (render.border) holds Blender's fractions of the frame,
// min_x, max_x, min_y, max_y in [0, 1], y measured from the BOTTOM edge.
// The pixel rule, recalled from the disprect Blender's render pipeline forms
// and not checked against a Blender (DESIGN.md §8 lists it as unpinned):
//   xmin = (int)(min_x * W)   xmax = (int)(max_x * W)       (float32 product,
//   ymin = (int)(min_y * H)   ymax = (int)(max_y * H)        truncated)
// and, with rows counted from the top, x0 = xmin, x1 = xmax, y0 = H - ymax,
// y1 = H - ymin. min == max gives an empty region.
//
// Host code includes this without any HIP header.
#pragma once

namespace rr {

struct RegionRect {
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    constexpr bool empty() const { return x0 >= x1 || y0 >= y1; }
    constexpr int w() const { return x1 - x0; }
    constexpr int h() const { return y1 - y0; }
};

constexpr RegionRect region_clamp(RegionRect r, int W, int H) {
    if (r.x0 < 0) r.x0 = 0;
    if (r.y0 < 0) r.y0 = 0;
    if (r.x1 > W) r.x1 = W;
    if (r.y1 > H) r.y1 = H;
    return r;
}

inline int border_pixel(double fraction, int n) { return (int)((float)fraction * (float)n); }

inline RegionRect region_of_border(double min_x, double max_x, double min_y, double max_y, int W, int H) {
    RegionRect r;
    r.x0 = border_pixel(min_x, W);
    r.x1 = border_pixel(max_x, W);
    r.y0 = H - border_pixel(max_y, H);
    r.y1 = H - border_pixel(min_y, H);
    return r;
}

}  // namespace rr
