// The windowed film of a region frame (rr_set_region; region.hip): from a
// slot's full W x H film of float4 sums, either the region's w x h pixels alone
// (crop) or the full frame with (0, 0, 0, 0) outside the region. The 8-bit pass
// (view_device), the reduction and the film-reading coders then take it as they
// take a frame's own film, at its own size.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "region_rule.h"

namespace rr {

// Enqueues k_film_window on st. r: inside the W x H frame and not empty
// (anything else throws). crop: out is r.w() x r.h(), else W x H. Inside the
// region out = (film.x, film.y, film.z, alpha_sum): the colour sums' own bits
// and in w what the caller marks the inside with (a frame passes 1: the coders
// of an uncropped frame read w != 0 as "inside", CoderInput::alpha_mask, and
// rescale nothing); outside (no crop) zeros, and the film
// there is never read: a split-path region frame leaves it unwritten.
void film_window_device(const float4* film, int W, int H, RegionRect r, bool crop, float alpha_sum, float4* out,
                        hipStream_t st);

// The 8-bit image of an uncropped region frame: every pixel of the W x H image
// outside r becomes (0, 0, 0, 0) (the view pass writes A = 255 everywhere, and
// a dither may lift the black outside).
void window_mask8_device(uint8_t* rgba8, int W, int H, RegionRect r, hipStream_t st);

}  // namespace rr
