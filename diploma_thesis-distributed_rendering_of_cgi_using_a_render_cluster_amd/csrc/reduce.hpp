// The film reduction of a reduced output (rr_frame_output.reduce; reduce.hip):
// a slot's W x H film of float4 sums becomes a ceil(W / K) x ceil(H / K) film of
// sums by the box mean of reduce_rule.h, which the 8-bit pass (view_device) and
// the film-reading coders then take as they take the frame's own.
#pragma once

#include <hip/hip_runtime.h>

#include "reduce_rule.h"

namespace rr {

// Enqueues k_film_reduce<K> on st: out = the reduction of `film` (W x H) at
// factor K, 1, 2, 4 or 8 (anything else throws; a frame runs it at 2, 4 and 8). Reads film, writes out
// (reduced_size(W, K) x reduced_size(H, K) float4), nothing else.
void film_reduce_device(const float4* film, int W, int H, int K, float4* out, hipStream_t st);

// The same image on the host, by the same rule: rgba and out as 4 floats a pixel.
void film_reduce_host(const float* rgba, int W, int H, int K, float* out);

}  // namespace rr
