// The device WEBP coder (webp.hip): the VP8L payload of a lossless WebP file
// from a slot's RGBA8 image, by the rules of webp_rule.h: subtract-green, the
// left-neighbour predictor, copies at distance 1, five prefix codes. The payload
// is formed in a dense device buffer and gathered into pinned host memory as
// [uint64 length][8 B pad][bytes] with 16-byte stores; the host puts the RIFF
// and chunk headers in front and the pad byte behind (image_io
// webp_wrap_stream).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rr {

// Pixels a workgroup takes of its row per step (one a lane).
constexpr int kWebpChunk = 256;

struct WebpPlan {
    int W, H, C;
    uint32_t body_cap;  // bytes the payload takes at most (webp_body_max_bytes)
};

// false: W or H outside 1 .. 16384, C not 1, 3 or 4, or a payload bound of 2 GB
// and more.
bool webp_plan(int W, int H, int C, WebpPlan& p);

// The slot scratch, carved from one allocation of 32-bit words. body: the
// payload's words, zeroed where the tokens go before they are ORed in. hist:
// the five alphabets' counts (webp_rule.h's table), zeroed per frame. resid: a
// pixel's residual word. rec: its kind << 30 | at a copy's first pixel the
// copy's length. codes: code | length << 16 per symbol. row_bits / row_off: a
// row's bits and its offset in bits from the end of the header. meta: the
// header's bits, the payload's bytes.
struct WebpBufs {
    uint32_t* body;  // body_cap bytes rounded up to 16, + 32
    uint32_t *hist, *resid, *rec, *codes, *row_bits, *meta;
    uint64_t* row_off;
    size_t words;
};
WebpBufs webp_carve(const WebpPlan& p, uint32_t* base);  // base nullptr: only `words`
size_t webp_scratch_words(const WebpPlan& p);

// Enqueues the coder on st: host_out (device-visible pinned memory of
// body_stream_bytes(p.body_cap)) gets the stream. Reads d_rgba, writes scratch and host_out.
void webp_encode_device(const uint8_t* d_rgba, const WebpPlan& p, uint32_t* scratch, uint8_t* host_out,
                        hipStream_t st);

}  // namespace rr
