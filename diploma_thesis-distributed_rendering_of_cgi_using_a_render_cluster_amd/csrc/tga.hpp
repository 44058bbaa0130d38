// The device TARGA coder (tga.hip): the body of a "TARGA" (run-length coded by
// the rule of tga_rule.h) or "TARGA_RAW" file from a slot's RGBA8 image, rows
// bottom first, pixels B, G, R(, A) or the grey code. The body is formed in a
// dense device buffer and gathered into pinned host memory as
// [uint64 length][8 B pad][bytes] with 16-byte stores; the host puts the
// 18-byte header in front (image_io tga_header_bytes).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rr {

// Pixels a workgroup of k_tga_size takes of its row per step (one a lane).
constexpr int kTgaChunk = 256;

struct TgaPlan {
    int W, H, C;
    bool rle;
    uint32_t body_cap;  // bytes the body takes at most (tga_body_max_bytes), the raw body's exact length
};

// false: a size outside the format (W or H above 65535, C not 1, 3 or 4) or a
// body of 2 GB and more.
bool tga_plan(int W, int H, int C, bool rle, TgaPlan& p);

// The slot scratch, carved from one allocation of 32-bit words. Per pixel of a
// run-length coded frame k_tga_size leaves 5 bytes for k_tga_emit: `rec`, the
// pixel's byte offset in its coded row | writes its C bytes << 30 | first of
// its packet << 31, and `hdr`, at a packet's first pixel the packet's header
// byte. row_bytes / row_off: per file row its coded length and its offset in
// the body; total: the body's length (4 words, one used).
struct TgaBufs {
    uint8_t* body;  // body_cap bytes rounded up to 16, + 16
    uint32_t *rec, *row_bytes, *row_off, *total;
    uint8_t* hdr;
    size_t words;
};
TgaBufs tga_carve(const TgaPlan& p, uint32_t* base);  // base nullptr: only `words`
size_t tga_scratch_words(const TgaPlan& p);

// Enqueues the coder on st: host_out (device-visible pinned memory of
// body_stream_bytes(p.body_cap)) gets the stream. Reads d_rgba, writes scratch and host_out.
void tga_encode_device(const uint8_t* d_rgba, const TgaPlan& p, uint32_t* scratch, uint8_t* host_out, hipStream_t st);

}  // namespace rr
