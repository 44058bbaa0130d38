// The device IRIS coder (iris.hip): the body of a Silicon Graphics image file
// ("IRIS", .rgb) from a slot's RGBA8 image: the start table and the length
// table, big-endian, and the row-planes run-length coded by the rule of
// iris_rule.h, rows bottom first, channels R, G, B(, A) or the grey code. The
// body is formed in a dense device buffer and gathered into pinned host memory
// as [uint64 length][8 B pad][bytes] with 16-byte stores; the host puts the
// 512-byte header in front (image_io iris_header_bytes).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rr {

// Bytes a workgroup of k_iris_size takes of its row-plane per step (one a lane).
constexpr int kIrisChunk = 256;

struct IrisPlan {
    int W, H, C;
    uint32_t body_cap;  // bytes the body takes at most (iris_body_max_bytes)
};

// false: a size outside the format (W or H above 65535, C not 1, 3 or 4) or a
// body bound of 2 GB and more.
bool iris_plan(int W, int H, int C, IrisPlan& p);

// The slot scratch, carved from one allocation of 32-bit words. Per byte of a
// row-plane k_iris_size leaves 5 bytes for k_iris_emit: `rec`, the byte's
// offset in its coded row-plane | writes its byte << 30 | first of its packet
// << 31, and `hdr`, at a packet's first byte the packet's header byte; both
// indexed (file row C + channel) W + x. plane_bytes / plane_off: per file row
// and channel, in the order of the coded row-planes, the coded length and the
// offset in the body; total: the body's length (4 words, one used).
struct IrisBufs {
    uint8_t* body;  // body_cap bytes rounded up to 16, + 16
    uint32_t *rec, *plane_bytes, *plane_off, *total;
    uint8_t* hdr;
    size_t words;
};
IrisBufs iris_carve(const IrisPlan& p, uint32_t* base);  // base nullptr: only `words`
size_t iris_scratch_words(const IrisPlan& p);

// Enqueues the coder on st: host_out (device-visible pinned memory of
// body_stream_bytes(p.body_cap)) gets the stream. Reads d_rgba, writes scratch and host_out.
void iris_encode_device(const uint8_t* d_rgba, const IrisPlan& p, uint32_t* scratch, uint8_t* host_out,
                        hipStream_t st);

}  // namespace rr
