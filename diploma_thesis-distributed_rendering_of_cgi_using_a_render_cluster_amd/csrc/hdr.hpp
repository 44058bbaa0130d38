// The device HDR coder (hdr.hip): the body of a Radiance RGBE file ("HDR") from
// a slot's film, rows top first: per pixel the RGBE quad of the film's means
// (film x inv_spp; C = 1: the Rec.709 luma of the means in R, G and B), the
// rows run-length coded plane by plane, or flat, by the rules of hdr_rule.h.
// The body is formed in a dense device buffer and gathered into pinned host
// memory as [uint64 length][8 B pad][bytes] with 16-byte stores; the host puts
// the text header in front (image_io hdr_header_bytes).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rr {

// Bytes a workgroup of k_hdr_size takes of its plane per step (one a lane).
constexpr int kHdrChunk = 256;

struct HdrPlan {
    int W, H, C;        // C: 3, or 1 for R = G = B = luma
    bool flat;          // hdr_row_flat(W): the body is the quads
    uint32_t body_cap;  // bytes the body takes at most (hdr_body_max_bytes), a flat body's exact length
};

// false: W or H not positive, C not 1 or 3, or a body bound of 2 GB and more.
bool hdr_plan(int W, int H, int C, HdrPlan& p);

// The slot scratch, carved from one allocation of 32-bit words. quad: a word a
// pixel, the file's R, G, B, E bytes (a flat body as it is). Per plane byte of
// a coded frame k_hdr_size leaves 5 bytes for k_hdr_emit: `rec`, the byte's
// offset in its coded plane | writes its byte << 30 | first of its packet << 31,
// and `hdr`, at a packet's first byte the packet's header byte; both indexed
// (4 row + plane) W + x. plane_bytes: per row and plane the coded length;
// row_off: per row its offset in the body; total: the body's length (4 words,
// one used).
struct HdrBufs {
    uint32_t* quad;  // W H words rounded up to 16 bytes, + 16
    uint8_t* body;   // coded: body_cap bytes rounded up to 16, + 16
    uint32_t *rec, *plane_bytes, *row_off, *total;
    uint8_t* hdr;
    size_t words;
};
HdrBufs hdr_carve(const HdrPlan& p, uint32_t* base);  // base nullptr: only `words`
size_t hdr_scratch_words(const HdrPlan& p);

// Enqueues the coder on st: host_out (device-visible pinned memory of
// body_stream_bytes(p.body_cap)) gets the stream. Reads the film, writes scratch and host_out.
void hdr_encode_device(const float4* d_film, float inv_spp, const HdrPlan& p, uint32_t* scratch, uint8_t* host_out,
                       hipStream_t st);

}  // namespace rr
