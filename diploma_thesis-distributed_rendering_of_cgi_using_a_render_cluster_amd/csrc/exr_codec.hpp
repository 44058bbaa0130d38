// The device coders of OPEN_EXR files with a chunk per scanline (exr_codec.hip;
// rr_set_exr_codec RR_EXR_CODEC_NONE and RR_EXR_CODEC_RLE): the chunks'
// payloads back to back from a slot's film, into pinned host memory as
// [uint64 length][8 B pad][bytes], and for RLE a table {mode, bytes} per
// scanline (mode 0 packets, 1 the raw scanline). The host writes the header,
// the offset table and the chunk framing (image_io exr_wrap_rows). Plain host
// header: frame.hpp includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rr {

struct ExrRowsPlan {
    int W, H, C;
    bool full;           // FLOAT channels, else HALF
    bool rle;            // RLE, else NONE
    uint32_t row_bytes;  // a scanline's bytes: 2 C W or 4 C W
    // the body's bound, the raw size H * row_bytes: a scanline whose packets are
    // not shorter is stored raw, so no body is longer (NONE: its exact length)
    uint32_t body_cap;
};

struct ExrRowsBufs {
    uint8_t* body;        // the dense body
    uint32_t* total;      // its length
    uint32_t* rec;        // RLE: a record per byte of the image (rle_device.hpp)
    uint8_t* hdr;         // RLE: the packets' header bytes, at their first bytes
    uint32_t* row_bytes;  // RLE: the scanlines' packed lengths
    uint32_t* row_off;    // RLE: the scanlines' offsets in the body
    size_t words;
};

// false: a size outside the range of the ZIP coder at the same depth (W above
// 2^19 at 16, 2^18 at 32; a file of 2 GB and more). depth: 16 or 32.
bool exr_rows_plan(int W, int H, int C, int depth, bool rle, ExrRowsPlan& p);
ExrRowsBufs exr_rows_carve(const ExrRowsPlan& p, uint32_t* base);  // base nullptr: only `words`
size_t exr_rows_scratch_words(const ExrRowsPlan& p);
// film: W x H float4 sums, scaled by inv_spp; alpha_one: A = 1.0 (rendered
// frames), else film.w * inv_spp. host_tab (RLE): 2 H words of pinned memory.
void exr_rows_encode_device(const float4* d_film, float inv_spp, int alpha_one, const ExrRowsPlan& p,
                            uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st);

}  // namespace rr
