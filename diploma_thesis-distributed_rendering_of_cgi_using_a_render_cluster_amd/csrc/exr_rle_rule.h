// The packet rule of RLE chunks of OPEN_EXR files (rr_set_exr_codec
// RR_EXR_CODEC_RLE), shared by the host statement (image_io exr_rle_pack) and
// the device coder (exr_codec.hip).
//
// A chunk is one scanline. Its n bytes (the planes' halfs or floats) are
// reordered and differenced as for ZIP (exr_samples.hpp exr_pred_byte); the
// elements of the rule are those n bytes, and the packets follow the shared
// rule of rle_rule.h with the numbers of ExrRle:
//  - a run of at least 3 equal bytes is a run stretch;
//  - a run packet stands for at most 128 bytes: the byte count - 1 (0 .. 127)
//    and the value;
//  - a literal packet holds at most 127 bytes: the byte -count as a signed
//    char (count 1 .. 127) and its bytes.
// OpenEXR's decoder is the contract: a negative count copies -count bytes,
// otherwise count + 1 copies of the next byte. Which bytes go into which
// packet is the project's own rule, not pinned against OpenEXR's own writer;
// every decoder returns the same bytes. A scanline whose packets are not
// shorter than n is stored as its n unprocessed bytes (OpenEXR's rule for
// every codec). Integers only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rle_rule.h"

namespace rr {

struct ExrRle {
    static constexpr uint32_t kMinRun = 3;
    static constexpr uint32_t kRunPacket = 128, kLitPacket = 127;
    static constexpr uint32_t kElemBytes = 1;
    static RR_RLE_HD uint32_t header(bool run, uint32_t count) { return (run ? count - 1u : 0u - count) & 0xFFu; }
};

// The bytes the packets of n bytes take at most (all literal).
RR_RLE_HD constexpr uint64_t exr_rle_row_max_bytes(uint64_t n) { return n + (n + ExrRle::kLitPacket - 1) / ExrRle::kLitPacket; }

// The widest scanline: 4 channels of 2^18 floats (exr32_plan), or of 2^19 halfs.
constexpr uint64_t kExrRleMaxRowBytes = 16ull << 18;

}  // namespace rr
