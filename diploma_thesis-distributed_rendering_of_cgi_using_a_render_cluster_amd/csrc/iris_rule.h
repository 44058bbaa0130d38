// The rules of Silicon Graphics image files ("IRIS", .rgb), which Blender always
// writes run-length coded, shared by the host encoder (image_io encode_iris) and
// the device coder (iris.hip), and the sizes both take from them.
//
// The file, every number big-endian: a 512-byte header (image_io
// iris_header_bytes), the start table and the length table, H C uint32 entries
// each, then the coded row-planes. A row-plane is one channel of one row: W
// bytes, channel z of the RGBA8 pixels (C = 3, 4: R, G, B(, A)) or the grey code
// of grey.h (C = 1). File row 0 is the image's bottom row. Table entry y + z H
// describes file row y of channel z: its offset from the start of the file, and
// its coded bytes, terminator included. The coded row-planes are contiguous:
// file row 0 first, within a row channel 0 .. C - 1.
//
// The packet rule. No packet crosses a row-plane. Within a row-plane the
// packets follow the shared rule of rle_rule.h with the numbers of IrisRle:
//  - a run of at least 3 bytes is a run stretch (runs of 2 are literals);
//  - a packet stands for at most 127 bytes: the count has 7 bits. A run packet
//    is the byte count and the value, a literal packet the byte 0x80 | count
//    and count bytes;
//  - after the last packet comes one 0 byte, the terminator.
// A row-plane is longest when all of it is literal: W + ceil(W / 127) + 1 bytes.
// UNPINNED: the rule is the project's own and is not pinned against Blender's
// files. Blender's writer, quoted from memory with no Blender to check it
// against: runs from 3 equal bytes, packets of at most 126, and possibly another
// order of the coded row-planes. Every reader goes through the tables and
// returns the same pixels from either; the bytes of the files may differ.
//
// With eq(j) = "byte j equals byte j - 1" (false for j <= 0 and j >= W), byte i
// lies in a run stretch (rle_in_run) when one of the three windows of two
// consecutive eq bits that cover it is all set:
//   eq(i - 1) & eq(i) | eq(i) & eq(i + 1) | eq(i + 1) & eq(i + 2)
// Integers only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rle_rule.h"

#define RR_IRIS_HD RR_RLE_HD

namespace rr {

constexpr uint32_t kIrisMinRun = 3;      // bytes a run stretch has at least
constexpr uint32_t kIrisPacket = 127;    // bytes a packet stands for at most: the count has 7 bits and 0 ends the row
constexpr uint32_t kIrisHeaderBytes = 512;
constexpr int kIrisMaxSide = 65535;      // width and height are uint16 fields

// The bytes a coded row-plane takes at most: all literal, and the terminator.
RR_IRIS_HD constexpr uint64_t iris_plane_max_bytes(uint64_t W) { return W + (W + kIrisPacket - 1) / kIrisPacket + 1; }

// The bytes of the two tables.
RR_IRIS_HD constexpr uint64_t iris_table_bytes(uint64_t H, uint64_t C) { return 8 * H * C; }

// The body's bound: the tables and every row-plane at its maximum. 0: W, H or
// C outside the format, or a bound of 2 GB and more.
RR_IRIS_HD uint64_t iris_body_max_bytes(int W, int H, int C) {
    if (W <= 0 || H <= 0 || W > kIrisMaxSide || H > kIrisMaxSide || (C != 1 && C != 3 && C != 4)) return 0;
    const uint64_t n = (uint64_t)H * (uint64_t)C;
    const uint64_t bound = iris_table_bytes((uint64_t)H, (uint64_t)C) + n * iris_plane_max_bytes((uint64_t)W);
    return bound < (1ull << 31) ? bound : 0;
}

// The numbers of the packet rule for a row-plane's bytes (count: 1 .. 127).
struct IrisRle {
    static constexpr uint32_t kMinRun = kIrisMinRun, kRunPacket = kIrisPacket, kLitPacket = kIrisPacket;
    static constexpr uint32_t kElemBytes = 1;
    static RR_IRIS_HD uint32_t header(bool run, uint32_t count) { return (run ? 0u : 0x80u) | count; }
};

}  // namespace rr
