// 8-bit PNG encode on the device: the Sub-filtered scanlines of the RGBA8 frame
// in front of the deflate coder (deflate.hip), so only the zlib stream crosses
// PCIe and the host writes the chunk framing (image_io png_wrap_stream).
// Replaces the PNG side of Blender's write_still (render-timing-script.py:83-92).
//
// A row is 4W + 1 filtered bytes: filter type 1 (Sub), then every image byte
// less the byte 4 positions (one pixel) before it. The bands are the pieces of
// one zlib stream with the stored fallback; the match distances are 1 (zero
// runs), 4 (the pixel period) and 4W + 1 (the filtered row above).
// Same image -> same bytes.
#include <hip/hip_runtime.h>

#include "deflate.hpp"
#include "device.hpp"

namespace rr {

namespace {

struct Png8Front {
    const uint8_t* __restrict__ rgba;
    __device__ __forceinline__ uint32_t operator()(const DeflatePlan& p, int row0, uint32_t, uint32_t j) const {
        const uint32_t row = j / p.stride, x = j - row * p.stride;
        uint32_t v = 1u;  // filter type Sub
        if (x > 0) {
            const uint8_t* src = rgba + (size_t)(row0 + (int)row) * ((size_t)p.W * 4);
            v = ((uint32_t)src[x - 1] - (x > 4 ? (uint32_t)src[x - 5] : 0u)) & 0xFFu;
        }
        return v;
    }
};

}  // namespace

bool png_plan(int W, int H, DeflatePlan& p) {
    // a band's bit offsets (at most 16 bits a byte) stay below 2^32
    if (W <= 0 || H <= 0 || W > (1 << 20)) return false;
    const bool ok = deflate_plan(W, H, 4u * (uint32_t)W + 1u, p);
    p.dist[0] = 1u;
    p.dist[1] = 4u;
    p.dist[2] = p.stride <= 32768u ? p.stride : 0u;
    return ok;
}

void png_encode_device(const uint8_t* d_rgba, const DeflatePlan& p, uint32_t* scratch, uint8_t* host_out,
                       uint32_t* host_tab, hipStream_t st) {
    const DeflateBufs c = deflate_carve(p, scratch);
    k_deflate_front<<<dim3(p.nsub, p.nbands), 256, 0, st>>>(Png8Front{d_rgba}, p, c.filt, c.adler_part);
    deflate_bands_device(p, c, st);
    deflate_gather_device(p, c, host_out, host_tab, st);
}

}  // namespace rr
