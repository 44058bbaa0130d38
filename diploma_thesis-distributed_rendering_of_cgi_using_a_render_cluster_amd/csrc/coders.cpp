// The coders of a frame's file: the dispatch to the device coders (formats.hpp
// lists them), the host-built files around their streams, and the host coders
// of an RGBA8 image. See frame.hpp.
#include <cerrno>
#include <cstring>

#include "api_util.hpp"
#include "frame.hpp"
#include "image_io.hpp"

namespace rr {

static_assert(kSrgb16LutSize == kSrgb16N, "host table and device read agree on the interval count");
void ensure_srgb16(rr_ctx* c) {
    if (c->srgb16_lut.ptr) return;
    std::vector<float> lut(kSrgb16LutSize + 2);
    build_srgb16_lut(lut.data());
    c->srgb16_lut.ensure(lut.size());
    RR_HIP(hipMemcpy(c->srgb16_lut.ptr, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
}

const float* jpeg_table(rr_ctx* c, int quality) {
    if (quality < 1 || quality > 100) throw std::runtime_error("jpeg_quality must be 1..100");
    DevBuf<float>& d = c->jpeg_tab[quality];
    if (d.ptr) return d.ptr;
    JpegTables t;
    jpeg_tables(quality, t);
    float tab[192];  // dct | qinv luma | qinv chroma
    std::memcpy(tab, t.dct, sizeof t.dct);
    std::memcpy(tab + 64, t.qinv_l, sizeof t.qinv_l);
    std::memcpy(tab + 128, t.qinv_c, sizeof t.qinv_c);
    DevBuf<float> fresh;  // a buffer no kernel reads yet: nothing to wait for
    fresh.ensure(192);
    RR_HIP(hipMemcpy(fresh.ptr, tab, sizeof tab, hipMemcpyHostToDevice));
    d = std::move(fresh);
    return d.ptr;
}

std::string webp_quality_warning(int quality) {
    if (quality >= 100) return "";
    return "WEBP at quality " + std::to_string(quality) +
           ": lossy WEBP is not built, the file is lossless (as at quality 100)";
}

namespace {

// The pinned memory p as the device addresses it.
template <class T>
T* device_pointer(const PinnedBuf& p) {
    void* dev = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev, p.ptr, 0));
    return static_cast<T*>(dev);
}

// One body coder, every fact of it here. plan: the format's plan in o and its
// BodyShape (scratch words; what a body holds at least); false: a size out of
// range. launch: enqueues the coder. file: the file around a body of len bytes.
struct BodyCoder {
    bool (*plan)(const FrameOutput& fo, int W, int H, CodedOut& o);
    void (*launch)(const CoderInput& in, const CodedOut& o, uint32_t* scratch, uint8_t* out, hipStream_t st);
    void (*file)(const CodedOut& o, const uint8_t* body, size_t len, std::vector<uint8_t>& data);
};

template <class Plan>
bool shaped(CodedOut& o, Coder k, const Plan& p, size_t scratch_words, uint64_t min_len) {
    o.body = {k, p.W, p.H, p.body_cap, scratch_words, min_len};
    return true;
}

const BodyCoder kTga = {
    [](const FrameOutput& fo, int W, int H, CodedOut& o) {  // a raw body has its exact length
        return tga_plan(W, H, fo.color_mode, !fo.tga_raw, o.tga) &&
               shaped(o, fo.coder, o.tga, tga_scratch_words(o.tga), o.tga.rle ? 0 : o.tga.body_cap);
    },
    [](const CoderInput& in, const CodedOut& o, uint32_t* scratch, uint8_t* out, hipStream_t st) {
        tga_encode_device(in.rgba8, o.tga, scratch, out, st);
    },
    [](const CodedOut& o, const uint8_t* body, size_t len, std::vector<uint8_t>& data) {
        tga_header_bytes(o.tga.W, o.tga.H, o.tga.C, o.tga.rle, data);
        data.insert(data.end(), body, body + len);
    }};
const BodyCoder kHdr = {
    [](const FrameOutput& fo, int W, int H, CodedOut& o) {  // so has a flat one
        return hdr_plan(W, H, fo.color_mode, o.hdr) &&
               shaped(o, fo.coder, o.hdr, hdr_scratch_words(o.hdr), o.hdr.flat ? o.hdr.body_cap : 0);
    },
    [](const CoderInput& in, const CodedOut& o, uint32_t* scratch, uint8_t* out, hipStream_t st) {
        hdr_encode_device(in.film, in.inv_spp, o.hdr, scratch, out, st);
    },
    [](const CodedOut& o, const uint8_t* body, size_t len, std::vector<uint8_t>& data) {
        hdr_header_bytes(o.hdr.W, o.hdr.H, data);
        data.insert(data.end(), body, body + len);
    }};
const BodyCoder kIris = {
    [](const FrameOutput& fo, int W, int H, CodedOut& o) {  // the tables; of every row-plane a packet and its terminator
        return iris_plan(W, H, fo.color_mode, o.iris) &&
               shaped(o, fo.coder, o.iris, iris_scratch_words(o.iris), (8 + 3) * (uint64_t)o.iris.H * (uint64_t)o.iris.C);
    },
    [](const CoderInput& in, const CodedOut& o, uint32_t* scratch, uint8_t* out, hipStream_t st) {
        iris_encode_device(in.rgba8, o.iris, scratch, out, st);
    },
    [](const CodedOut& o, const uint8_t* body, size_t len, std::vector<uint8_t>& data) {
        iris_header_bytes(o.iris.W, o.iris.H, o.iris.C, data);
        data.insert(data.end(), body, body + len);
    }};
const BodyCoder kWebp = {
    [](const FrameOutput& fo, int W, int H, CodedOut& o) {  // the 5 bytes of signature and sizes
        return webp_plan(W, H, fo.color_mode, o.webp) && shaped(o, fo.coder, o.webp, webp_scratch_words(o.webp), 5);
    },
    [](const CoderInput& in, const CodedOut& o, uint32_t* scratch, uint8_t* out, hipStream_t st) {
        webp_encode_device(in.rgba8, o.webp, scratch, out, st);
    },
    [](const CodedOut&, const uint8_t* body, size_t len, std::vector<uint8_t>& data) {
        webp_wrap_stream(body, len, data);  // the RIFF and chunk headers, and the pad byte
    }};
// OPEN_EXR with a chunk per scanline (rr_set_exr_codec NONE, RLE): the body path's
// scratch and stream under the format's own coder rows, Exr and Exr32. NONE has
// its exact length, an RLE body a byte of every scanline at least.
const BodyCoder kExrRows = {
    [](const FrameOutput& fo, int W, int H, CodedOut& o) {
        const bool rle = fo.exr_codec == RR_EXR_CODEC_RLE;
        return exr_rows_plan(W, H, fo.color_mode, coder_info(fo.coder).depth, rle, o.exr_rows) &&
               shaped(o, fo.coder, o.exr_rows, exr_rows_scratch_words(o.exr_rows),
                      rle ? (uint64_t)o.exr_rows.H : o.exr_rows.body_cap);
    },
    [](const CoderInput& in, const CodedOut& o, uint32_t* scratch, uint8_t* out, hipStream_t st) {
        uint32_t* tab = o.exr_rows.rle ? device_pointer<uint32_t>(o.tab) : nullptr;
        exr_rows_encode_device(in.film, in.inv_spp, (in.alpha_mask ? 2 : in.alpha_one ? 1 : 0), o.exr_rows, scratch, out, tab, st);
    },
    [](const CodedOut& o, const uint8_t* body, size_t len, std::vector<uint8_t>& data) {
        const ExrRowsPlan& p = o.exr_rows;
        const uint32_t* tab = p.rle ? reinterpret_cast<const uint32_t*>(o.tab.ptr) : nullptr;
        if (!exr_wrap_rows(p.W, p.H, body, len, tab, data, p.full ? 2 : 1, p.C, p.rle ? 1 : 0))
            throw std::runtime_error("device EXR scanline table does not match its body");
    }};
// Whether fo's file is an OPEN_EXR file coded by kExrRows.
bool exr_rows(const FrameOutput& fo) {
    if (fo.coder != Coder::Exr && fo.coder != Coder::Exr32) return false;
    const int codec = exr_codec_written(fo);
    return codec == RR_EXR_CODEC_NONE || codec == RR_EXR_CODEC_RLE;
}
bool exr_pxr24(const FrameOutput& fo) {
    return (fo.coder == Coder::Exr || fo.coder == Coder::Exr32) && exr_codec_written(fo) == RR_EXR_CODEC_PXR24;
}
const BodyCoder& body_coder(Coder k) {
    if (k == Coder::Exr || k == Coder::Exr32) return kExrRows;
    return k == Coder::Tga ? kTga : k == Coder::Hdr ? kHdr : k == Coder::Iris ? kIris : kWebp;
}

// The length at the head of o's stream, which `what` coded: over(len, cap) says
// whether it is more than that coder can have left in a stream of cap bytes.
template <class Over>
uint64_t stream_len(const CodedOut& o, const std::string& what, Over over) {
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    if (over(len, o.stream.cap)) throw std::runtime_error("device " + what + " stream overflow");
    return len;
}

// What body coder k's plan in o takes of f's scratch and o's pinned buffers.
void reserve_body(Coder k, int W, int H, DevFrame& f, CodedOut& o) {
    const BodyShape& b = o.body;
    if (b.coder != k || b.W != W || b.H != H)
        throw std::runtime_error(std::string(coder_info(k).name) + " plan of another image");
    f.body_scratch.ensure(b.scratch_words);
    o.stream.ensure(body_stream_bytes(b.body_cap));
    if (device_deflate(k) && o.exr_rows.rle) o.tab.ensure((size_t)b.H * 2 * sizeof(uint32_t));  // the scanlines' table
}

// Device encode by body coder k into o's pinned stream, by the plan in o.
void enqueue_body(Coder k, const CoderInput& in, DevFrame& f, hipStream_t st, CodedOut& o) {
    f.prof.begin(st, RR_K_PNG);
    body_coder(k).launch(in, o, f.body_scratch.ptr, device_pointer<uint8_t>(o.stream), st);
    f.prof.end(st);
}

// The file of body coder k's image: a body within the plan's bound and the stream, no less than its least.
void body_file_bytes(const CodedOut& o, Coder k, std::vector<uint8_t>& data) {
    const BodyShape& b = o.body;
    const uint64_t len = stream_len(o, coder_info(k).name, [&](uint64_t len, size_t cap) {
        return len > b.body_cap || len + 16 > cap || len < b.min_len;
    });
    body_coder(k).file(o, o.stream.ptr + 16, (size_t)len, data);
}

// Device JPEG encode of an RGBA8 image (transform into f.jpeg_coeffs + Huffman
// coding) into o's pinned stream. grey: a one-component file (RR_COLOR_BW).
void reserve_jpeg(rr_ctx* c, int W, int H, bool grey, DevFrame& f, CodedOut& o) {
    if (!c->jpeg_huff.ptr) {
        quiesce(c);
        uint32_t h[4 * 256];
        jpeg_huff_tables(h);
        c->jpeg_huff.ensure(4 * 256);
        RR_HIP(hipMemcpy(c->jpeg_huff.ptr, h, sizeof h, hipMemcpyHostToDevice));
    }
    const size_t mcuy = jpeg_mcu_rows(H, grey);
    const size_t nblocks = jpeg_block_count(W, H, grey);
    f.jpeg_coeffs.ensure(jpeg_coeff_count(W, H, grey));
    f.jpeg_blk.ensure(2 * nblocks + 2 * mcuy);
    f.jpeg_scratch.ensure(mcuy * jpeg_row_scratch_words(W, grey));
    o.stream.ensure(jpeg_stream_max_bytes(W, H, grey) + 16);
}

void enqueue_jpeg(rr_ctx* c, const CoderInput& in, bool grey, int quality, DevFrame& f, hipStream_t st, CodedOut& o) {
    const int W = in.W, H = in.H;
    const size_t mcuy = jpeg_mcu_rows(H, grey);
    const size_t nblocks = jpeg_block_count(W, H, grey);
    o.jpeg = {W, H, quality, grey};
    uint32_t* blk = f.jpeg_blk.ptr;
    JpegDevBufs b{blk, blk + nblocks, blk + 2 * nblocks, blk + 2 * nblocks + mcuy, f.jpeg_scratch.ptr};
    jpeg_encode_device(in.rgba8, W, H, grey, in.jpeg_tab, c->jpeg_huff.ptr, f.jpeg_coeffs.ptr, b,
                       device_pointer<uint8_t>(o.stream), st);
}

// The file of a device-coded JPEG: host-built header + the device stream.
void jpeg_file_bytes(const CodedOut& o, std::vector<uint8_t>& data) {
    const uint64_t len =
        stream_len(o, coder_info(Coder::Jpeg).name, [](uint64_t len, size_t cap) { return len + 16 > cap; });
    jpeg_header_bytes(o.jpeg.W, o.jpeg.H, o.jpeg.quality, data, o.jpeg.grey);
    data.insert(data.end(), o.stream.ptr + 16, o.stream.ptr + 16 + len);
}

// The file of a deflate-coded image: the host-built container of format k
// around the device stream. C: the channels the stream was coded with.
// compression: an OPEN_EXR file's attribute, 3 ZIP or 5 PXR24.
void deflate_file_bytes(const CodedOut& o, Coder k, int C, std::vector<uint8_t>& data, int compression = 3) {
    const DeflatePlan& p = o.deflate;
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(o.tab.ptr);
    // one stream: its bound counts the 4 bytes of Adler-32 the host adds
    const uint64_t len = stream_len(o, "deflate", [&](uint64_t len, size_t cap) {
        return len > cap || len + 16 + (p.own_stream ? 0 : 4) > cap;
    });
    switch (k) {
    case Coder::Png8:
    case Coder::Png16:
        png_wrap_stream(p.W, p.H, o.stream.ptr + 16, (size_t)len, tab, p.nbands, data, k == Coder::Png16 ? 16 : 8,
                        C == 4 ? 6 : C == 3 ? 2 : 0);
        break;
    case Coder::Exr:
    case Coder::Exr32:
        if (!exr_wrap_stream(p.W, p.H, o.stream.ptr + 16, (size_t)len, tab, p.nbands, data, k == Coder::Exr32 ? 2 : 1,
                             C, compression))
            throw std::runtime_error("device EXR chunk table does not match its stream");
        break;
    default:
        throw std::runtime_error("not a deflate-coded frame");
    }
}

}  // namespace

int plan_or_refuse(const FrameOutput& fo, int W, int H, CodedOut& o) {
    const Coder k = fo.coder;
    const int C = fo.color_mode;
    DeflatePlan& p = o.deflate;
    const bool ok = exr_rows(fo)        ? kExrRows.plan(fo, W, H, o)
                    : exr_pxr24(fo)     ? pxr24_plan(W, H, C, coder_info(k).depth, p)
                    : k == Coder::Png8  ? png_plan(W, H, C, p)
                    : k == Coder::Png16 ? png16_plan(W, H, C, p)
                    : k == Coder::Exr   ? exr_plan(W, H, C, p)
                    : k == Coder::Exr32 ? exr32_plan(W, H, C, p)
                                        : !device_body(k) || body_coder(k).plan(fo, W, H, o);
    return ok ? RR_OK : fail(RR_EINVAL, coder_info(k).range);
}

void reserve_coder(rr_ctx* c, const FrameOutput& fo, int W, int H, DevFrame& f, CodedOut& o) {
    const Coder k = fo.coder;
    const int C = fo.color_mode;
    if (k == Coder::Jpeg) return reserve_jpeg(c, W, H, C == RR_COLOR_BW, f, o);
    if (device_body(k) || exr_rows(fo)) return reserve_body(k, W, H, f, o);
    if (!device_deflate(k)) throw std::runtime_error("no device coder for this output");
    // the front ends' own buffers. "PNG" at compression 0 .. 100: a filter type
    // per row of the H rows, and at 16 bits the raw scanlines, 2C W H bytes
    // (less than the plan's stream, which is below 2 GB)
    const bool png = k == Coder::Png8 || k == Coder::Png16;
    const bool adaptive = png && fo.png_compression >= 0;
    if (k == Coder::Png16) ensure_srgb16(c);
    if (adaptive) f.png_ftype.ensure((size_t)H);
    if (adaptive && k == Coder::Png16) f.png_raw.ensure((size_t)2 * (size_t)C * (size_t)W * (size_t)H);
    // the coder's scratch and its pinned outputs
    const DeflatePlan& p = o.deflate;
    if (p.W != W || p.H != H) throw std::runtime_error(std::string(coder_info(k).name) + " plan of another image");
    f.deflate_scratch.ensure(deflate_scratch_words(p));
    o.stream.ensure((p.own_stream ? exr_stream_max_bytes(p) : deflate_stream_max_bytes(p)) + 32);
    o.tab.ensure((size_t)p.nbands * (p.own_stream ? 4 : 2) * sizeof(uint32_t));
}

void enqueue_coder(rr_ctx* c, const FrameOutput& fo, const CoderInput& in, DevFrame& f, hipStream_t st, CodedOut& o) {
    const Coder k = fo.coder;
    const int C = fo.color_mode;
    reserve_coder(c, fo, in.W, in.H, f, o);
    if (k == Coder::Jpeg) return enqueue_jpeg(c, in, C == RR_COLOR_BW, fo.quality, f, st, o);
    if (device_body(k) || exr_rows(fo)) return enqueue_body(k, in, f, st, o);
    const bool png = k == Coder::Png8 || k == Coder::Png16;
    const bool adaptive = png && fo.png_compression >= 0;
    Png16Front front{};
    if (k == Coder::Png16) {
        if (in.view_transform >= VIEW_FILMIC && !c->filmic.ready)
            throw std::runtime_error("Filmic view transform without LUTs");
        front = Png16Front{in.film, in.inv_spp, in.exposure_scale, in.view_transform, c->srgb16_lut.ptr,
                           view_args(c, in.view_transform, in.look, in.gamma)};
        front.alpha_mask = in.alpha_mask ? 1 : 0;
    }
    const DeflatePlan& p = o.deflate;
    uint32_t* scratch = f.deflate_scratch.ptr;
    uint8_t* out = device_pointer<uint8_t>(o.stream);
    uint32_t* tab = device_pointer<uint32_t>(o.tab);
    f.prof.begin(st, RR_K_PNG);
    switch (k) {
    case Coder::Png8:
        if (adaptive) png_encode_device_adaptive(in.rgba8, C, p, scratch, f.png_ftype.ptr, out, tab, st);
        else png_encode_device(in.rgba8, C, p, scratch, out, tab, st);
        break;
    case Coder::Png16:
        if (adaptive) png16_encode_device_adaptive(front, C, p, scratch, f.png_raw.ptr, f.png_ftype.ptr, out, tab, st);
        else png16_encode_device(front, C, p, scratch, out, tab, st);
        break;
    case Coder::Exr:  // HALF channels
        if (exr_pxr24(fo)) pxr24_encode_device(in.film, in.inv_spp, (in.alpha_mask ? 2 : in.alpha_one ? 1 : 0), C, 16, p, scratch, out, tab, st);
        else exr_encode_device(in.film, in.inv_spp, (in.alpha_mask ? 2 : in.alpha_one ? 1 : 0), C, p, scratch, out, tab, st);
        break;
    default:  // Coder::Exr32: FLOAT channels
        if (exr_pxr24(fo)) pxr24_encode_device(in.film, in.inv_spp, (in.alpha_mask ? 2 : in.alpha_one ? 1 : 0), C, 32, p, scratch, out, tab, st);
        else exr32_encode_device(in.film, in.inv_spp, (in.alpha_mask ? 2 : in.alpha_one ? 1 : 0), C, p, scratch, out, tab, st);
        break;
    }
    f.prof.end(st);
}

void coded_file_bytes(const CodedOut& o, const FrameOutput& fo, std::vector<uint8_t>& data) {
    if (fo.coder == Coder::Jpeg) jpeg_file_bytes(o, data);
    else if (device_body(fo.coder) || exr_rows(fo)) body_file_bytes(o, fo.coder, data);
    else deflate_file_bytes(o, fo.coder, fo.color_mode, data, exr_pxr24(fo) ? 5 : 3);
}

int do_encode(const uint8_t* rgba, int W, int H, const char* out_path, const char* format, int quality,
              uint64_t* bytes, int mode, int compression) {
    if (!out_path || !format) return fail(RR_EINVAL, "out_path and format are required");
    const Format* f = find_format(format);
    if (!f || coder_info(f->coder).film) return fail(RR_ENOTSUP, unsupported_format(format, true));
    const Coder k = f->coder;
    const int C = resolve_color_mode(mode, f->no_alpha);
    const bool adaptive = compression >= 0;  // "PNG"
    std::vector<uint8_t> data;
    if (k == Coder::Jpeg) {
        if (quality < 1 || quality > 100) return fail(RR_EINVAL, "jpeg_quality must be 1..100");
        if (!encode_jpeg(rgba, W, H, quality, data, 0, C == RR_COLOR_BW)) return fail(RR_EINVAL, "JPEG encode failed");
    } else if (k == Coder::Png8) {
        if (!encode_png(rgba, W, H, data, adaptive ? png_zlib_level(compression) : 1, 0, C, adaptive))
            return fail(RR_EIO, "PNG encode failed");
    } else if (!(k == Coder::Tga    ? encode_tga(rgba, W, H, C, !f->tga_raw, data)
                 : k == Coder::Iris ? encode_iris(rgba, W, H, C, data)
                                    : encode_webp(rgba, W, H, C, data))) {  // lossless: the caller flags a quality below 100
        return fail(RR_EINVAL, coder_info(k).range);
    }
    const std::string path = std::string(out_path) + f->ext;
    if (!write_file(path, data)) return fail(RR_EIO, "cannot write " + path + ": " + std::strerror(errno));
    if (bytes) *bytes = data.size();
    return RR_OK;
}

}  // namespace rr
