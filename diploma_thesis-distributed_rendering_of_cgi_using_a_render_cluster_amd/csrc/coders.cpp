// The coders of a frame's file: the dispatch to the device coders (jpeg.hip,
// png.hip, png16.hip, exr.hip, tga.hip, hdr.hip, iris.hip, webp.hip), the host-built files around their streams, and
// the host coders of an RGBA8 image. See frame.hpp.
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

void ensure_jpeg_table(rr_ctx* c, int quality) {
    if (c->jpeg_tab_quality == quality) return;
    quiesce(c);
    JpegTables t;
    jpeg_tables(quality, t);
    float tab[192];  // dct | qinv luma | qinv chroma
    std::memcpy(tab, t.dct, sizeof t.dct);
    std::memcpy(tab + 64, t.qinv_l, sizeof t.qinv_l);
    std::memcpy(tab + 128, t.qinv_c, sizeof t.qinv_c);
    c->jpeg_tab.ensure(192);
    RR_HIP(hipMemcpy(c->jpeg_tab.ptr, tab, sizeof tab, hipMemcpyHostToDevice));
    c->jpeg_tab_quality = quality;
}

int plan_or_refuse(Coder k, int C, int W, int H, DeflatePlan& p) {
    const bool ok = k == Coder::Png8    ? png_plan(W, H, C, p)
                    : k == Coder::Png16 ? png16_plan(W, H, C, p)
                    : k == Coder::Exr32 ? exr32_plan(W, H, C, p)
                                        : exr_plan(W, H, C, p);
    if (ok) return RR_OK;
    const char* name = k == Coder::Png8    ? "PNG"
                       : k == Coder::Png16 ? "16-bit PNG"
                       : k == Coder::Exr32 ? "32-bit EXR"
                                           : "EXR";
    return fail(RR_EINVAL, std::string("image size outside the device ") + name + " encoder's range");
}

static const char* const kIrisRange =
    "image size outside the IRIS format's range (65535 x 65535, a body bound below 2 GB)";
static const char* const kWebpRange =
    "image size outside the WEBP format's range (16384 x 16384, a payload bound below 2 GB)";

int plan_or_refuse(const FrameOutput& fo, int W, int H, BodyOut& o) {
    const int C = fo.color_mode;
    switch (fo.coder) {
    case Coder::Tga:
        if (tga_plan(W, H, C, !fo.tga_raw, o.tga)) return RR_OK;
        return fail(RR_EINVAL, "image size outside the TARGA format's range (65535 x 65535, a body below 2 GB)");
    case Coder::Hdr:
        if (hdr_plan(W, H, C, o.hdr)) return RR_OK;
        return fail(RR_EINVAL, "image size outside the HDR coder's range (a body bound below 2 GB)");
    case Coder::Iris:
        return iris_plan(W, H, C, o.iris) ? RR_OK : fail(RR_EINVAL, kIrisRange);
    case Coder::Webp:
        return webp_plan(W, H, C, o.webp) ? RR_OK : fail(RR_EINVAL, kWebpRange);
    default:
        return RR_OK;  // no body coder: nothing to plan
    }
}

std::string webp_quality_warning(int quality) {
    if (quality >= 100) return "";
    return "WEBP at quality " + std::to_string(quality) +
           ": lossy WEBP is not built, the file is lossless (as at quality 100)";
}

namespace {

// Device encode by a body coder (TARGA, HDR, IRIS, WEBP) into o's pinned
// stream, by the format's plan p: launch(scratch, host_out) enqueues it.
template <class Plan, class Launch>
void enqueue_body(const char* name, const Plan& p, size_t scratch_words, const CoderInput& in, DevFrame& f,
                  hipStream_t st, BodyOut& o, Launch launch) {
    if (p.W != in.W || p.H != in.H) throw std::runtime_error(std::string(name) + " plan of another image");
    f.body_scratch.ensure(scratch_words);
    o.stream.ensure(body_stream_bytes(p.body_cap));
    void* dev_host = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, o.stream.ptr, 0));
    f.prof.begin(st, RR_K_PNG);
    launch(f.body_scratch.ptr, static_cast<uint8_t*>(dev_host));
    f.prof.end(st);
}

void enqueue_body(Coder k, const CoderInput& in, DevFrame& f, hipStream_t st, BodyOut& o) {
    if (k == Coder::Tga)
        enqueue_body("TARGA", o.tga, tga_scratch_words(o.tga), in, f, st, o, [&](uint32_t* scratch, uint8_t* out) {
            tga_encode_device(in.rgba8, o.tga, scratch, out, st);
        });
    else if (k == Coder::Hdr)
        enqueue_body("HDR", o.hdr, hdr_scratch_words(o.hdr), in, f, st, o, [&](uint32_t* scratch, uint8_t* out) {
            hdr_encode_device(in.film, in.inv_spp, o.hdr, scratch, out, st);
        });
    else if (k == Coder::Iris)
        enqueue_body("IRIS", o.iris, iris_scratch_words(o.iris), in, f, st, o, [&](uint32_t* scratch, uint8_t* out) {
            iris_encode_device(in.rgba8, o.iris, scratch, out, st);
        });
    else
        enqueue_body("WEBP", o.webp, webp_scratch_words(o.webp), in, f, st, o, [&](uint32_t* scratch, uint8_t* out) {
            webp_encode_device(in.rgba8, o.webp, scratch, out, st);
        });
}

// The checked length of the body in o's stream: within the plan's bound
// body_cap and the stream, and at least min_len (an exact length: body_cap).
uint64_t body_stream_len(const BodyOut& o, const char* name, uint32_t body_cap, uint64_t min_len) {
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    if (len > body_cap || len + 16 > o.stream.cap || len < min_len)
        throw std::runtime_error(std::string("device ") + name + " stream overflow");
    return len;
}

// The file of a device-coded TARGA, HDR, IRIS or WEBP image: the host-built
// header + the device body. What a body holds at least: a raw TARGA and a flat
// HDR body their exact length; IRIS the tables and every coded row-plane a
// packet and its terminator; WEBP the 5 bytes of signature and sizes, inside
// the host-built RIFF and chunk headers.
void body_file_bytes(const BodyOut& o, Coder k, std::vector<uint8_t>& data) {
    const uint8_t* body = o.stream.ptr + 16;
    if (k == Coder::Tga) {
        const TgaPlan& p = o.tga;
        const uint64_t len = body_stream_len(o, "TARGA", p.body_cap, p.rle ? 0 : p.body_cap);
        tga_header_bytes(p.W, p.H, p.C, p.rle, data);
        data.insert(data.end(), body, body + len);
    } else if (k == Coder::Hdr) {
        const HdrPlan& p = o.hdr;
        const uint64_t len = body_stream_len(o, "HDR", p.body_cap, p.flat ? p.body_cap : 0);
        hdr_header_bytes(p.W, p.H, data);
        data.insert(data.end(), body, body + len);
    } else if (k == Coder::Iris) {
        const IrisPlan& p = o.iris;
        const uint64_t planes = (uint64_t)p.H * (uint64_t)p.C;
        const uint64_t len = body_stream_len(o, "IRIS", p.body_cap, 8 * planes + 3 * planes);
        iris_header_bytes(p.W, p.H, p.C, data);
        data.insert(data.end(), body, body + len);
    } else {
        webp_wrap_stream(body, (size_t)body_stream_len(o, "WEBP", o.webp.body_cap, 5), data);
    }
}

// Device JPEG encode of an RGBA8 image (transform into f.jpeg_coeffs + Huffman
// coding) into o's pinned stream. grey: a one-component file (RR_COLOR_BW).
void enqueue_jpeg(rr_ctx* c, const CoderInput& in, bool grey, int quality, DevFrame& f, hipStream_t st, JpegOut& o) {
    const int W = in.W, H = in.H;
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
    o.W = W;
    o.H = H;
    o.quality = quality;
    o.grey = grey;
    void* dev_host = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, o.stream.ptr, 0));
    uint32_t* blk = f.jpeg_blk.ptr;
    JpegDevBufs b{blk, blk + nblocks, blk + 2 * nblocks, blk + 2 * nblocks + mcuy, f.jpeg_scratch.ptr};
    jpeg_encode_device(in.rgba8, W, H, grey, in.jpeg_tab, c->jpeg_huff.ptr, f.jpeg_coeffs.ptr, b,
                       static_cast<uint8_t*>(dev_host), st);
}

// The file of a device-coded JPEG: host-built header + the device stream.
void jpeg_file_bytes(const JpegOut& o, std::vector<uint8_t>& data) {
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    if (len + 16 > o.stream.cap) throw std::runtime_error("device JPEG stream overflow");
    jpeg_header_bytes(o.W, o.H, o.quality, data, o.grey);
    data.insert(data.end(), o.stream.ptr + 16, o.stream.ptr + 16 + len);
}

// The file of a deflate-coded image: the host-built container of format k
// around the device stream. C: the channels the stream was coded with.
void deflate_file_bytes(const DeflateOut& o, Coder k, int C, std::vector<uint8_t>& data) {
    const DeflatePlan& p = o.plan;
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(o.tab.ptr);
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    // one stream: its bound counts the 4 bytes of Adler-32 the host adds
    if (len > o.stream.cap || len + 16 + (p.own_stream ? 0 : 4) > o.stream.cap)
        throw std::runtime_error("device deflate stream overflow");
    switch (k) {
    case Coder::Png8:
    case Coder::Png16:
        png_wrap_stream(p.W, p.H, o.stream.ptr + 16, (size_t)len, tab, p.nbands, data, k == Coder::Png16 ? 16 : 8,
                        C == 4 ? 6 : C == 3 ? 2 : 0);
        break;
    case Coder::Exr:
    case Coder::Exr32:
        if (!exr_wrap_stream(p.W, p.H, o.stream.ptr + 16, (size_t)len, tab, p.nbands, data, k == Coder::Exr32 ? 2 : 1,
                             C))
            throw std::runtime_error("device EXR chunk table does not match its stream");
        break;
    default:
        throw std::runtime_error("not a deflate-coded frame");
    }
}

}  // namespace

void enqueue_coder(rr_ctx* c, const FrameOutput& fo, const CoderInput& in, DevFrame& f, hipStream_t st, CodedOut& o) {
    const Coder k = fo.coder;
    const int C = fo.color_mode;
    if (k == Coder::Jpeg) return enqueue_jpeg(c, in, C == RR_COLOR_BW, fo.quality, f, st, o.jpeg);
    if (device_body(k)) return enqueue_body(k, in, f, st, o.body);
    if (!device_deflate(k)) throw std::runtime_error("no device coder for this output");
    // the front ends' own buffers. "PNG" at compression 0 .. 100: a filter type
    // per row of the H rows, and at 16 bits the raw scanlines, 2C W H bytes
    // (less than the plan's stream, which is below 2 GB)
    const bool png = k == Coder::Png8 || k == Coder::Png16;
    const bool adaptive = png && fo.png_compression >= 0;
    Png16Front front{};
    if (k == Coder::Png16) {
        if (in.view_transform >= VIEW_FILMIC && !c->filmic.ready)
            throw std::runtime_error("Filmic view transform without LUTs");
        ensure_srgb16(c);
        front = Png16Front{in.film, in.inv_spp, in.exposure_scale, in.view_transform, c->srgb16_lut.ptr,
                           view_args(c, in.view_transform, in.look, in.gamma)};
    }
    if (adaptive) f.png_ftype.ensure((size_t)in.H);
    if (adaptive && k == Coder::Png16) f.png_raw.ensure((size_t)2 * (size_t)C * (size_t)in.W * (size_t)in.H);
    // the coder's scratch and its pinned outputs
    DeflateOut& d = o.deflate;
    const DeflatePlan& p = d.plan;
    f.deflate_scratch.ensure(deflate_scratch_words(p));
    d.stream.ensure((p.own_stream ? exr_stream_max_bytes(p) : deflate_stream_max_bytes(p)) + 32);
    d.tab.ensure((size_t)p.nbands * (p.own_stream ? 4 : 2) * sizeof(uint32_t));
    void *dev_host = nullptr, *dev_tab = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, d.stream.ptr, 0));
    RR_HIP(hipHostGetDevicePointer(&dev_tab, d.tab.ptr, 0));
    uint32_t* scratch = f.deflate_scratch.ptr;
    uint8_t* out = static_cast<uint8_t*>(dev_host);
    uint32_t* tab = static_cast<uint32_t*>(dev_tab);
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
        exr_encode_device(in.film, in.inv_spp, in.alpha_one, C, p, scratch, out, tab, st);
        break;
    default:  // Coder::Exr32: FLOAT channels
        exr32_encode_device(in.film, in.inv_spp, in.alpha_one, C, p, scratch, out, tab, st);
        break;
    }
    f.prof.end(st);
}

void coded_file_bytes(const CodedOut& o, const FrameOutput& fo, std::vector<uint8_t>& data) {
    if (fo.coder == Coder::Jpeg) jpeg_file_bytes(o.jpeg, data);
    else if (device_body(fo.coder)) body_file_bytes(o.body, fo.coder, data);
    else deflate_file_bytes(o.deflate, fo.coder, fo.color_mode, data);
}

int do_encode(const uint8_t* rgba, int W, int H, const char* out_path, const char* format, int quality,
              uint64_t* bytes, int mode, int compression) {
    if (!out_path || !format) return fail(RR_EINVAL, "out_path and format are required");
    const std::string fmt(format);
    std::vector<uint8_t> data;
    std::string ext;
    if (fmt == "JPEG") {
        if (quality < 1 || quality > 100) return fail(RR_EINVAL, "jpeg_quality must be 1..100");
        if (!encode_jpeg(rgba, W, H, quality, data, 0, resolve_color_mode(mode, true) == RR_COLOR_BW))
            return fail(RR_EINVAL, "JPEG encode failed");
        ext = ".jpg";
    } else if (fmt == "PNG") {
        const bool adaptive = compression >= 0;
        if (!encode_png(rgba, W, H, data, adaptive ? png_zlib_level(compression) : 1, 0, resolve_color_mode(mode, false),
                        adaptive))
            return fail(RR_EIO, "PNG encode failed");
        ext = ".png";
    } else if (fmt == "TARGA" || fmt == "TARGA_RAW") {
        if (!encode_tga(rgba, W, H, resolve_color_mode(mode, false), fmt == "TARGA", data))
            return fail(RR_EINVAL, "image size outside the TARGA format's range (65535 x 65535, a body below 2 GB)");
        ext = ".tga";
    } else if (fmt == "IRIS") {
        if (!encode_iris(rgba, W, H, resolve_color_mode(mode, false), data)) return fail(RR_EINVAL, kIrisRange);
        ext = ".rgb";
    } else if (fmt == "WEBP") {  // lossless at every quality: the caller flags one below 100
        if (!encode_webp(rgba, W, H, resolve_color_mode(mode, false), data)) return fail(RR_EINVAL, kWebpRange);
        ext = ".webp";
    } else if (fmt == "OPEN_EXR" || fmt == "HDR") {
        return fail(RR_ENOTSUP, "unsupported output format '" + fmt +
                                    "' for an RGBA8 image: it needs the float film (JPEG, PNG, TARGA, TARGA_RAW, "
                                    "IRIS and WEBP are supported here)");
    } else {
        return fail(RR_ENOTSUP, "unsupported output format '" + fmt +
                                    "' (JPEG, PNG, TARGA, TARGA_RAW, IRIS and WEBP are supported here; OPEN_EXR and "
                                    "HDR need the float film)");
    }
    const std::string path = std::string(out_path) + ext;
    if (!write_file(path, data)) return fail(RR_EIO, "cannot write " + path + ": " + std::strerror(errno));
    if (bytes) *bytes = data.size();
    return RR_OK;
}

}  // namespace rr
