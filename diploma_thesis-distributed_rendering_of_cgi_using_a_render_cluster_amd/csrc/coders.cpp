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

int plan_or_refuse(const FrameOutput& fo, int W, int H, TgaPlan& p) {
    if (tga_plan(W, H, fo.color_mode, !fo.tga_raw, p)) return RR_OK;
    return fail(RR_EINVAL, "image size outside the TARGA format's range (65535 x 65535, a body below 2 GB)");
}

int plan_or_refuse(const FrameOutput& fo, int W, int H, HdrPlan& p) {
    if (hdr_plan(W, H, fo.color_mode, p)) return RR_OK;
    return fail(RR_EINVAL, "image size outside the HDR coder's range (a body bound below 2 GB)");
}

static const char* const kIrisRange =
    "image size outside the IRIS format's range (65535 x 65535, a body bound below 2 GB)";

int plan_or_refuse(const FrameOutput& fo, int W, int H, IrisPlan& p) {
    if (iris_plan(W, H, fo.color_mode, p)) return RR_OK;
    return fail(RR_EINVAL, kIrisRange);
}

static const char* const kWebpRange =
    "image size outside the WEBP format's range (16384 x 16384, a payload bound below 2 GB)";

int plan_or_refuse(const FrameOutput& fo, int W, int H, WebpPlan& p) {
    if (webp_plan(W, H, fo.color_mode, p)) return RR_OK;
    return fail(RR_EINVAL, kWebpRange);
}

std::string webp_quality_warning(int quality) {
    if (quality >= 100) return "";
    return "WEBP at quality " + std::to_string(quality) +
           ": lossy WEBP is not built, the file is lossless (as at quality 100)";
}

namespace {

// Device WEBP encode of an RGBA8 image into o's pinned stream, by o.plan.
void enqueue_webp(const CoderInput& in, DevFrame& f, hipStream_t st, WebpOut& o) {
    const WebpPlan& p = o.plan;
    if (p.W != in.W || p.H != in.H) throw std::runtime_error("WEBP plan of another image");
    f.webp_scratch.ensure(webp_scratch_words(p));
    o.stream.ensure(webp_stream_bytes(p));
    void* dev_host = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, o.stream.ptr, 0));
    f.prof.begin(st, RR_K_PNG);
    webp_encode_device(in.rgba8, p, f.webp_scratch.ptr, static_cast<uint8_t*>(dev_host), st);
    f.prof.end(st);
}

// The file of a device-coded WEBP image: the host-built RIFF and chunk headers
// around the device's payload (at least the 5 bytes of signature and sizes).
void webp_file_bytes(const WebpOut& o, std::vector<uint8_t>& data) {
    const WebpPlan& p = o.plan;
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    if (len > p.body_cap || len + 16 > o.stream.cap || len < 5) throw std::runtime_error("device WEBP stream overflow");
    webp_wrap_stream(o.stream.ptr + 16, (size_t)len, data);
}

// Device IRIS encode of an RGBA8 image into o's pinned stream, by o.plan.
void enqueue_iris(const CoderInput& in, DevFrame& f, hipStream_t st, IrisOut& o) {
    const IrisPlan& p = o.plan;
    if (p.W != in.W || p.H != in.H) throw std::runtime_error("IRIS plan of another image");
    f.iris_scratch.ensure(iris_scratch_words(p));
    o.stream.ensure(iris_stream_bytes(p));
    void* dev_host = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, o.stream.ptr, 0));
    f.prof.begin(st, RR_K_PNG);
    iris_encode_device(in.rgba8, p, f.iris_scratch.ptr, static_cast<uint8_t*>(dev_host), st);
    f.prof.end(st);
}

// The file of a device-coded IRIS image: host-built header + the device body
// (the tables and the coded row-planes, each at least its terminator).
void iris_file_bytes(const IrisOut& o, std::vector<uint8_t>& data) {
    const IrisPlan& p = o.plan;
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    const uint64_t planes = (uint64_t)p.H * (uint64_t)p.C;
    if (len > p.body_cap || len + 16 > o.stream.cap || len < 8 * planes + 3 * planes)
        throw std::runtime_error("device IRIS stream overflow");
    iris_header_bytes(p.W, p.H, p.C, data);
    data.insert(data.end(), o.stream.ptr + 16, o.stream.ptr + 16 + len);
}

// Device HDR encode of a film into o's pinned stream, by o.plan.
void enqueue_hdr(const CoderInput& in, DevFrame& f, hipStream_t st, HdrOut& o) {
    const HdrPlan& p = o.plan;
    if (p.W != in.W || p.H != in.H) throw std::runtime_error("HDR plan of another image");
    f.hdr_scratch.ensure(hdr_scratch_words(p));
    o.stream.ensure(hdr_stream_bytes(p));
    void* dev_host = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, o.stream.ptr, 0));
    f.prof.begin(st, RR_K_PNG);
    hdr_encode_device(in.film, in.inv_spp, p, f.hdr_scratch.ptr, static_cast<uint8_t*>(dev_host), st);
    f.prof.end(st);
}

// The file of a device-coded HDR image: host-built header + the device body.
void hdr_file_bytes(const HdrOut& o, std::vector<uint8_t>& data) {
    const HdrPlan& p = o.plan;
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    if (len > p.body_cap || len + 16 > o.stream.cap || (p.flat && len != p.body_cap))
        throw std::runtime_error("device HDR stream overflow");
    hdr_header_bytes(p.W, p.H, data);
    data.insert(data.end(), o.stream.ptr + 16, o.stream.ptr + 16 + len);
}

// Device TARGA encode of an RGBA8 image into o's pinned stream, by o.plan.
void enqueue_tga(const CoderInput& in, DevFrame& f, hipStream_t st, TgaOut& o) {
    const TgaPlan& p = o.plan;
    if (p.W != in.W || p.H != in.H) throw std::runtime_error("TARGA plan of another image");
    f.tga_scratch.ensure(tga_scratch_words(p));
    o.stream.ensure(tga_stream_bytes(p));
    void* dev_host = nullptr;
    RR_HIP(hipHostGetDevicePointer(&dev_host, o.stream.ptr, 0));
    f.prof.begin(st, RR_K_PNG);
    tga_encode_device(in.rgba8, p, f.tga_scratch.ptr, static_cast<uint8_t*>(dev_host), st);
    f.prof.end(st);
}

// The file of a device-coded TARGA image: host-built header + the device body.
void tga_file_bytes(const TgaOut& o, std::vector<uint8_t>& data) {
    const TgaPlan& p = o.plan;
    uint64_t len = 0;
    std::memcpy(&len, o.stream.ptr, sizeof len);
    if (len > p.body_cap || len + 16 > o.stream.cap || (!p.rle && len != p.body_cap))
        throw std::runtime_error("device TARGA stream overflow");
    tga_header_bytes(p.W, p.H, p.C, p.rle, data);
    data.insert(data.end(), o.stream.ptr + 16, o.stream.ptr + 16 + len);
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
    if (k == Coder::Tga) return enqueue_tga(in, f, st, o.tga);
    if (k == Coder::Hdr) return enqueue_hdr(in, f, st, o.hdr);
    if (k == Coder::Iris) return enqueue_iris(in, f, st, o.iris);
    if (k == Coder::Webp) return enqueue_webp(in, f, st, o.webp);
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
    else if (fo.coder == Coder::Tga) tga_file_bytes(o.tga, data);
    else if (fo.coder == Coder::Hdr) hdr_file_bytes(o.hdr, data);
    else if (fo.coder == Coder::Iris) iris_file_bytes(o.iris, data);
    else if (fo.coder == Coder::Webp) webp_file_bytes(o.webp, data);
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
