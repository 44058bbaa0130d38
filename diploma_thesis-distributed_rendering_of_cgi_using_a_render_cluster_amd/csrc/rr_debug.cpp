// The inspection entry points of the C ABI (include/rr.h rr_debug_*): the
// tests' and tools' view into the scene, the hierarchy builds, the traversal
// and the device coders. They work on the context's home stream with its home
// frame state and coder outputs, with no frame pending (RR_EBUSY otherwise),
// and change nothing of a frame slot.
#include <algorithm>
#include <cstring>

#include "api_util.hpp"
#include "frame.hpp"
#include "image_io.hpp"
#include "png_filter.h"
#include "pxr24_rule.h"

using namespace rr;

namespace {

// The view settings of an inspection call on c with a view of the caller's:
// the context's look (with the Filmic view) and display gamma, None and 1
// where the context leaves them to a scene. Nothing is substituted here: a
// view or look whose LUT is not loaded is RR_EINVAL.
int debug_view_settings(const rr_ctx* c, int view, int& look, float& gamma) {
    if (view < VIEW_STANDARD || view > VIEW_FALSE_COLOR) return fail(RR_EINVAL, "unsupported view transform");
    if (view >= VIEW_FILMIC && !c->filmic.ready)
        return fail(RR_EINVAL, "Filmic view transform without LUTs (rr_set_ocio_config / RR_OCIO_DIR)");
    if (view == VIEW_FALSE_COLOR && !c->filmic.has_false_color())
        return fail(RR_EINVAL, std::string("False Color view transform without ") + kFalseColorFile);
    look = (view == VIEW_FILMIC && c->settings.look > 0) ? c->settings.look : 0;
    if (look && !c->filmic.has_look(look))
        return fail(RR_EINVAL, std::string("look '") + kLooks[look].name + "' without " + kLooks[look].file);
    gamma = c->settings.gamma != 0.f ? c->settings.gamma : 1.f;
    return RR_OK;
}

// The body of the coders' entry points: a w x h image of the caller's (RGBA8,
// or float RGBA means for a coder of the film, CoderInfo::film) through coder k in C
// channels, with the context's PNG compression; the file's bytes to `out` if
// `cap` suffices. alpha_one, view_transform, exposure_scale: CoderInput's.
// exr_codec: FrameOutput's (rr_debug_encode_device: the context's).
int debug_encode(rr_ctx* c, Coder k, int C, const void* image, int w, int h, bool alpha_one, int view_transform,
                 float exposure_scale, int quality, uint8_t* out, uint64_t cap, uint64_t* len, bool tga_raw = false,
                 int exr_codec = RR_EXR_CODEC_ZIP) {
    CoderInput in;
    in.W = w;
    in.H = h;
    in.alpha_one = alpha_one;
    in.exposure_scale = exposure_scale;
    in.view_transform = view_transform;
    if (k == Coder::Png16)
        if (const int rc = debug_view_settings(c, view_transform, in.look, in.gamma)) return rc;
    const FrameOutput fo{k, C, png_compression_of(c->settings), quality, tga_raw, exr_codec};
    if (const int rc = plan_or_refuse(fo, w, h, c->home_coded)) return rc;
    if (k == Coder::Webp) c->frame_warning = webp_quality_warning(quality);  // flagged as a frame's file is
    if ((k == Coder::Exr || k == Coder::Exr32) && exr_codec != RR_EXR_CODEC_ZIP) c->frame_warning = exr_codec_warning(fo);
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        set_device(c);
        const size_t bytes = (size_t)w * h * (coder_info(k).film ? sizeof(float4) : 4);
        DevBuf<uint8_t> img;
        img.ensure(bytes);
        RR_HIP(hipMemcpy(img.ptr, image, bytes, hipMemcpyHostToDevice));
        in.rgba8 = img.ptr;
        in.film = reinterpret_cast<const float4*>(img.ptr);
        if (k == Coder::Jpeg) in.jpeg_tab = jpeg_table(c, quality);
        enqueue_coder(c, fo, in, c->home, c->stream, c->home_coded);
        RR_HIP(hipStreamSynchronize(c->stream));
        std::vector<uint8_t> data;
        coded_file_bytes(c->home_coded, fo, data);
        *len = data.size();
        if (out && cap >= *len) std::memcpy(out, data.data(), data.size());
        return RR_OK;
    });
}

}  // namespace

extern "C" {

int rr_debug_jpeg_device(rr_ctx* c, const uint8_t* rgba8, int32_t w, int32_t h, int32_t quality, uint8_t* out,
                         uint64_t cap, uint64_t* len) {
    if (!c || !rgba8 || !len || w <= 0 || h <= 0 || w > 65535 || h > 65535) return fail(RR_EINVAL, "bad arguments");
    if (quality < 1 || quality > 100) return fail(RR_EINVAL, "jpeg_quality must be 1..100");
    return debug_encode(c, Coder::Jpeg, RR_COLOR_RGB, rgba8, w, h, true, VIEW_STANDARD, 1.0f, quality, out, cap, len);
}

int rr_debug_png_device(rr_ctx* c, const uint8_t* rgba8, int32_t w, int32_t h, uint8_t* out, uint64_t cap,
                        uint64_t* len) {
    if (!c || !rgba8 || !len || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    return debug_encode(c, Coder::Png8, 4, rgba8, w, h, true, VIEW_STANDARD, 1.0f, 0, out, cap, len);
}

// (rr_debug_exr_device and rr_debug_exr32_device write the image's own alpha;
// rr_debug_encode_device A = 1, as in a rendered frame's file)
int rr_debug_exr_device(rr_ctx* c, const float* rgba, int32_t w, int32_t h, uint8_t* out, uint64_t cap,
                        uint64_t* len) {
    if (!c || !rgba || !len || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    return debug_encode(c, Coder::Exr, 4, rgba, w, h, false, VIEW_STANDARD, 1.0f, 0, out, cap, len);
}

int rr_debug_exr32_device(rr_ctx* c, const float* rgba, int32_t w, int32_t h, uint8_t* out, uint64_t cap,
                          uint64_t* len) {
    if (!c || !rgba || !len || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    return debug_encode(c, Coder::Exr32, 4, rgba, w, h, false, VIEW_STANDARD, 1.0f, 0, out, cap, len);
}

int rr_debug_png16_device(rr_ctx* c, const float* rgba, int32_t w, int32_t h, int32_t view_transform,
                          float exposure_scale, uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!c || !rgba || !len || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    return debug_encode(c, Coder::Png16, 4, rgba, w, h, true, view_transform, exposure_scale, 0, out, cap, len);
}

int rr_debug_encode_device(rr_ctx* c, const char* format, int32_t depth, int32_t color_mode, const void* image,
                           int32_t image_is_float, int32_t w, int32_t h, int32_t view_transform, float exposure_scale,
                           int32_t jpeg_quality, uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!c || !format || !image || !len || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    if (!valid_color_mode(color_mode)) return fail(RR_EINVAL, "bad colour mode");
    const Format* f = find_format(format);
    const int C = resolve_color_mode(color_mode, f && f->no_alpha);
    // A format of one coder takes that coder's image at its depth. Where the depth chooses the coder, a depth
    // that is no coder's names none, as an unknown format does: both are asked for a float image, then refused.
    const bool fixed = f && !f->deep_depth;
    Coder k = f ? format_coder(*f, depth) : Coder::None;
    const bool depth_ok = depth == 0 || depth == coder_info(k).depth;
    if (!fixed && !depth_ok) k = Coder::None;
    const CoderInfo& ci = coder_info(k);
    const bool film = k == Coder::None || ci.film;
    if ((image_is_float != 0) != film || (fixed && !depth_ok)) {
        const std::string image = film ? "a float RGBA image" : "an RGBA8 image";
        if (fixed) return fail(RR_EINVAL, ci.name + (" takes " + image) + " at depth " + std::to_string(ci.depth));
        return fail(RR_EINVAL, film ? "16-bit PNG and OPEN_EXR take " + image : "8-bit PNG takes " + image);
    }
    if (k == Coder::None)
        return fail(RR_EINVAL, std::string("no such format and depth: '") + format + "' at " + std::to_string(depth));
    if (k == Coder::Jpeg) {
        if (w > 65535 || h > 65535) return fail(RR_EINVAL, ci.range);
        if (jpeg_quality < 1 || jpeg_quality > 100) return fail(RR_EINVAL, "jpeg_quality must be 1..100");
    }
    // (WEBP: a jpeg_quality below 100 is flagged, rr_last_warning, the file lossless)
    return debug_encode(c, k, C, image, w, h, true, view_transform, exposure_scale, jpeg_quality, out, cap, len,
                        f->tga_raw, exr_codec_of(c->settings));
}

int rr_debug_hdr_host(const float* rgba, int32_t w, int32_t h, int32_t color_mode, uint8_t* out, uint64_t cap,
                      uint64_t* bytes) {
    if (!rgba || !bytes || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    if (!valid_color_mode(color_mode)) return fail(RR_EINVAL, "bad colour mode");
    return guarded([&] {
        std::vector<uint8_t> data;
        if (!encode_hdr(rgba, w, h, resolve_color_mode(color_mode, true), data))
            return fail(RR_EINVAL, coder_info(Coder::Hdr).range);
        *bytes = data.size();
        if (out && cap >= *bytes) std::memcpy(out, data.data(), data.size());
        return RR_OK;
    });
}

int rr_debug_png_filters(const uint8_t* raw, int32_t row_bytes, int32_t rows, int32_t bpp, uint8_t* types) {
    if (!raw || !types || row_bytes <= 0 || rows <= 0 || bpp < 1 || bpp > 8) return fail(RR_EINVAL, "bad arguments");
    for (int32_t y = 0; y < rows; ++y) {
        const uint8_t* cur = raw + (size_t)y * (size_t)row_bytes;
        types[y] = (uint8_t)png_pick_row(cur, y ? cur - row_bytes : nullptr, (size_t)row_bytes, (size_t)bpp, (size_t)rows);
    }
    return RR_OK;
}

int rr_debug_scene_png_compression(rr_scene* s, int32_t* compression) {
    if (!s || !compression) return fail(RR_EINVAL, "NULL argument");
    *compression = s->desc.render.png_compression;
    return RR_OK;
}

int rr_debug_scene_exr_codec(rr_scene* s, int32_t* codec) {
    if (!s || !codec) return fail(RR_EINVAL, "NULL argument");
    *codec = s->desc.render.exr_codec;
    return RR_OK;
}

int rr_debug_float24(const float* in, uint64_t n, uint32_t* out) {
    if ((!in || !out) && n) return fail(RR_EINVAL, "NULL array");
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t bits;
        std::memcpy(&bits, in + i, 4);
        out[i] = float24_bits(bits);
    }
    return RR_OK;
}

int rr_debug_exr_rle(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!in || !len || !n) return fail(RR_EINVAL, "bad arguments");
    return guarded([&] {
        std::vector<uint8_t> data;
        exr_rle_pack(in, (size_t)n, data);
        *len = data.size();
        if (out && cap >= *len) std::memcpy(out, data.data(), data.size());
        return RR_OK;
    });
}

int rr_debug_sin_fixed(const float* in, uint64_t n, float* out) {
    if ((!in || !out) && n) return fail(RR_EINVAL, "NULL array");
    sin_fixed_host(in, (size_t)n, out);
    return RR_OK;
}

int rr_debug_dither_noise(int32_t w, int32_t h, float* out) {
    if (!out || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    dither_noise_host(w, h, out);
    return RR_OK;
}

int rr_debug_view_device(rr_ctx* c, const float* rgba, int32_t w, int32_t h, int32_t view_transform,
                         float exposure_scale, uint8_t* rgba8_out) {
    if (!c || !rgba || !rgba8_out || w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)1 << 28)
        return fail(RR_EINVAL, "bad arguments");
    int look = 0;
    float gamma = 1.f;
    if (const int rc = debug_view_settings(c, view_transform, look, gamma)) return rc;
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        set_device(c);
        const size_t npix = (size_t)w * h;
        ensure_srgb(c);
        DevBuf<float4> img;
        DevBuf<uchar4> q;
        img.ensure(npix);
        q.ensure(npix);
        RR_HIP(hipMemcpy(img.ptr, rgba, npix * sizeof(float4), hipMemcpyHostToDevice));
        FrameConsts k{};
        k.W = w;
        k.H = h;
        k.npix = (int)npix;
        k.inv_spp = 1.0f;
        k.exposure_scale = exposure_scale;
        k.view_transform = view_transform;
        k.div_w = FastDiv::make((uint32_t)w);
        view_device(view_args(c, view_transform, look, gamma, dither_of(c->settings)), k, c->paths.srgb_lut.ptr,
                    img.ptr, q.ptr, c->stream);
        RR_HIP(hipStreamSynchronize(c->stream));
        RR_HIP(hipMemcpy(rgba8_out, q.ptr, npix * 4, hipMemcpyDeviceToHost));
        return RR_OK;
    });
}

int rr_debug_display_gamma(const float* in, uint64_t n, float gamma, float* out) {
    if ((!in || !out) && n) return fail(RR_EINVAL, "NULL array");
    if (!(gamma > 0.f) || gamma > kGammaMax) return fail(RR_EINVAL, "display gamma must be above 0 and at most 5");
    display_gamma_host(in, (size_t)n, gamma, out);
    return RR_OK;
}

int rr_debug_scene_view(rr_scene* s, int32_t* view_transform, char* look, int32_t cap, float* gamma) {
    if (!s) return fail(RR_EINVAL, "scene is NULL");
    const RenderDesc& r = s->desc.render;
    if (view_transform) *view_transform = r.view_transform;
    const char* name = kLooks[r.look].name;
    if (look && cap > (int32_t)std::strlen(name)) std::strcpy(look, name);
    if (gamma) *gamma = (float)r.gamma;
    return RR_OK;
}

int rr_debug_srgb16_table(float* table, int32_t cap, int32_t* n) {
    if (!n) return fail(RR_EINVAL, "n is NULL");
    *n = kSrgb16LutSize + 1;
    if (table && cap >= *n) {
        std::vector<float> lut(kSrgb16LutSize + 2);
        build_srgb16_lut(lut.data());
        std::memcpy(table, lut.data(), (size_t)*n * sizeof(float));
    }
    return RR_OK;
}

int rr_debug_scene_mesh(rr_scene* s, float* tri_local9, int32_t* tri_object) {
    if (!s) return fail(RR_EINVAL, "scene is NULL");
    const size_t n = s->desc.tri_obj.size();
    if (tri_local9)
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) tri_local9[9 * i + 3 * k + a] = s->desc.tri_local[12 * i + 4 * k + a];
    if (tri_object && n) std::memcpy(tri_object, s->desc.tri_obj.data(), n * sizeof(int32_t));
    return RR_OK;
}

int rr_debug_counts(rr_scene* s, int32_t* nt, int32_t* nl, int32_t* nm, int32_t* no) {
    if (!s) return fail(RR_EINVAL, "scene is NULL");
    int lights = 0;
    for (auto& o : s->desc.objects) lights += o.type == OBJ_LIGHT;
    if (nt) *nt = (int32_t)s->desc.tri_obj.size();
    if (nl) *nl = lights;
    if (nm) *nm = (int32_t)s->desc.materials.size();
    if (no) *no = (int32_t)s->desc.objects.size();
    return RR_OK;
}

int rr_debug_frame_state(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params, float* tris_world,
                         int32_t* tri_material, float* camera, float* lights, float* materials, float* world,
                         int32_t* render_ints, float* render_floats) {
    if (!s) return fail(RR_EINVAL, "NULL scene");
    if (!c && tris_world) return fail(RR_EINVAL, "world triangles need a device context");
    return guarded([&] {
        FrameSetup fs = setup_frame(s->desc, frame, params);
        if (c) resolve_view(c, fs);  // render_ints[5]: the transform a frame on c is rendered with
        const int n = s->mesh.n_tris;
        if (c) {  // host-only queries (c == NULL) skip the device part
            if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
            set_device(c);
            PinnedBuf staging;
            prepare_frame(c, s, s->build, c->home, c->stream, fs, staging);
            RR_HIP(hipStreamSynchronize(c->stream));
        }
        if (tris_world && n > 0) {
            std::vector<float4> w((size_t)3 * n);
            RR_HIP(hipMemcpyAsync(w.data(), s->build.tri_world.ptr, w.size() * sizeof(float4), hipMemcpyDeviceToHost,
                                  c->stream));
            RR_HIP(hipStreamSynchronize(c->stream));
            for (size_t i = 0; i < w.size(); ++i) {
                tris_world[3 * i] = w[i].x;
                tris_world[3 * i + 1] = w[i].y;
                tris_world[3 * i + 2] = w[i].z;
            }
        }
        if (tri_material) std::memcpy(tri_material, s->desc.tri_mat.data(), n * sizeof(int32_t));
        if (camera) std::memcpy(camera, fs.cam, sizeof fs.cam);
        if (lights && !fs.lights.empty()) std::memcpy(lights, fs.lights.data(), fs.lights.size() * sizeof(float));
        if (materials) std::memcpy(materials, fs.materials.data(), fs.materials.size() * sizeof(float));
        if (world) std::memcpy(world, fs.world, sizeof fs.world);
        if (render_ints) {
            const int32_t ri[RR_RENDER_INTS] = {fs.W, fs.H, fs.spp, fs.max_bounces, (int32_t)fs.seed,
                                               fs.view_transform, choose_spp_chunk(fs), frame_hier(fs, n),
                                               fs.max_diffuse, fs.max_glossy};
            std::memcpy(render_ints, ri, sizeof ri);
        }
        if (render_floats) {
            const float rf[RR_RENDER_FLOATS] = {fs.clamp_indirect, fs.filter_width, fs.exposure_scale, 0.f};
            std::memcpy(render_floats, rf, sizeof rf);
        }
        return RR_OK;
    });
}

int rr_debug_bvh(rr_ctx* c, rr_scene* s, int32_t frame, uint32_t* keys, uint32_t* order, int32_t* children,
                 float* boxes) {
    return rr_debug_bvh_hier(c, s, frame, 0, keys, order, children, boxes);
}

int rr_debug_bvh_hier(rr_ctx* c, rr_scene* s, int32_t frame, int32_t hier, uint32_t* keys, uint32_t* order,
                      int32_t* children, float* boxes) {
    if (!c || !s) return fail(RR_EINVAL, "NULL ctx or scene");
    if (hier != 0 && hier != kHierLbvh && hier != kHierPloc) return fail(RR_EINVAL, "hier must be 0, 2 or 3");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        FrameSetup fs = setup_frame(s->desc, frame, nullptr);
        set_device(c);
        PinnedBuf staging;
        prepare_frame(c, s, s->build, c->home, c->stream, fs, staging, hier);
        const DevBuild& d = s->build;
        const int n = s->mesh.n_tris;
        hipStream_t st = c->stream;
        const int ni = n > 1 ? n - 1 : n;  // a single triangle has one (leaf-only) node
        std::vector<BvhNode> nodes((size_t)ni);
        if (n > 0) {
            if (keys) RR_HIP(hipMemcpyAsync(keys, d.keys[0].ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            if (order) RR_HIP(hipMemcpyAsync(order, d.vals[0].ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            RR_HIP(hipMemcpyAsync(nodes.data(), d.nodes.ptr, ni * sizeof(BvhNode), hipMemcpyDeviceToHost, st));
        }
        RR_HIP(hipStreamSynchronize(st));  // also for an empty scene: prepare_frame's uploads read `staging`
        for (int i = 0; i < ni; ++i) {
            const float* f = reinterpret_cast<const float*>(&nodes[i]);
            if (boxes) std::memcpy(boxes + 12 * i, f, 12 * sizeof(float));
            if (children) {
                children[2 * i] = nodes[i].d.x;
                children[2 * i + 1] = nodes[i].d.y;
            }
        }
        return RR_OK;
    });
}

int rr_debug_qbvh(rr_ctx* c, rr_scene* s, int32_t frame, int32_t* nq, int32_t* children, uint32_t* nodes16,
                  int32_t* tri_orig) {
    if (!c || !s || !nq) return fail(RR_EINVAL, "NULL ctx, scene or nq");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        FrameSetup fs = setup_frame(s->desc, frame, nullptr);
        set_device(c);
        PinnedBuf staging;
        prepare_frame(c, s, s->build, c->home, c->stream, fs, staging, kHierQWide);
        const DevBuild& d = s->build;
        hipStream_t st = c->stream;
        const int n = s->mesh.n_tris;
        *nq = 0;
        if (n > 0) {
            const uint32_t cnt = (uint32_t)d.nq;
            *nq = (int32_t)cnt;
            if (children || nodes16) {
                std::vector<QNode6> nodes(cnt);
                RR_HIP(hipMemcpyAsync(nodes.data(), d.qnodes.ptr, cnt * sizeof(QNode6), hipMemcpyDeviceToHost, st));
                RR_HIP(hipStreamSynchronize(st));
                for (uint32_t i = 0; i < cnt; ++i) {
                    const QNode6& q = nodes[i];
                    if (children) {  // the implicit references, spelled out (unused slots: 0x7fffffff)
                        const uint32_t eb = (uint32_t)f2i(q.org.w);
                        for (int k = 0; k < kQWidth; ++k) {
                            const uint32_t lox = k < 4 ? (q.a.z >> (8 * k)) & 255u : (q.c.x >> (8 * (k - 4))) & 255u;
                            const uint32_t hix = k < 4 ? (q.b.y >> (8 * k)) & 255u : (q.c.y >> (16 + 8 * (k - 4))) & 255u;
                            const bool unused = lox == 255u && hix == 0u && !((eb >> (24 + k)) & 1u);
                            children[kQWidth * (size_t)i + k] = unused ? 0x7fffffff : q6_ref(q, k);
                        }
                    }
                    if (nodes16) std::memcpy(nodes16 + 16 * (size_t)i, &q, sizeof(QNode6));
                }
            }
            if (tri_orig) {  // original id of each position of the hierarchy's triangle array
                std::vector<TriPack> tp((size_t)n);
                RR_HIP(hipMemcpyAsync(tp.data(), d.tris.ptr, (size_t)n * sizeof(TriPack), hipMemcpyDeviceToHost, st));
                RR_HIP(hipStreamSynchronize(st));
                for (int i = 0; i < n; ++i) tri_orig[i] = f2i(tp[(size_t)i].p0.w);
            }
        }
        return RR_OK;
    });
}

int rr_debug_trace(rr_ctx* c, rr_scene* s, int32_t frame, int32_t bvh_width, int32_t n, const float* rays,
                   float* hits, int32_t* prims, uint8_t* occluded) {
    if (!c || !s || n < 0 || (n > 0 && !rays)) return fail(RR_EINVAL, "bad arguments");
    if (bvh_width < 0 || bvh_width == 1 || bvh_width > 7)
        return fail(RR_EINVAL, "hierarchy must be 0 (frame's), 2 (LBVH), 3 (PLOC), 4 (6-wide), 5 (6-wide, packets) "
                               "6 (6-wide, one LDS stack entry) or 7 (6-wide, beam packets)");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        FrameSetup fs = setup_frame(s->desc, frame, nullptr);
        set_device(c);
        PinnedBuf staging;
        const int hier = bvh_width >= 5 ? kHierQWide : (bvh_width ? bvh_width : frame_hier(fs, s->mesh.n_tris));
        prepare_frame(c, s, s->build, c->home, c->stream, fs, staging, hier);
        const int width = bvh_width >= 5 ? bvh_width : (hier == kHierQWide ? 4 : 2);
        hipStream_t st = c->stream;
        DevBuf<float4> dr, dh;
        DevBuf<int32_t> dp;
        DevBuf<uint8_t> dq;
        const size_t m = n > 0 ? (size_t)n : 1;
        dr.ensure(2 * m);
        dh.ensure(m);
        dp.ensure(m);
        dq.ensure(m);
        if (n > 0) RR_HIP(hipMemcpyAsync(dr.ptr, rays, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice, st));
        trace_batch_device(s->mesh, s->build, c->paths, c->home, n, dr.ptr, dh.ptr, dp.ptr, dq.ptr, st, width);
        std::vector<float4> h(m);
        if (n > 0) {
            RR_HIP(hipMemcpyAsync(h.data(), dh.ptr, n * sizeof(float4), hipMemcpyDeviceToHost, st));
            if (prims) RR_HIP(hipMemcpyAsync(prims, dp.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            if (occluded) RR_HIP(hipMemcpyAsync(occluded, dq.ptr, n, hipMemcpyDeviceToHost, st));
        }
        RR_HIP(hipStreamSynchronize(st));
        if (hits)
            for (int i = 0; i < n; ++i) {
                hits[4 * i] = h[i].x;
                hits[4 * i + 1] = h[i].y;
                hits[4 * i + 2] = h[i].z;
                hits[4 * i + 3] = 0.0f;
            }
        return RR_OK;
    });
}

int rr_debug_tile_costs(rr_ctx* c, int32_t capacity, uint32_t* costs, int32_t* order, int32_t* n_tiles,
                        uint64_t* unit_log, int32_t unit_capacity) {
    if (!c || capacity < 0 || !n_tiles || (capacity > 0 && (!costs || !order)) || unit_capacity < 0 ||
        (unit_capacity > 0 && !unit_log))
        return fail(RR_EINVAL, "bad arguments");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        *n_tiles = 0;
        const FrameSlot* sl = c->last_enqueued;
        if (!sl || !sl->tiles) return RR_OK;  // no tile frame yet
        set_device(c);
        const DevFrame& f = sl->dev;
        const size_t n = std::min(f.tile_cost.cap, f.tile_order.cap);
        *n_tiles = (int32_t)n;
        const size_t m = std::min<size_t>(n, (size_t)capacity);
        if (m > 0) {
            // the cost buffer is longer than the order's: behind the frame's tile costs it holds, per tile, the
            // samples a counting launch's covered body ran (tiles.hip); a caller with room gets those words too
            const size_t mc = std::min<size_t>(f.tile_cost.cap, (size_t)capacity);
            RR_HIP(hipMemcpy(costs, f.tile_cost.ptr, mc * sizeof(uint32_t), hipMemcpyDeviceToHost));
            RR_HIP(hipMemcpy(order, f.tile_order.ptr, m * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        const size_t nu = std::min<size_t>((size_t)unit_capacity, kUnitLog);
        if (nu > 0) {
            std::memset(unit_log, 0, 2 * nu * sizeof(uint64_t));
            // only the launch that wrote it (a counting frame): an older frame's log stays unreported
            if (f.unit_logged && f.trav_counts.cap >= (size_t)(kTravWords + 2 * kUnitLog))
                RR_HIP(hipMemcpy(unit_log, f.trav_counts.ptr + kTravWords, 2 * nu * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost));
        }
        return RR_OK;
    });
}

int rr_debug_fastmath_check(rr_ctx* c, uint32_t lo, uint64_t n, uint64_t* counts5) {
    if (!c || !counts5 || n > (1ull << 32) - lo) return fail(RR_EINVAL, "bad arguments");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        set_device(c);
        hipStream_t st = c->stream;
        DevBuf<unsigned long long> d;
        d.ensure(5);
        fastmath_check_device(lo, n, d.ptr, st);
        RR_HIP(hipMemcpyAsync(counts5, d.ptr, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        RR_HIP(hipStreamSynchronize(st));
        return RR_OK;
    });
}

int rr_debug_bsdf_sample(rr_ctx* c, const float* mat12, const float* n3, const float* wo3, int32_t n,
                         const float* u, float* wi3, float* f3, float* pdf, int32_t* ok) {
    if (!c || !mat12 || !n3 || !wo3 || n < 0 || (n > 0 && (!u || !wi3 || !f3 || !pdf || !ok)))
        return fail(RR_EINVAL, "bad arguments");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        set_device(c);
        hipStream_t st = c->stream;
        const size_t m = n > 0 ? (size_t)n : 1;
        DevBuf<float> dm, du, dw, df, dp, dl;
        DevBuf<int32_t> dk;
        float lut[kMatLutFloatsPerMat];
        build_material_lut(mat12, lut);
        dl.ensure(kMatLutFloatsPerMat);
        RR_HIP(hipMemcpyAsync(dl.ptr, lut, sizeof lut, hipMemcpyHostToDevice, st));
        dm.ensure(RR_MAT_FLOATS);
        du.ensure(3 * m); dw.ensure(3 * m); df.ensure(3 * m); dp.ensure(m); dk.ensure(m);
        RR_HIP(hipMemcpyAsync(dm.ptr, mat12, RR_MAT_FLOATS * sizeof(float), hipMemcpyHostToDevice, st));
        if (n > 0) RR_HIP(hipMemcpyAsync(du.ptr, u, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
        bsdf_batch_device(dm.ptr, dl.ptr, n3, wo3, n, du.ptr, dw.ptr, df.ptr, dp.ptr, dk.ptr, st);
        if (n > 0) {
            RR_HIP(hipMemcpyAsync(wi3, dw.ptr, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
            RR_HIP(hipMemcpyAsync(f3, df.ptr, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
            RR_HIP(hipMemcpyAsync(pdf, dp.ptr, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
            RR_HIP(hipMemcpyAsync(ok, dk.ptr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        RR_HIP(hipStreamSynchronize(st));
        return RR_OK;
    });
}

int rr_debug_film_reduce(rr_ctx* c, const float* rgba, int32_t w, int32_t h, int32_t reduce, float* out) {
    if (!rgba || !out || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    if (!reduce_factor_valid(reduce)) return fail(RR_EINVAL, "reduce must be 1, 2, 4 or 8");
    return guarded([&] {
        if (!c) {  // the rule as the host states it
            film_reduce_host(rgba, w, h, reduce, out);
            return RR_OK;
        }
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        set_device(c);
        hipStream_t st = c->stream;
        const size_t n_in = (size_t)w * h, n_out = (size_t)reduced_size(w, reduce) * reduced_size(h, reduce);
        DevBuf<float4> in, red;
        in.ensure(n_in);
        red.ensure(n_out);
        RR_HIP(hipMemcpyAsync(in.ptr, rgba, n_in * sizeof(float4), hipMemcpyHostToDevice, st));
        film_reduce_device(in.ptr, w, h, reduce, red.ptr, st);
        RR_HIP(hipMemcpyAsync(out, red.ptr, n_out * sizeof(float4), hipMemcpyDeviceToHost, st));
        RR_HIP(hipStreamSynchronize(st));
        return RR_OK;
    });
}

int rr_debug_film_window(rr_ctx* c, const float* rgba, int32_t w, int32_t h, int32_t x0, int32_t y0, int32_t x1,
                         int32_t y1, int32_t crop, float alpha_sum, float* out) {
    if (!c || !rgba || !out || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad arguments");
    const RegionRect r{x0, y0, x1, y1};
    if (r.empty() || x0 < 0 || y0 < 0 || x1 > w || y1 > h)
        return fail(RR_EINVAL, "the region must lie inside the image and hold a pixel");
    return guarded([&] {
        if (!idle(c)) return fail(RR_EBUSY, "submitted frames are pending");
        set_device(c);
        hipStream_t st = c->stream;
        const size_t n_in = (size_t)w * h, n_out = crop ? (size_t)r.w() * r.h() : n_in;
        DevBuf<float4> in, win;
        in.ensure(n_in);
        win.ensure(n_out);
        RR_HIP(hipMemcpyAsync(in.ptr, rgba, n_in * sizeof(float4), hipMemcpyHostToDevice, st));
        film_window_device(in.ptr, w, h, r, crop != 0, alpha_sum, win.ptr, st);
        RR_HIP(hipMemcpyAsync(out, win.ptr, n_out * sizeof(float4), hipMemcpyDeviceToHost, st));
        RR_HIP(hipStreamSynchronize(st));
        return RR_OK;
    });
}

int rr_debug_object_matrix(rr_scene* s, int32_t obj, double frame, double* m16) {
    if (!s || !m16) return fail(RR_EINVAL, "NULL argument");
    return guarded([&] {
        object_matrix(s->desc, obj, frame, m16);
        return RR_OK;
    });
}

}  // extern "C"
