// C ABI of the renderer (include/rr.h). One rr_ctx per GPU; one rr_scene per
// exported project, cached for the worker's lifetime. Every function here is
// an argument check and a call: the frame's life is in frame.cpp, the coders
// in coders.cpp, the settings in settings.cpp; rr_debug.cpp has the
// inspection entry points.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>

#include "api_util.hpp"
#include "frame.hpp"
#include "image_io.hpp"

using namespace rr;

namespace {

// rr_set_*: a refused value is RR_EINVAL and changes nothing.
int setter_result(bool ok, const std::string& err) { return ok ? RR_OK : fail(RR_EINVAL, err); }

}  // namespace

extern "C" {

void rr_render_params_default(rr_render_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->spp = 0;
    p->max_bounces = -1;
    p->clamp_indirect = -1.0f;
    p->seed = 0;
    p->use_scene_seed = 1;
    p->width = 0;
    p->height = 0;
    p->view_transform = RR_VIEW_SCENE;
    p->spp_per_chunk = 0;
    p->max_diffuse_bounces = -1;
    p->max_glossy_bounces = -1;
}

// The warning of a host encode, which has no context: rr_last_warning(NULL).
static void set_encode_warning(const char* format, int quality) {
    const Format* f = find_format(format);
    g_warn = f && f->coder == Coder::Webp ? webp_quality_warning(quality) : "";
}

int32_t rr_abi_version(void) { return RR_ABI_VERSION; }

const char* rr_last_error(rr_ctx*) { return g_err.c_str(); }

const char* rr_last_warning(rr_ctx* c) {
    if (!c) return g_warn.c_str();
    c->warning = c->ctx_warning;
    if (!c->frame_warning.empty()) c->warning += (c->warning.empty() ? "" : "; ") + c->frame_warning;
    return c->warning.c_str();
}

int rr_set_ocio_config(rr_ctx* c, const char* dir) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    return guarded([&] {
        set_device(c);
        quiesce(c);
        c->filmic.release();
        c->ctx_warning.clear();  // an RR_OCIO_DIR problem is superseded by this call
        if (!dir || !*dir) return RR_OK;
        FilmicLuts l;
        std::string err;
        if (!load_filmic_luts(dir, l, err)) return fail(err.rfind("no ", 0) == 0 || err.rfind("cannot", 0) == 0 ? RR_ENOENT : RR_EINVAL, err);
        c->filmic.upload(l, dir);
        return RR_OK;
    });
}

int rr_create(int device_ordinal, rr_ctx** out) {
    if (!out) return fail(RR_EINVAL, "out is NULL");
    *out = nullptr;
    return guarded([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RR_ENODEV, "no HIP device available");
        if (device_ordinal < 0 || device_ordinal >= n)
            return fail(RR_ENODEV, "device ordinal " + std::to_string(device_ordinal) + " out of range (" +
                                       std::to_string(n) + " visible)");
        OutputSettings settings;
        std::string err;
        if (!settings_from_env(settings, err)) return fail(RR_EINVAL, err);
        std::unique_ptr<rr_ctx> c(new rr_ctx());
        c->device = device_ordinal;
        c->settings = settings;
        set_device(c.get());
        // One stream per slot and no other, so that each gets a hardware queue
        // of its own (GPU_MAX_HW_QUEUES is 4, and the process's null stream
        // holds one): streams created beyond that share a queue, and a queue
        // runs its kernels in order, so frames of two slots on one queue
        // cannot overlap. The home stream (inspection calls) is slot 0's;
        // with RR_MAX_FRAMES_IN_FLIGHT = 3 the three slots and the null stream
        // take the four queues.
        for (auto& sl : c->slots) RR_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        c->stream = c->slots[0].stream;
        if (const char* d = getenv("RR_OCIO_DIR")) {
            // a broken LUT directory does not fail the context: Filmic frames fall
            // back to Standard and carry the reason in rr_last_warning
            FilmicLuts l;
            std::string lut_err;
            if (*d && load_filmic_luts(d, l, lut_err)) c->filmic.upload(l, d);
            else if (*d) c->ctx_warning = "RR_OCIO_DIR: " + lut_err;
        }
        *out = c.release();
        return RR_OK;
    });
}

void rr_destroy(rr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (auto& sl : c->slots)
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    c->paths.release();
    c->home.release();
    c->filmic.release();
    for (auto& t : c->jpeg_tab) t.release();
    c->jpeg_huff.release();
    c->srgb16_lut.release();
    for (auto& sl : c->slots)
        for (auto& e : sl.ev)
            if (e) (void)hipEventDestroy(e);
    for (auto& e : c->start_ring)
        if (e) (void)hipEventDestroy(e);
    for (rr_scene* s : c->scenes) {  // still-open scenes: back to host-only handles
        s->mesh.release();
        s->build.release();
        s->ctx = nullptr;
    }
    for (auto& sl : c->slots) {
        if (sl.stream) (void)hipStreamDestroy(sl.stream);  // c->stream is slot 0's
        sl.dev.release();
        for (auto& r : sl.dev.reduced) {
            r.film.release();
            r.rgba8.release();
        }
        sl.build.release();
    }
    delete c;
}

int rr_scene_load(rr_ctx* c, const char* path, rr_scene** out) {
    if (!path || !out) return fail(RR_EINVAL, "NULL argument");
    *out = nullptr;
    {
        FILE* f = std::fopen(path, "rb");
        if (!f) return fail(RR_ENOENT, std::string("scene file doesn't exist: ") + path);
        std::fclose(f);
    }
    return guarded([&] {
        std::unique_ptr<rr_scene> s(new rr_scene());
        s->desc = load_scene(path);
        s->mesh.n_tris = (int)s->desc.tri_obj.size();
        s->mesh.n_objs = (int)s->desc.objects.size();
        if (c) bind_scene(c, s.get());  // NULL: host-only handle, bound to a context at its first render
        *out = s.release();
        return RR_OK;
    });
}

void rr_scene_free(rr_scene* s) {
    if (!s) return;
    if (rr_ctx* c = s->ctx) {
        (void)hipSetDevice(c->device);
        for (auto& sl : c->slots) {
            if (sl.stream) (void)hipStreamSynchronize(sl.stream);
            if (sl.build_scene == s) {  // the slot's build products of this scene
                sl.build.release();
                sl.build_scene = nullptr;
            }
        }
        c->scenes.erase(s);
    }
    s->mesh.release();
    s->build.release();
    delete s;
}

int rr_scene_resolution(rr_scene* s, const rr_render_params* p, int32_t* w, int32_t* h) {
    if (!s) return fail(RR_EINVAL, "scene is NULL");
    const RenderDesc& r = s->desc.render;
    if (w) *w = (p && p->width > 0) ? p->width : (r.resx * r.percent) / 100;
    if (h) *h = (p && p->height > 0) ? p->height : (r.resy * r.percent) / 100;
    return RR_OK;
}

int rr_region_resolution(rr_ctx* c, rr_scene* s, const rr_render_params* p, int32_t* w, int32_t* h) {
    if (!c || !s) return fail(RR_EINVAL, "NULL ctx or scene");
    int32_t W = 0, H = 0;
    rr_scene_resolution(s, p, &W, &H);
    FrameRegion rg;
    std::string err;
    if (!resolve_region(c->settings, s->desc.render, W, H, rg, err)) return fail(RR_EINVAL, err);
    if (w) *w = rg.out_w(W);
    if (h) *h = rg.out_h(H);
    return RR_OK;
}

int rr_set_region(rr_ctx* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t crop) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_region(c->settings, x0, y0, x1, y1, crop != 0, err), err);
}

int rr_set_region_off(rr_ctx* c) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    set_region_off(c->settings);
    return RR_OK;
}

int rr_set_region_from_scene(rr_ctx* c, int32_t on) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    set_region_from_scene(c->settings, on != 0);
    return RR_OK;
}

}  // extern "C"

namespace {

// A frame's submission, with the files it was asked for (none: a frame without
// a path). What the context and the scene add comes on top; the whole list is
// checked, resolved and planned before anything is enqueued.
int submit_frame(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params,
                 std::vector<OutputRequest> list, uint64_t* ticket) {
    if (s->ctx && s->ctx != c) return fail(RR_EINVAL, "scene belongs to another context");
    add_extra_outputs(c->settings, s->desc.render, list);
    if (!list.empty()) {
        std::string err;
        if (const int rc = check_outputs(list, err)) return fail(rc, err);
    }
    FrameSlot* sl = slot_for(c, c->next_ticket);
    if (sl->busy) return fail(RR_EBUSY, "too many frames in flight (complete the oldest first)");
    return guarded([&] {
        sl->t_call = std::chrono::steady_clock::now();
        sl->tm = rr_frame_timing{};
        sl->tm.loaded_at = unix_now();
        const auto t_anim = std::chrono::steady_clock::now();
        sl->fs = setup_frame(s->desc, frame, params);
        sl->view_warning = resolve_view(c, sl->fs);
        sl->view_substituted = !sl->view_warning.empty();
        sl->anim_ms = ms_since(t_anim);
        sl->tm.started_rendering_at = unix_now();
        sl->scene = s;
        sl->n_outs = 0;  // (a refusal below leaves the slot without a frame)
        {
            std::string err;
            if (!resolve_region(c->settings, s->desc.render, sl->fs.W, sl->fs.H, sl->region, err))
                return fail(RR_EINVAL, err);
        }
        const int OW = sl->region.out_w(sl->fs.W), OH = sl->region.out_h(sl->fs.H);
        bool slot_only = !list.empty();
        for (size_t i = 0; i < list.size(); ++i) {
            const OutputRequest& q = list[i];
            SlotOutput& o = sl->outs[i];
            o.out = resolve_output(c->settings, s->desc.render, q.format.c_str(), true, q.quality);
            o.path = q.path;
            o.reduce = q.reduce;
            o.W = reduced_size(OW, q.reduce);
            o.H = reduced_size(OH, q.reduce);
            o.bytes = 0;
            if (const int rc = plan_or_refuse(o.out, o.W, o.H, o.coded)) return rc;
            o.warning = o.out.coder == Coder::Webp ? webp_quality_warning(o.out.quality) : exr_codec_warning(o.out);
            if (!slot_coder(o.out.coder)) slot_only = false;
        }
        sl->n_outs = (int)list.size();
        sl->slot_coders_only = slot_only;
        for (int i = 0; i < sl->n_outs; ++i)
            if (sl->outs[i].out.coder == Coder::Png16) {
                set_device(c);
                ensure_srgb16(c);
            }
        sl->film_out = nullptr;
        sl->anchor = idle(c);
        sl->submit_at = unix_now();
        sl->ticket = c->next_ticket;
        enqueue_frame(c, *sl);
        sl->busy = true;
        ++c->next_ticket;
        *ticket = sl->ticket;
        return RR_OK;
    });
}

}  // namespace

extern "C" {

int rr_frame_submit(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params, const char* out_path,
                    const char* format, int32_t jpeg_quality, uint64_t* ticket) {
    if (!c || !s || !ticket) return fail(RR_EINVAL, "NULL ctx, scene or ticket");
    if (out_path && !format) return fail(RR_EINVAL, "format is required when out_path is given");
    std::vector<OutputRequest> list;
    if (out_path) list.push_back({out_path, format, jpeg_quality, 1});
    return submit_frame(c, s, frame, params, std::move(list), ticket);
}

int rr_frame_submit_outputs(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params,
                            const rr_frame_output* outs, int32_t n, uint64_t* ticket) {
    if (!c || !s || !ticket) return fail(RR_EINVAL, "NULL ctx, scene or ticket");
    if (n < 1 || n > RR_MAX_FRAME_OUTPUTS || !outs)
        return fail(RR_EINVAL, "a frame writes 1 .. " + std::to_string(RR_MAX_FRAME_OUTPUTS) + " files, not " +
                                   std::to_string(n));
    std::vector<OutputRequest> list;
    for (int32_t i = 0; i < n; ++i) {
        if (!outs[i].out_path || !outs[i].format) return fail(RR_EINVAL, "every output needs out_path and format");
        list.push_back({outs[i].out_path, outs[i].format, outs[i].jpeg_quality, outs[i].reduce});
    }
    return submit_frame(c, s, frame, params, std::move(list), ticket);
}

int rr_frame_complete(rr_ctx* c, uint64_t ticket, rr_frame_timing* timing, rr_frame_stats* stats) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    if (ticket != c->next_complete) return fail(RR_EINVAL, "frames must be completed in submission order");
    FrameSlot* sl = slot_for(c, ticket);
    if (!sl->busy || sl->ticket != ticket) return fail(RR_EINVAL, "unknown ticket");
    const int rc = guarded([&] {
        finish_frame(c, *sl);
        const FrameSetup& fs = sl->fs;
        set_render_span(c, *sl, unix_now());
        const auto t_enc = std::chrono::steady_clock::now();
        // Every file is built and written, also behind one that failed: the
        // first failure's code is the frame's, and its text names every file
        // that was not written.
        int failed = RR_OK;
        std::string failures;
        c->last_outputs = sl->n_outs;
        for (int i = 0; i < sl->n_outs; ++i) {
            SlotOutput& o = sl->outs[i];
            const FrameOutput& fo = o.out;
            o.bytes = 0;
            int e = RR_OK;
            if (fo.coder == Coder::Jpeg || slot_coder(fo.coder)) {  // the host's container + the device-coded stream
                std::vector<uint8_t> data;
                coded_file_bytes(o.coded, fo, data);
                const std::string path = o.path + coder_ext(fo.coder);
                if (write_file(path, data)) o.bytes = data.size();
                else e = fail(RR_EIO, "cannot write " + path + ": " + std::strerror(errno));
            } else if (fo.coder == Coder::HostRgba) {  // a submitted frame's: "PNG" by the host coder
                e = do_encode(o.host_rgba.ptr, o.W, o.H, o.path.c_str(), "PNG", fo.quality, &o.bytes, fo.color_mode,
                              fo.png_compression);
            }
            c->last_output_bytes[i] = o.bytes;
            if (e != RR_OK) {
                if (failed == RR_OK) failed = e;
                failures += (failures.empty() ? "" : "; ") + g_err;
            }
        }
        if (failed != RR_OK) return fail(failed, failures);
        const uint64_t bytes = sl->n_outs ? sl->outs[0].bytes : 0;
        const double enc_ms = ms_since(t_enc);
        sl->tm.file_saving_finished_at = unix_now();
        if (timing) *timing = sl->tm;
        c->frame_warning = sl->view_warning;
        for (int i = 0; i < sl->n_outs; ++i)
            if (!sl->outs[i].warning.empty())
                c->frame_warning += (c->frame_warning.empty() ? "" : "; ") + sl->outs[i].warning;
        if (stats) {
            fill_stats(stats, fs, sl->r, sl->scene->mesh.n_tris);
            stats->view_transform_substituted = sl->view_substituted ? 1 : 0;
            stats->anim_ms = sl->anim_ms;
            stats->encode_ms = enc_ms;
            stats->output_bytes = bytes;
            stats->total_ms = ms_since(sl->t_call);
        }
        return RR_OK;
    });
    sl->busy = false;
    c->next_complete = ticket + 1;
    return rc;
}

int rr_render_frame(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params, const char* out_path,
                    const char* format, int32_t jpeg_quality, rr_frame_timing* timing, rr_frame_stats* stats) {
    if (c && c->next_complete != c->next_ticket)
        return fail(RR_EBUSY, "rr_render_frame while submitted frames are pending");
    uint64_t t = 0;
    const int rc = rr_frame_submit(c, s, frame, params, out_path, format, jpeg_quality, &t);
    if (rc != RR_OK) return rc;
    return rr_frame_complete(c, t, timing, stats);
}

int rr_render_frame_outputs(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params,
                            const rr_frame_output* outs, int32_t n, rr_frame_timing* timing, rr_frame_stats* stats) {
    if (c && c->next_complete != c->next_ticket)
        return fail(RR_EBUSY, "rr_render_frame_outputs while submitted frames are pending");
    uint64_t t = 0;
    const int rc = rr_frame_submit_outputs(c, s, frame, params, outs, n, &t);
    if (rc != RR_OK) return rc;
    return rr_frame_complete(c, t, timing, stats);
}

int rr_last_output_bytes(rr_ctx* c, int32_t index, uint64_t* bytes) {
    if (!c || !bytes) return fail(RR_EINVAL, "NULL argument");
    if (index < 0 || index >= c->last_outputs)
        return fail(RR_EINVAL, "the frame completed last wrote " + std::to_string(c->last_outputs) + " files");
    *bytes = c->last_output_bytes[index];
    return RR_OK;
}

int rr_set_extra_outputs(rr_ctx* c, const char* spec) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_extra_outputs(c->settings, spec, err), err);
}

int rr_synchronize(rr_ctx* c) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    return guarded([&] {
        set_device(c);
        quiesce(c);
        return RR_OK;
    });
}

int rr_render_frame_to_memory(rr_ctx* c, rr_scene* s, int32_t frame, const rr_render_params* params,
                              float* film, uint8_t* rgba8, rr_frame_stats* stats) {
    if (!c || !s) return fail(RR_EINVAL, "NULL ctx or scene");
    if (s->ctx && s->ctx != c) return fail(RR_EINVAL, "scene belongs to another context");
    if (c->next_complete != c->next_ticket) return fail(RR_EBUSY, "submitted frames are pending");
    FrameSlot* sl = slot_for(c, c->next_ticket);
    return guarded([&] {
        sl->t_call = std::chrono::steady_clock::now();
        sl->fs = setup_frame(s->desc, frame, params);
        sl->view_warning = resolve_view(c, sl->fs);
        sl->view_substituted = !sl->view_warning.empty();
        sl->scene = s;
        {
            std::string err;
            if (!resolve_region(c->settings, s->desc.render, sl->fs.W, sl->fs.H, sl->region, err))
                return fail(RR_EINVAL, err);
        }
        const int OW = sl->region.out_w(sl->fs.W), OH = sl->region.out_h(sl->fs.H);
        SlotOutput& o = sl->outs[0];  // the 8-bit image to the host; no file
        o.out = FrameOutput{};
        o.out.coder = Coder::HostRgba;
        o.path.clear();
        o.warning.clear();
        o.reduce = 1;
        o.W = OW;
        o.H = OH;
        sl->n_outs = 1;
        sl->slot_coders_only = false;
        sl->film_out = film;
        sl->ticket = c->next_ticket;
        enqueue_frame(c, *sl);
        finish_frame(c, *sl);
        sl->film_out = nullptr;
        const FrameSetup& fs = sl->fs;
        if (rgba8) std::memcpy(rgba8, sl->outs[0].host_rgba.ptr, (size_t)OW * OH * 4);
        c->frame_warning = sl->view_warning;
        if (stats) {
            fill_stats(stats, fs, sl->r, s->mesh.n_tris);
            stats->view_transform_substituted = sl->view_substituted ? 1 : 0;
            stats->total_ms = ms_since(sl->t_call);
        }
        return RR_OK;
    });
}

int rr_encode_image(const uint8_t* rgba8, int32_t w, int32_t h, const char* out_path, const char* format,
                    int32_t quality, uint64_t* bytes) {
    if (!rgba8 || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad image");
    set_encode_warning(format, quality);
    return guarded([&] { return do_encode(rgba8, w, h, out_path, format, quality, bytes); });
}

int rr_encode_image_mode(const uint8_t* rgba8, int32_t w, int32_t h, const char* out_path, const char* format,
                         int32_t quality, int32_t color_mode, uint64_t* bytes) {
    if (!rgba8 || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad image");
    if (!valid_color_mode(color_mode)) return fail(RR_EINVAL, "bad colour mode");
    set_encode_warning(format, quality);
    return guarded([&] { return do_encode(rgba8, w, h, out_path, format, quality, bytes, color_mode); });
}

int rr_encode_image_png(const uint8_t* rgba8, int32_t w, int32_t h, const char* out_path, int32_t color_mode,
                        int32_t compression, uint64_t* bytes) {
    if (!rgba8 || w <= 0 || h <= 0) return fail(RR_EINVAL, "bad image");
    if (!valid_color_mode(color_mode)) return fail(RR_EINVAL, "bad colour mode");
    if (!valid_png_compression(compression) || compression == RR_PNG_COMPRESSION_SCENE)
        return fail(RR_EINVAL, "PNG compression must be 0 .. 100 or RR_PNG_COMPRESSION_LEGACY");
    return guarded([&] { return do_encode(rgba8, w, h, out_path, "PNG", 90, bytes, color_mode, compression); });
}

// The settings (settings.hpp has their values): read when a frame is
// submitted; frames in flight keep their choice.

int rr_set_device_png(rr_ctx* c, int32_t on) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    set_device_png(c->settings, on != 0);
    return RR_OK;
}

int rr_set_png_depth(rr_ctx* c, int32_t depth) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_png_depth(c->settings, depth, err), err);
}

int rr_set_exr_depth(rr_ctx* c, int32_t depth) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_exr_depth(c->settings, depth, err), err);
}

int rr_set_exr_codec(rr_ctx* c, int32_t codec) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_exr_codec(c->settings, codec, err), err);
}

int rr_set_color_mode(rr_ctx* c, int32_t mode) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_color_mode(c->settings, mode, err), err);
}

int rr_set_look(rr_ctx* c, const char* name) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_look(c->settings, name, err), err);
}

int rr_set_display_gamma(rr_ctx* c, float gamma) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_display_gamma(c->settings, gamma, err), err);
}

int rr_set_dither(rr_ctx* c, float intensity) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_dither(c->settings, intensity, err), err);
}

int rr_set_png_compression(rr_ctx* c, int32_t percent) {
    if (!c) return fail(RR_EINVAL, "NULL ctx");
    std::string err;
    return setter_result(set_png_compression(c->settings, percent, err), err);
}

}  // extern "C"
