// The state behind the C ABI's handles (rr_ctx, rr_scene, a frame slot) and
// the life of one frame: prepare, enqueue, finish, statistics (frame.cpp), and
// the device coders that write its file (coders.cpp). rr_api.cpp and
// rr_debug.cpp hold the extern "C" entry points that call these.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <string>
#include <unordered_set>
#include <vector>

#include "deflate.hpp"
#include "device.hpp"
#include "exr_codec.hpp"
#include "hdr.hpp"
#include "iris.hpp"
#include "reduce.hpp"
#include "region.hpp"
#include "rr.h"
#include "scene.hpp"
#include "settings.hpp"
#include "tga.hpp"
#include "view.hpp"
#include "webp.hpp"

namespace rr {

// Pinned host memory, grow-only, freed with its owner.
struct PinnedBuf {
    uint8_t* ptr = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    void ensure(size_t n) {
        if (n <= cap) return;
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
        RR_HIP(hipHostMalloc(reinterpret_cast<void**>(&ptr), n, hipHostMallocDefault));
        cap = n;
    }
    ~PinnedBuf() {
        if (ptr) (void)hipHostFree(ptr);
    }
};

// What a device-coded JPEG was coded with: the file's header is built from these.
struct JpegOut {
    int W = 0, H = 0, quality = 0;
    bool grey = false;
};

// What every body coder's plan says: whose it is, the image, the body's bound, the
// slot scratch the coder takes and the least a body holds (an exact length: body_cap).
struct BodyShape {
    Coder coder = Coder::None;
    int W = 0, H = 0;
    uint32_t body_cap = 0;
    size_t scratch_words = 0;
    uint64_t min_len = 0;
};

// The pinned stream of a body of at most body_cap bytes: 16 + the body rounded
// up to 16.
inline size_t body_stream_bytes(uint32_t body_cap) { return 16 + ((size_t)body_cap + 15) / 16 * 16; }

// Where a device coder writes: a frame slot has one for each of its outputs, and
// the context one more for the inspection entry points. An output is one file,
// so its coder writes the one pinned stream, [uint64 length][8 B pad][bytes]; a deflate
// coder also the bands' table, 2 or 4 words per band by the plan's own_stream.
// The rest is what the host builds the file's header or container from; the
// plans are made before the coder is enqueued (plan_or_refuse).
struct CodedOut {
    PinnedBuf stream, tab;
    JpegOut jpeg;
    rr::DeflatePlan deflate{};
    BodyShape body;  // of the plan below that the frame's format uses
    rr::ExrRowsPlan exr_rows{};  // OPEN_EXR with the codec NONE or RLE: a body in the stream, RLE's row table in tab
    rr::TgaPlan tga{};
    rr::HdrPlan hdr{};
    rr::IrisPlan iris{};
    rr::WebpPlan webp{};
};

// One file of a frame (rr_frame_output), resolved when the frame is submitted.
// Pinned memory grows on demand: an output a context never uses holds none.
struct SlotOutput {
    FrameOutput out;      // resolve_output
    CodedOut coded;       // the device-coded file's stream; its plan is made when the frame is submitted
    std::string path;     // without the extension
    std::string warning;  // a WEBP file below quality 100: lossless all the same; OPEN_EXR of a codec not built: ZIP
    int reduce = 1;       // the factor its image is reduced by
    int W = 0, H = 0;     // the image's size: the frame's, reduced
    PinnedBuf host_rgba;  // Coder::HostRgba: the 8-bit image, for the host coder
    uint64_t bytes = 0;   // the file's size, once written
};

struct FrameRun {
    int W, H, chunks, spp_chunk, tile_slices;
    long long pixels_run;  // the pixels whose camera rays ran: the frame's, or on the split path a region's
    bool rebuilt;
    float build_ms, trace_ms, readback_ms;
    float render_ms, device_ms;  // ev0 -> ev4 (build + trace + view transform), ev0 -> ev2 (+ device JPEG)
    std::vector<int32_t> counters;
    double kernel_ms[RR_K_CLASSES];
    int32_t kernel_launches[RR_K_CLASSES];
    unsigned long long trav[rr::kTravWords];
};

// One frame between rr_frame_submit and rr_frame_complete: its stream, its
// device state, its host-side outputs (pinned, so the device-to-host copies
// stay asynchronous), events and the request. Several slots = the next queued
// frames render while the host encodes and writes the previous one.
struct FrameSlot {
    bool busy = false;
    uint64_t ticket = 0;
    // 0 start, 1 built, 4 image done (before the device JPEG coder), 2 stream
    // work done (every output's coder), 3 outputs on the host (after their
    // copies), 5 (frames whose files all come from slot coders) before the
    // slot's reductions and coders: the state shared between frames is free
    hipEvent_t ev[6] = {};
    // The slot's frames run on its own stream and write only its own device
    // state, so a k_tiles frame runs on the GPU beside the other slots'
    // frames, and the copies of a frame's outputs to the host run while the
    // next frames' kernels write the other slots'.
    hipStream_t stream = nullptr;
    rr::DevFrame dev;
    // The products of the hierarchy builds of this slot's k_tiles frames, for
    // the scene `build_scene`. Frames of the split path never overlap their
    // predecessor, so they use the scene's own set: a large scene is held
    // once, not once per slot.
    rr::DevBuild build;
    const rr_scene* build_scene = nullptr;
    bool tiles = false;  // this frame renders with k_tiles (may overlap its neighbours)
    PinnedBuf host_counters, host_upload;
    // The frame's files, outs[0 .. n_outs): none for a frame without a path. rr_render_frame_to_memory has
    // one of Coder::HostRgba without a path: the 8-bit image to the host.
    SlotOutput outs[RR_MAX_FRAME_OUTPUTS];
    int n_outs = 0;
    bool slot_coders_only = false;  // every output is coded by a slot coder (enqueue_frame: what the next frame waits for)
    rr::FrameSetup fs;
    rr::FrameRegion region;  // resolve_region at submit: what of the frame is rendered and written
    bool view_substituted = false;  // the scene's view settings not applied in full (view_warning says what)
    std::string view_warning;
    double submit_at = 0.0;         // UNIX time when the device work was enqueued
    bool anchor = false;            // submitted to an idle context: its device start is submit_at
    rr_scene* scene = nullptr;
    float* film_out = nullptr;
    FrameRun r{};
    rr_frame_timing tm{};
    double anim_ms = 0.0;
    std::chrono::steady_clock::time_point t_call;
};

}  // namespace rr

struct rr_ctx {
    int device = 0;
    // the home stream, which the inspection entry points enqueue on: slot 0's
    // (rr_create says why there is no further stream)
    hipStream_t stream = nullptr;
    rr::DevPaths paths;  // shared by all frames: the split path's queues, read-only tables
    rr::DevFrame home;   // the inspection entry points' frame state (a frame uses its slot's)
    rr::CodedOut home_coded;  // and their coders' outputs: an inspection call touches no frame slot
    // tables of the device JPEG coder (jpeg.hip), read by every slot's frames:
    // the transform's by quality, each written once when first asked for and
    // never again (so two JPEG outputs of one frame may differ in quality, and
    // a change of quality waits for nobody); the entropy coder's Huffman codes
    rr::DevBuf<float> jpeg_tab[101];
    rr::DevBuf<uint32_t> jpeg_huff;
    rr::OutputSettings settings;  // rr_set_* / RR_* (settings.hpp)
    rr::DevBuf<float> srgb16_lut;  // the 16-bit path's sRGB table (build_srgb16_lut), uploaded at its first frame
    std::vector<float> filter_cache;
    float filter_width_cached = -1.f;
    bool srgb_uploaded = false;
    rr::FrameSlot slots[RR_MAX_FRAMES_IN_FLIGHT];
    uint64_t next_ticket = 1;     // tickets are issued in submission order
    uint64_t next_complete = 1;   // the ticket rr_frame_complete expects next
    rr::FrameSlot* last_enqueued = nullptr;  // the slot of the frame enqueued last (its ev[2]: device work done)
    // UNIX-time estimate of when the compute stream finished the last completed
    // frame (rr_frame_complete): the next frame's device work cannot start before
    double gpu_free_at = 0.0;
    rr::FilmicDev filmic;         // the Filmic family's LUTs (rr_set_ocio_config / RR_OCIO_DIR)
    // rr_last_warning = the context's warning (a broken RR_OCIO_DIR, kept for
    // the context's lifetime) + the last completed frame's
    std::string ctx_warning, frame_warning, warning;
    // the files of the frame completed last (rr_last_output_bytes)
    uint64_t last_output_bytes[RR_MAX_FRAME_OUTPUTS] = {};
    int last_outputs = 0;
    // Device start times of completed frames (rr_frame_complete): every frame
    // also records its start on start_ring[ticket % kStartRing], which outlives
    // the frame slot's own events by a few frames, so the next frame's start is
    // the previous one's plus the device clock's difference between the two.
    static constexpr int kStartRing = 8;
    hipEvent_t start_ring[kStartRing] = {};
    uint64_t chain_ticket = 0;   // last completed frame whose device start is known (0: none)
    double chain_unix = 0.0;     // its device start, UNIX seconds
    double last_render_end = 0.0;  // finished_rendering_at of the last completed frame
    // scenes bound to this context: rr_destroy releases their device buffers
    // and unbinds them, so a scene freed after its context touches no freed state
    std::unordered_set<rr_scene*> scenes;
};

struct rr_scene {
    rr_ctx* ctx = nullptr;
    rr::SceneDesc desc;
    rr::DevMesh mesh;    // uploaded once
    rr::DevBuild build;  // split-path frames and the inspection calls build here; k_tiles frames in their slot's set
};

namespace rr {

inline void set_device(rr_ctx* c) { RR_HIP(hipSetDevice(c->device)); }
inline FrameSlot* slot_for(rr_ctx* c, uint64_t ticket) { return &c->slots[ticket % RR_MAX_FRAMES_IN_FLIGHT]; }
inline bool idle(rr_ctx* c) { return c->next_complete == c->next_ticket; }

// Waits for every stream of the context. Called before a table that all
// frames read (filter, sRGB, JPEG, Filmic) is rewritten, since a frame of
// another slot may still be reading it.
void quiesce(rr_ctx* c);

// A scene is used with exactly one context; a host-only handle binds on first
// use, which uploads its triangles.
void bind_scene(rr_ctx* c, rr_scene* s);

// Hierarchy ids (render_ints[7] of rr_debug_frame_state, rr_debug_trace):
// 2 = Karras LBVH (BVH2), 3 = PLOC (BVH2), 4 = PLOC (LBVH below 3 triangles)
// collapsed to the quantised 6-wide hierarchy (rr_device.h QNode6).
constexpr int kHierLbvh = 2, kHierPloc = 3, kHierQWide = 4;  // 4: the quantised 6-wide collapse (ABI value kept)

FrameConsts make_consts(const FrameSetup& fs, int n_tris);

// The hierarchy the frame kernels walk: the LBVH for frames k_tiles renders
// (LDS-resident scenes), the quantised BVH4 for the split path (larger scenes,
// and LDS-resident ones under RR_FLAG_WAVEFRONT).
int frame_hier(const FrameSetup& fs, int n_tris);

// The samples a chunk of the split path takes: by the frame's size alone, and
// lowered to what the device's free memory holds.
int choose_spp_chunk(const FrameSetup& fs);
// npix: the pixels the split path enumerates (a region's; 0: the frame's).
int fit_spp_chunk(const FrameSetup& fs, const DevPaths& p, long long npix = 0);

// The view transform, look and display gamma a frame on ctx is rendered with
// (fs.view_transform, fs.look, fs.gamma). The context's look and gamma come
// before the scene's. The Filmic family needs the context's LUTs, without them
// Standard; False Color its cube, without it Standard; a look the Filmic view
// and its curve, without either no look. Returns what of the view settings
// the frame does not apply ("" if nothing): those fallbacks, and the scene's
// own notes (FrameSetup::view_note: a view transform or look nobody knows).
std::string resolve_view(const rr_ctx* c, FrameSetup& fs);

// The view settings as kernel arguments, for a view, look and gamma that
// resolve_view (or an inspection call's own check) has passed. dither: the
// 8-bit pass's intensity (the 16-bit front end takes none).
FilmicArgs view_args(const rr_ctx* c, int view, int look, float gamma, float dither = 0.f);

// The 8-bit path's sRGB table on the device (DevPaths::srgb_lut), uploaded
// once with every stream idle.
void ensure_srgb(rr_ctx* c);

// Upload per-frame constants and (re)build the LBVH if object transforms changed.
// `staging` (pinned, per frame slot) keeps the host-to-device copies
// asynchronous, so a frame can be enqueued while the previous one still runs.
// Works on stream st with frame state f and builds into d, a set of products
// of s's mesh. Returns whether it rebuilt.
// hier: 0 = the frame's hierarchy, else a kHier* id (inspection entry points).
bool prepare_frame(rr_ctx* c, rr_scene* s, DevBuild& d, DevFrame& f, hipStream_t st, const FrameSetup& fs,
                   PinnedBuf& staging, int hier = 0);

// Enqueue the device part of one frame on its slot's stream, with the slot's
// device state (no host synchronisation): LBVH (if needed), wavefront, tonemap,
// optionally the file's device coder, and the asynchronous copies of the slot's outputs.
void enqueue_frame(rr_ctx* c, FrameSlot& sl);
// Wait for a slot's device work and collect its timings and counters.
void finish_frame(rr_ctx* c, FrameSlot& sl);
// The frame's render span in the worker's record (sl.tm), from the device's
// own clock, once finish_frame has returned. t_sync: the UNIX time then.
void set_render_span(rr_ctx* c, FrameSlot& sl, double t_sync);
// width, height: the frame's; camera_rays: of the pixels that ran (FrameRun::pixels_run).
void fill_stats(rr_frame_stats* st, const FrameSetup& fs, const FrameRun& r, int n_tris);

// ---- the device coders (coders.cpp) ----------------------------------------

// The image a coder reads (formats.hpp CoderInfo::film): rgba8, or the film,
// W x H float4 sums scaled by inv_spp. exposure_scale, view_transform, look
// and gamma (resolved: resolve_view, or an inspection call's own check): Png16,
// which takes the film through exposure and view transform again at 16 bits.
// alpha_one (Exr, Exr32): A = 1, as in a rendered frame's file; else the
// image's own alpha. jpeg_tab: the transform's table for the file's quality
// (jpeg_table).
struct CoderInput {
    const uint8_t* rgba8 = nullptr;
    const float4* film = nullptr;
    int W = 0, H = 0;
    float inv_spp = 1.0f, exposure_scale = 1.0f;
    int view_transform = VIEW_STANDARD, look = 0;
    float gamma = 1.0f;
    bool alpha_one = true;
    // the film is an uncropped region frame's windowed film: film.w != 0 marks the region. Exr, Exr32: A = 1
    // there and 0 outside; Png16: A = 65535 there, (0, 0, 0, 0) outside. Comes before alpha_one.
    bool alpha_mask = false;
    const float* jpeg_tab = nullptr;
};

// The plan of a W x H image for fo's deflate or body coder, into o (any other
// coder has none: RR_OK). A size outside the coder's range is refused
// (RR_EINVAL, CoderInfo::range), never rerouted: there is no other coder that
// writes the same file.
int plan_or_refuse(const FrameOutput& fo, int W, int H, CodedOut& o);
// What a WEBP file of this quality is flagged with (rr_last_warning): "" at 100
// and above, else that the file is lossless, as lossy WEBP is not built.
std::string webp_quality_warning(int quality);

// The 16-bit path's sRGB table on the device. Written once, before the first
// kernel that reads it is enqueued, and never again.
void ensure_srgb16(rr_ctx* c);
// The device JPEG transform's table for `quality` (1 .. 100), uploaded when
// first asked for into a buffer nothing reads yet.
const float* jpeg_table(rr_ctx* c, int quality);

// Everything enqueue_coder(fo, a W x H image) allocates, in f's scratch and o's
// pinned buffers, and the tables it uploads. A frame reserves for all its
// outputs before it enqueues the first coder: the coders of one frame run one
// after another on the slot's stream and share f's scratch, and a buffer that
// grew (DevBuf::ensure frees and allocates) under a coder still queued would be
// freed under it. Grow-only, so the scratch ends at the largest plan's size.
void reserve_coder(rr_ctx* c, const FrameOutput& fo, int W, int H, DevFrame& f, CodedOut& o);

// Enqueue the device coder that `fo` names (Jpeg ... Webp) on stream st, with
// f's scratch and profiler, into o's pinned buffers. fo.color_mode: the file's
// channels; fo.png_compression ("PNG"): LEGACY the Sub front end, 0 .. 100 the
// adaptive one (the device coders have one effort level). A deflate or body
// coder codes by its plan in o (plan_or_refuse). Reserves first (reserve_coder:
// nothing new for a frame that has reserved already).
void enqueue_coder(rr_ctx* c, const FrameOutput& fo, const CoderInput& in, DevFrame& f, hipStream_t st, CodedOut& o);

// The file of a device-coded image, once its stream is on the host: the
// host-built header or container around it.
void coded_file_bytes(const CodedOut& o, const FrameOutput& fo, std::vector<uint8_t>& data);

// The host coders: an RGBA8 image as a file of `format` at out_path + its
// extension (a format that needs the float film: RR_ENOTSUP). mode: a colour
// mode as rr_set_color_mode takes it, 0 the format's own layout. compression ("PNG"): LEGACY, or 0 .. 100 (rr_set_png_compression).
int do_encode(const uint8_t* rgba, int W, int H, const char* out_path, const char* format, int quality,
              uint64_t* bytes, int mode = 0, int compression = RR_PNG_COMPRESSION_LEGACY);

}  // namespace rr
