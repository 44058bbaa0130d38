/*
 * rr.h — C ABI of the MI355X frame renderer ("rr" = render-runner backend).
 *
 * This is the drop-in boundary for the one hot path of the render cluster: the
 * worker's per-frame render step. In the reference that step is a process
 * boundary: BlenderJobRunner::render_frame spawns `blender <blend> --background
 * --python render-timing-script.py -- --render-output … --render-format …
 * --render-frame N` and parses its stdout
 * (/root/reference/worker/src/rendering/runner/mod.rs:72-203, argv :140-158,
 * spawn :165-174; stdout protocol worker/src/rendering/runner/utilities.rs:105-203).
 * Here the same step is an in-process call: scene exported once per project,
 * uploaded once, then rr_render_frame() per frame index.
 *
 * Plain C types only (no torch / HIP types). All functions return 0 on success
 * and a negative errno-style code on failure; rr_last_error() then holds a
 * UTF-8 message (thread-local, valid until the next call on this thread).
 *
 * Threading: one rr_ctx per GPU per process; a ctx is NOT thread-safe, calls on
 * one ctx must be serialised by the caller (the reference worker renders one
 * frame at a time per worker: worker/src/rendering/queue.rs:79-118).
 * Ownership: the caller owns ctx and scene handles (Rust Drop -> rr_scene_free /
 * rr_destroy).
 */
#ifndef RR_H
#define RR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 8

/* error codes (negative errno values) */
#define RR_OK 0
#define RR_ENOENT (-2)   /* file missing (reference: runner/mod.rs:82-87, :99-104) */
#define RR_EIO (-5)      /* read/write failure (reference: create_dir_all :117-121) */
#define RR_ENOMEM (-12)  /* host or device allocation failure */
#define RR_EINVAL (-22)  /* bad argument / malformed scene */
#define RR_ENODEV (-19)  /* HIP device unavailable / kernel launch failure */
#define RR_ENOTSUP (-95) /* unsupported output format or scene feature */
#define RR_EBUSY (-16)   /* rr_frame_submit with RR_MAX_FRAMES_IN_FLIGHT frames pending */

/* Frames a context keeps between rr_frame_submit and rr_frame_complete. */
#define RR_MAX_FRAMES_IN_FLIGHT 3

typedef struct rr_ctx rr_ctx;
typedef struct rr_scene rr_scene;

/* View transform selector (scene "view_transform"). */
#define RR_VIEW_SCENE (-1)  /* use the scene file's setting */
#define RR_VIEW_STANDARD 0  /* sRGB OETF, Blender "Standard" */
#define RR_VIEW_RAW 1       /* linear values, clamped, no OETF */
#define RR_VIEW_FILMIC 2    /* Blender "Filmic" (display sRGB) through the OCIO LUTs of a
                             * Blender colour-management directory (rr_set_ocio_config), with
                             * the frame's look (rr_set_look); without the LUTs the frame is
                             * rendered with Standard and flagged
                             * (rr_frame_stats.view_transform_substituted, rr_last_warning) */
#define RR_VIEW_FILMIC_LOG 3   /* Blender "Filmic Log": the Filmic chain without its 1D curve */
#define RR_VIEW_FALSE_COLOR 4  /* Blender "False Color": Filmic Log's luminance through
                                * filmic_false_color.spi3d; without that file Standard, flagged */

/* Render parameters. Any field left at its "use scene" value takes the value
 * exported from the project (scene file "render" block). Zero-initialising the
 * struct and then calling rr_render_params_default() gives scene defaults. */
typedef struct rr_render_params {
    int32_t spp;            /* samples per pixel; <= 0: scene */
    int32_t max_bounces;    /* path length cap; < 0: scene */
    float clamp_indirect;   /* max component of indirect contributions; < 0: scene; 0: off */
    uint32_t seed;          /* RNG seed (Cycles "seed") */
    int32_t use_scene_seed; /* != 0: ignore .seed, use the scene's */
    int32_t width;          /* <= 0: scene resolution_x * percentage */
    int32_t height;         /* <= 0: scene resolution_y * percentage */
    int32_t view_transform; /* RR_VIEW_* */
    int32_t spp_per_chunk;  /* samples in flight per wavefront chunk; <= 0: auto */
    int32_t flags;          /* RR_FLAG_* (measurement modes; 0 in production) */
    int32_t max_diffuse_bounces; /* Cycles max_diffuse_bounces (scene default 4); < 0: scene */
    int32_t max_glossy_bounces;  /* Cycles max_glossy_bounces (scene default 4); < 0: scene */
} rr_render_params;

/* Measurement flags (rr_render_params.flags). */
#define RR_FLAG_PROFILE_KERNELS 1  /* HIP events around every launch -> stats.kernel_ms[] */
#define RR_FLAG_COUNT_TRAVERSAL 2  /* count BVH nodes visited / triangles tested -> stats */
#define RR_FLAG_WAVEFRONT 4        /* LDS-resident scenes: the split trace/shade kernels of large scenes
                                    * (quantised BVH4 from HBM) instead of k_tiles (parity: both paths) */

/* Kernel classes of rr_frame_stats.kernel_ms / kernel_launches. */
#define RR_K_BUILD 0     /* world transform + Morton + radix sort + Karras + refit */
#define RR_K_PRIMARY 1   /* bounce 0: raygen + closest hit + shade + queue compaction */
#define RR_K_EXTEND 2    /* bounces >= 1: closest hit + shade + queue compaction */
#define RR_K_SHADOW 3    /* any-hit traversal of shadow rays */
#define RR_K_ACCUM 4     /* film accumulate + tonemap */
#define RR_K_SHADE 5     /* split path (large scenes): shading kernels; PRIMARY/EXTEND then time traversal only */
#define RR_K_TILES 6     /* LDS-resident scenes: k_tiles, every sample of an 8x8 pixel tile run to completion + film + tonemap */
#define RR_K_PNG 7       /* device deflate coder of the frame's format (PNG with rr_set_device_png, 16-bit PNG, or OPEN_EXR), the TARGA packer, the HDR, the IRIS or the WEBP coder: all its kernels, one event pair per frame */
#define RR_K_CLASSES 8

/* The five timestamps the reference recovers from Blender's stdout
 * (PartialRenderStatistics, worker/src/rendering/runner/utilities.rs:14-20,
 * derived at :177-194). UNIX seconds as f64, the serde representation of
 * FrameRenderTime (shared/src/results/worker_trace.rs:13-34). The caller adds
 * started_process_at / exited_process_at around the call exactly as
 * runner/mod.rs:165,176 do. */
typedef struct rr_frame_timing {
    double loaded_at;              /* reference: script start, render-timing-script.py:13 */
    double started_rendering_at;   /* reference: :86 */
    double finished_rendering_at;  /* reference: project_finished_rendering_at - saving (utilities.rs:185-190) */
    double file_saving_started_at; /* == finished_rendering_at (utilities.rs:191-192) */
    double file_saving_finished_at;/* reference: project_finished_rendering_at (utilities.rs:195-198) */
} rr_frame_timing;

/* Per-frame statistics (sidecar metrics; never part of the trace JSON). */
typedef struct rr_frame_stats {
    int32_t width, height, spp, chunks;
    uint64_t camera_rays;    /* camera samples, W * H * spp (camera_rays_traced: those traversed) */
    uint64_t extension_rays; /* continuation rays spawned (closest hit); extension_rays_escaped of them
                              * are resolved without a traversal */
    uint64_t shadow_rays;    /* NEE shadow rays spawned (any hit); shadow_rays_escaped of them are
                              * resolved without a traversal */
    uint64_t primary_continued; /* camera paths that continue past bounce 0 */
    uint64_t primary_shadow;    /* shadow rays spawned at bounce 0 */
    double anim_ms;          /* host animation eval + upload */
    double build_ms;         /* device: world transform + LBVH build (0 if cached) */
    double trace_ms;         /* device: wavefront kernels (raygen .. accumulate) */
    double readback_ms;      /* device->host of the 8-bit image (device JPEG / PNG / EXR: the coder + its stream) */
    double encode_ms;        /* host: JPEG/PNG encode (EXR: container) + write */
    double total_ms;         /* whole call */
    int32_t bvh_rebuilt;     /* 1 if the LBVH was rebuilt for this frame */
    int32_t n_triangles;
    uint64_t output_bytes;   /* encoded file size */
    /* RR_FLAG_PROFILE_KERNELS: summed device time and launch count per class */
    double kernel_ms[RR_K_CLASSES];
    int32_t kernel_launches[RR_K_CLASSES];
    /* RR_FLAG_COUNT_TRAVERSAL: BVH nodes visited / triangles tested over the
     * frame, per traversal kernel: [0] primary, [1] extend, [2] shadow */
    uint64_t trav_nodes[3], trav_tris[3];
    /* camera rays actually traced: camera_rays counts W*H*spp, of which the
     * ones outside the scene's screen rectangle (or meeting no triangle of
     * their tile) are resolved as background without a traversal */
    uint64_t camera_rays_traced;
    int32_t view_transform;            /* RR_VIEW_* the frame was rendered with */
    int32_t view_transform_substituted;/* 1: a view setting was not applied (a view or look without its LUT,
                                        * a look with a view that takes none, an unknown name); rr_last_warning */
    /* RR_FLAG_COUNT_TRAVERSAL, LDS-resident scenes: the shader clock the tile
     * kernel ran at, in GHz, measured inside it (shader-clock ticks over the
     * 100 MHz real-time counter across each wave's lifetime, summed over waves);
     * 0 when not measured */
    double kernel_clock_ghz;
    /* same launch: the waves' mean lifetime over the launch's span (first wave
     * start to last wave end), i.e. how full the persistent grid stayed; 0
     * when not measured */
    double kernel_wave_fill;
    /* LDS-resident scenes (k_tiles): work units per tile of the scene's
     * screen box — 1 when the frame overlapped another k_tiles frame in flight
     * (whole tiles, every sample group of a tile in one unit), the number of
     * 32-sample groups when it ran alone (one unit per group); 0 for frames of
     * the other paths. Scheduling only: both give the same bits. */
    int32_t tile_slices;
    /* traversal-stack pushes dropped for want of room over the frame (each a
     * missed subtree; counted in every frame; 0 on every bench scene) */
    int32_t stack_drops;
    /* LDS-resident scenes (k_tiles): continuation / shadow rays of extension_rays /
     * shadow_rays that leave a hull side of their triangle (every vertex of the
     * scene lies behind that side's plane), so they meet nothing and are
     * resolved without a traversal (the continuation adds the world term, the
     * shadow ray is unoccluded). Rays that entered a traversal =
     * camera_rays_traced + extension_rays - extension_rays_escaped + shadow_rays
     * - shadow_rays_escaped. 0 on the split path (every ray is traversed). */
    uint64_t extension_rays_escaped;
    uint64_t shadow_rays_escaped;
    /* RR_FLAG_COUNT_TRAVERSAL, LDS-resident scenes (with kernel_wave_fill):
     * the spread of the tile kernel's wave starts (last start - first start)
     * and of its wave ends (last end - first end), each over the launch's span;
     * 0 when not measured */
    double kernel_entry_spread;
    double kernel_exit_spread;
} rr_frame_stats;

/* Fill p with "use the scene's value" for every field. */
void rr_render_params_default(rr_render_params* p);

/* Library / ABI version (RR_ABI_VERSION). */
int32_t rr_abi_version(void);

/* Create a renderer context on HIP device `device_ordinal` (index among the
 * devices visible to this process). */
int rr_create(int device_ordinal, rr_ctx** out);

/* Load a scene exported once per project (".rrscene" JSON)
 * and upload its meshes to ctx's device. ctx may be NULL: the handle is then
 * host-only (animation / resolution queries) and binds to the first context
 * that renders it. The reference re-reads the .blend on
 * every frame (runner/mod.rs:142-146); here the scene is parsed and uploaded
 * once and cached in the returned handle. */
int rr_scene_load(rr_ctx* ctx, const char* scene_path, rr_scene** out);

/* Render one frame. Replaces the Blender subprocess of runner/mod.rs:140-174
 * plus scene.frame_set / render(write_still=True) of render-timing-script.py:81-92.
 *  - frame_index: the frame to evaluate (Blender frame number, scene.frame_set).
 *  - out_path: output path WITHOUT extension, '#' runs already substituted
 *    (render-timing-script.py:69-78,82); the library appends ".jpg" / ".png"
 *    / ".exr" / ".tga" / ".hdr" / ".rgb" / ".webp" as Blender's write_still does with
 *    R_EXTENSION. NULL: render only.
 *  - format: "JPEG", "PNG", "OPEN_EXR", "TARGA", "TARGA_RAW", "HDR", "IRIS" or "WEBP" (job output_file_format,
 *    shared/src/jobs/mod.rs:80, handed to image_settings.file_format,
 *    render-timing-script.py:83-92). "OPEN_EXR": the film's mean linear
 *    radiance before any view transform (alpha = 1) as A, B, G, R channels,
 *    ZIP compression in chunks of 16 scanlines, single-part scanline file.
 *    The channels are HALF by default (the means clamped to +-65504 and
 *    rounded to nearest even), or FLOAT (the means' own bits, what
 *    rr_render_frame_to_memory returns) where rr_set_exr_depth or the scene's
 *    render.exr_depth says 32. Coded on the GPU (exr.hip); there is no host
 *    EXR encoder. RR_EINVAL for a width above 2^19 (HALF) or 2^18 (FLOAT), or
 *    a frame of 2 GB and more.
 *    "TARGA" / "TARGA_RAW": the 8-bit image (view settings and dither
 *    applied) as an 18-byte header (type 2 true colour or 3 grey, + 8 for
 *    "TARGA"; bottom-left origin) and the rows bottom first, pixels B, G, R, A
 *    (rr_set_color_mode RGB: B, G, R; BW: the grey code), alpha 255;
 *    "TARGA" in run-length packets that never cross a row (the project's own
 *    choice of packets; any reader returns the same pixels), "TARGA_RAW"
 *    plain. No footer. Always 8 bits a channel: rr_set_png_depth and the
 *    scene's colour depth do not apply. Coded on the GPU (tga.hip).
 *    RR_EINVAL for a width or height above 65535 or a body of 2 GB and more.
 *    "HDR": a Radiance RGBE file of the values a FLOAT "OPEN_EXR" file of the
 *    frame holds (the film's means; no view transform, look, display gamma or
 *    dither; the depth settings and the PNG compression do not apply). The
 *    header "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y <H> +X <W>\n", then the
 *    rows top first: for a width of 8 .. 32767 the bytes 2, 2, W >> 8, W & 255
 *    and the R, G, B and E planes, each run-length coded on its own (run
 *    packets of at most 127, literal packets of at most 128 bytes, runs from 4
 *    bytes); any other width flat quads. No alpha: RGBA and no mode write RGB;
 *    BW writes R = G = B = the Rec.709 luma of the means. Quads truncate, by
 *    integer shifts of the floats' bits; the rule and the packets are the
 *    project's own (csrc/hdr_rule.h) and unpinned against Blender's files: any
 *    reader returns the same quads from either packing. Coded on the GPU
 *    (hdr.hip). RR_EINVAL for a body bound of 2 GB and more.
 *    "IRIS": a Silicon Graphics image file (.rgb) of the 8-bit image that
 *    "TARGA" takes (view settings and dither applied; always 8 bits a channel:
 *    the depth settings and the PNG compression do not apply), every number
 *    big-endian: a 512-byte header (magic 474, run-length coded, a byte a
 *    channel, dimension 2 for one channel else 3, W, H, C, pixmin 0, pixmax
 *    255, the rest 0), a start and a length table of H C uint32 entries each
 *    (entry y + z H: file row y of channel z, its offset in the file and its
 *    coded bytes), then the coded row-planes, file row 0 (the image's bottom
 *    row) first and within a row channel 0 .. C - 1. Channels R, G, B, A with
 *    alpha 255 (rr_set_color_mode RGB: R, G, B; BW: the grey code). A run
 *    packet is the byte n and a value, a literal packet 0x80 | n and n bytes,
 *    n at most 127, runs from 3 equal bytes; a 0 byte ends every row-plane.
 *    Packets and the order of the row-planes are the project's own choice
 *    (csrc/iris_rule.h), unpinned against Blender's files: any reader goes
 *    through the tables and returns the same pixels. Coded on the GPU
 *    (iris.hip). RR_EINVAL for a width or height above 65535 or a body bound
 *    (tables and row-planes at their longest) of 2 GB and more.
 *    "WEBP": a lossless WebP file (.webp) of the same 8-bit image: a RIFF
 *    container with one VP8L chunk, always 8 bits a channel. The payload, an
 *    LSB-first bit stream: byte 0x2F, W - 1 and H - 1 in 14 bits each, the
 *    alpha hint (1 with four channels: rr_set_color_mode RGBA or none; RGB:
 *    alpha 255, hint 0; BW: the grey code in R, G and B, hint 0), version 0;
 *    the subtract-green transform; the predictor transform with mode 1 (the
 *    left neighbour) in every block; no colour cache, no meta prefix codes;
 *    five prefix codes; literals, and copies of 3 .. 4096 equal residuals at
 *    distance 1 within a row. Pinned: the pixels, which libwebp returns
 *    exactly, and the bytes against a restatement of the writer. The run rule
 *    and the single predictor mode are the project's own (csrc/webp_rule.h):
 *    any reader returns the same pixels. Blender writes lossy VP8 below quality
 *    100: that is not built. jpeg_quality below 100 gives the same lossless
 *    file and sets rr_last_warning, naming the quality; the frame does not
 *    fail. Coded on the GPU (webp.hip). RR_EINVAL for a width or height above
 *    16384 or a payload bound (60 bits a pixel and the header) of 2 GB and
 *    more.
 *  - jpeg_quality: 1..100 (the reference script forces 90, :84); "WEBP": below
 *    100 flagged, see above; ignored for every other format.
 *  - timing / stats: optional outputs (may be NULL). */
int rr_render_frame(rr_ctx* ctx, rr_scene* scene, int32_t frame_index,
                    const rr_render_params* params, const char* out_path,
                    const char* format, int32_t jpeg_quality,
                    rr_frame_timing* timing, rr_frame_stats* stats);

/* Two-phase form of rr_render_frame, for a worker that keeps its next queued
 * frame in flight (eager-naive-coarse and dynamic keep
 * frames queued per worker, master/src/cluster/strategies.rs:70-150,250-405,
 * while the reference worker renders them strictly one after another,
 * worker/src/rendering/queue.rs:79-118). rr_frame_submit evaluates the
 * animation, enqueues the frame's device work and returns without waiting;
 * rr_frame_complete waits for that frame's device work, encodes and writes
 * the image and fills timing/stats exactly as rr_render_frame does. The
 * intended loop is submit(N+1), complete(N): the host encodes and writes
 * frame N while the GPU renders N+1. At most RR_MAX_FRAMES_IN_FLIGHT frames
 * may be pending (RR_EBUSY otherwise); they complete in submission order.
 * Each pending frame has its own stream: with three pending, frame N+2's
 * device work is queued while N+1 renders, and starts on the CUs N+1 leaves
 * idle before N's JPEG kernels (waiting behind N+1) have let the host
 * complete N.
 * rr_render_frame == submit + complete. Same arguments and errors as
 * rr_render_frame; a failed complete still retires its ticket. */
int rr_frame_submit(rr_ctx* ctx, rr_scene* scene, int32_t frame_index,
                    const rr_render_params* params, const char* out_path,
                    const char* format, int32_t jpeg_quality, uint64_t* ticket);
int rr_frame_complete(rr_ctx* ctx, uint64_t ticket, rr_frame_timing* timing,
                      rr_frame_stats* stats);

/* Several files from one rendered frame: the frame is traced once, its film
 * stays on the device, and every output is coded from it. An output is what
 * rr_frame_submit's (out_path, format, jpeg_quality) name, and goes through
 * the context's and the scene's depth, colour mode, codec, PNG compression and
 * dither settings on its own (JPEG beside an RGBA PNG: three components beside
 * four). reduce: 1, or 2, 4 or 8 for a proxy: the file then holds the frame
 * reduced by that factor, ceil(W / reduce) x ceil(H / reduce) pixels, each the
 * box mean of its block of the film (partial blocks at the right and bottom
 * edges average the pixels they have; float32 sums in row order, so the
 * result is reproducible bit for bit). An 8-bit output of a factor is the
 * view pass (exposure, view transform, look, gamma, dither keyed on its own
 * pixel coordinates) over the reduced film; "OPEN_EXR", "HDR" and 16-bit "PNG"
 * read the reduced film itself. Outputs of one factor share its film.
 *
 * rr_frame_submit(path, format, q) is rr_frame_submit_outputs with the one
 * output {path, format, q, 1}, and rr_frame_complete completes a frame of
 * several outputs as any other; a file that cannot be written is RR_EIO naming
 * it, and the frame's other files are written all the same. rr_frame_timing
 * and rr_frame_stats keep their meaning; stats.output_bytes is outs[0]'s, and
 * rr_last_output_bytes gives every file's size of the frame completed last
 * (RR_EINVAL for an index that frame did not have).
 *
 * Refused before anything is launched or written: n outside 1 ..
 * RR_MAX_FRAME_OUTPUTS, a reduce other than 1, 2, 4, 8, or two outputs of one
 * file name (RR_EINVAL, naming the file); a format nobody writes (RR_ENOTSUP,
 * rr_frame_submit's text); a size outside a coder's range, judged at the
 * output's reduced size (RR_EINVAL, the coder's text: a proxy can bring a
 * frame into a coder's range). Two JPEG outputs may differ in quality: the
 * context keeps the transform's table of every quality it has been asked for.
 * rr_last_warning joins the outputs' warnings in output order.
 *
 * What a context adds (rr_set_extra_outputs) or a scene (render.use_preview)
 * counts towards RR_MAX_FRAME_OUTPUTS. */
#define RR_MAX_FRAME_OUTPUTS 4
typedef struct rr_frame_output {
    const char* out_path;   /* without extension, as rr_frame_submit takes it */
    const char* format;     /* "JPEG", "PNG", ...: a format rr_render_frame writes */
    int32_t jpeg_quality;   /* as rr_frame_submit's */
    int32_t reduce;         /* 1, 2, 4 or 8 */
} rr_frame_output;
int rr_frame_submit_outputs(rr_ctx* ctx, rr_scene* scene, int32_t frame_index,
                            const rr_render_params* params, const rr_frame_output* outs,
                            int32_t n, uint64_t* ticket);
/* submit + complete, as rr_render_frame is */
int rr_render_frame_outputs(rr_ctx* ctx, rr_scene* scene, int32_t frame_index,
                            const rr_render_params* params, const rr_frame_output* outs,
                            int32_t n, rr_frame_timing* timing, rr_frame_stats* stats);
int rr_last_output_bytes(rr_ctx* ctx, int32_t index, uint64_t* bytes);

/* Files every frame of ctx that is submitted with a path writes beside its
 * own, for callers that cannot be changed (the Blender-CLI shim under the
 * reference worker). spec: "FORMAT[:K]" entries joined by commas, e.g.
 * "JPEG:4,PNG": a format name and a factor 1 (also when left out), 2, 4 or 8,
 * at most RR_MAX_FRAME_OUTPUTS - 1 entries. An entry of factor 1 writes
 * <out_path><ext>, one of factor K <out_path>.r<K><ext>, with the frame's
 * jpeg_quality. NULL or "": none. RR_EINVAL for a spec that does not parse,
 * which changes nothing; a frame whose own file an entry would overwrite is
 * refused when it is submitted (RR_EINVAL, as above). Also read from
 * RR_EXTRA_OUTPUTS by rr_create, like the other RR_* output settings.
 *
 * A scene may carry render.use_preview (Blender's image_settings.use_preview,
 * exported only when set): on a context without extra outputs an "OPEN_EXR"
 * frame of it also writes <out_path>.jpg, a JPEG of the frame's quality at
 * factor 1. Not pinned: what Blender writes for that setting, and where, is
 * recalled from memory. */
int rr_set_extra_outputs(rr_ctx* ctx, const char* spec);

/* The box mean of a reduced output (csrc/reduce_rule.h) of a w x h image of 4
 * floats a pixel, into out: ceil(w / reduce) x ceil(h / reduce) pixels. With
 * a context the device kernel runs (k_film_reduce), with ctx NULL the host's
 * statement of the same rule; reduce 1, 2, 4 or 8. */
int rr_debug_film_reduce(rr_ctx* ctx, const float* rgba, int32_t w, int32_t h, int32_t reduce,
                         float* out /* ceil(w/reduce) * ceil(h/reduce) * 4 */);

/* The render region: Blender's render border. Frames of ctx render and write
 * a rectangle of the frame instead of all of it. Off on a new context.
 *
 * rr_set_region: x0 <= x < x1, y0 <= y < y1 (half open) in pixels of the full
 * frame, rows top first. x0 < x1 and y0 < y1, each within +-2^30, else RR_EINVAL, which
 * changes nothing. The rectangle is clamped to the frame when a frame is
 * submitted; one that lies outside it altogether refuses that frame
 * (RR_EINVAL, naming the region and the frame's size) before anything is
 * launched. A region that covers the whole frame is the frame without a
 * region, byte for byte. rr_set_region_off turns it off. Read when a frame is
 * submitted, as the other settings are; frames in flight keep theirs.
 *
 * crop != 0: every output (each file, a reduced one before its reduction, the
 * images of rr_render_frame_to_memory) is the region's w x h pixels. crop 0:
 * the full frame, (0, 0, 0, 0) outside the region: RGB 0 in every format, and
 * A = 0 outside and opaque inside in the files that carry alpha (RGBA TARGA,
 * IRIS, WEBP, PNG at 8 and 16 bits, OPEN_EXR A), black in those that do not
 * (JPEG, HDR).
 *
 * Inside the region every value of every format and depth is the bits the
 * same frame has there when rendered whole: each pixel's samples are keyed on
 * its full-frame coordinates. The exception is the dither (rr_set_dither),
 * Blender's noise keyed on the OUTPUT image's own pixel coordinates as for the
 * reduced proxies, so a cropped 8-bit file with dither on is not a window of
 * the full frame's file. `reduce` and the extra outputs apply to the windowed
 * image.
 *
 * The split path (large scenes, RR_FLAG_WAVEFRONT) traces the region's pixels
 * alone; the tile path (k_tiles) runs the 8 x 8 tiles that meet the region,
 * partial tiles whole, and drops their pixels outside it. rr_frame_stats
 * describes what ran: camera_rays and the ray counters are the region's on
 * the split path, and on the tile path those of the tiles that ran (partial
 * tiles count whole); width and height stay the frame's.
 *
 * rr_set_region_from_scene(ctx, 1): a scene's render.border {min_x, max_x,
 * min_y, max_y, crop} (Blender's fractions, y from the bottom; exported only
 * with use_border set) gives the region of its frames and comes before
 * rr_set_region's; a scene without one leaves that in force. The pixel rule
 * (csrc/region_rule.h) is recalled, not pinned against a Blender.
 *
 * RR_REGION, read by rr_create: "x0,y0,x1,y1[,crop]", "scene", or "" (off).
 *
 * rr_region_resolution: the size of the files and of
 * rr_render_frame_to_memory's images for a frame of scene with params on ctx:
 * the region's with crop, else the frame's (rr_scene_resolution, unchanged). */
int rr_set_region(rr_ctx* ctx, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t crop);
int rr_set_region_off(rr_ctx* ctx);
int rr_set_region_from_scene(rr_ctx* ctx, int32_t on);
int rr_region_resolution(rr_ctx* ctx, rr_scene* scene, const rr_render_params* params,
                         int32_t* width, int32_t* height);

/* k_film_window (csrc/region.hip) on a w x h image of 4 floats a pixel: with
 * crop the (x1 - x0) x (y1 - y0) window, else the w x h image with zeros
 * outside it; inside, the image's x, y, z and w = alpha_sum. The region must
 * lie inside the image and hold a pixel (RR_EINVAL). */
int rr_debug_film_window(rr_ctx* ctx, const float* rgba, int32_t w, int32_t h, int32_t x0, int32_t y0,
                         int32_t x1, int32_t y1, int32_t crop, float alpha_sum, float* out);

/* Wait until every piece of device work ctx has enqueued (frames in flight
 * included) has finished; their tickets still have to be completed. */
int rr_synchronize(rr_ctx* ctx);

/* Render one frame into caller memory (no file). film_rgba: W*H*4 floats of
 * mean linear radiance (alpha = 1); rgba8: W*H*4 bytes after the view
 * transform. Either may be NULL. Rows are top to bottom. */
int rr_render_frame_to_memory(rr_ctx* ctx, rr_scene* scene, int32_t frame_index,
                              const rr_render_params* params, float* film_rgba,
                              uint8_t* rgba8, rr_frame_stats* stats);

/* Resolved output size for these params (after scene defaults). */
int rr_scene_resolution(rr_scene* scene, const rr_render_params* params,
                        int32_t* width, int32_t* height);

/* Encode an RGBA8 image (rows top to bottom) to `path` + extension.
 * Host encoder used by rr_render_frame; exported for tests. "JPEG", "PNG",
 * "TARGA", "TARGA_RAW", "IRIS" (four channels, as "PNG"; RR_EINVAL for a width
 * or height above 65535 or a body of 2 GB and more) and "WEBP" (four channels;
 * RR_EINVAL above 16384; lossless, and a jpeg_quality below 100 sets the
 * warning rr_last_warning(NULL) returns on this thread until the next host
 * encode): "OPEN_EXR" and "HDR" need the float film and are RR_ENOTSUP here. */
int rr_encode_image(const uint8_t* rgba8, int32_t width, int32_t height,
                    const char* out_path_no_ext, const char* format,
                    int32_t jpeg_quality, uint64_t* bytes_written);

/* Encode an RGBA8 image with the device JPEG path (forward DCT + Huffman
 * coding on the GPU, jpeg.hip; the path rr_render_frame takes for "JPEG").
 * *len receives the file size; the bytes are copied to out if cap >= *len.
 * Exported for parity tests against rr_encode_image. */
int rr_debug_jpeg_device(rr_ctx* ctx, const uint8_t* rgba8, int32_t width, int32_t height,
                         int32_t jpeg_quality, uint8_t* out, uint64_t cap, uint64_t* len);

/* Select the device PNG encoder for "PNG" frames of ctx (on != 0): Sub filter,
 * LZ77 and dynamic-Huffman deflate run on the GPU after the view transform
 * (png.hip, deflate.hip), only the zlib stream crosses PCIe and the host writes the chunk
 * framing — instead of the 8-bit image's readback and the zlib threads of
 * rr_encode_image. Replaces the PNG side of Blender's write_still
 * (render-timing-script.py:83-92). Off by default; rr_create reads
 * RR_DEVICE_PNG=1 from the environment the same way. The files decode to the
 * same pixels either way; their bytes differ. Applies to frames submitted
 * after the call. RR_EINVAL for a NULL ctx. */
int rr_set_device_png(rr_ctx* ctx, int32_t on);

/* Encode an RGBA8 image with the device PNG path (the one rr_set_device_png
 * selects for rendered frames; write_still, render-timing-script.py:83-92).
 * *len receives the file size; the bytes are copied to out if cap >= *len.
 * Exported for round-trip tests. */
int rr_debug_png_device(rr_ctx* ctx, const uint8_t* rgba8, int32_t width, int32_t height,
                        uint8_t* out, uint64_t cap, uint64_t* len);

/* Encode a float RGBA image (rows top to bottom, width * height * 4 floats,
 * taken as means: spp = 1, alpha from the image) with the device OpenEXR path
 * (the one "OPEN_EXR" frames take; write_still, render-timing-script.py:83-92).
 * *len receives the file size; the bytes are copied to out if cap >= *len.
 * Exported for round-trip tests. */
int rr_debug_exr_device(rr_ctx* ctx, const float* rgba, int32_t width, int32_t height,
                        uint8_t* out, uint64_t cap, uint64_t* len);

/* Bit depth of "PNG" frames of ctx: 0 = the scene's render.color_depth (8 when
 * the scene has none; the default), 8 or 16 = that depth. Replaces Blender's
 * image_settings.color_depth behind write_still (render-timing-script.py:83-92).
 * A 16-bit frame is RGBA with 16-bit samples, quantised from the float film
 * after exposure and view transform (not from the 8-bit image), and is always
 * coded on the device (png16.hip), whatever rr_set_device_png says: there is no
 * host 16-bit encoder, and rr_encode_image stays 8-bit. 8-bit PNG, JPEG and
 * OPEN_EXR frames are unaffected. rr_create reads RR_PNG_DEPTH (0, 8 or 16)
 * from the environment the same way. Applies to frames submitted after the
 * call. A 16-bit frame wider than 2^19 pixels, or with a stream of 2 GB and
 * more, is refused with RR_EINVAL when submitted. RR_EINVAL for a NULL ctx or
 * another depth. */
int rr_set_png_depth(rr_ctx* ctx, int32_t depth);

/* Encode a float RGBA image (rows top to bottom, width * height * 4 floats,
 * taken as means: spp = 1; alpha is forced to 1) with the device 16-bit PNG
 * path (the one 16-bit "PNG" frames take; write_still,
 * render-timing-script.py:83-92): value * exposure_scale, clamp to [0, 1],
 * view_transform (RR_VIEW_STANDARD, RR_VIEW_RAW, or one of the Filmic family
 * with the context's LUTs and look; a view or look without its LUT is
 * RR_EINVAL here), the context's display gamma, 16-bit quantisation,
 * Sub filter, deflate. *len receives the file size; the bytes are copied to out
 * if cap >= *len. Exported for round-trip tests. */
int rr_debug_png16_device(rr_ctx* ctx, const float* rgba, int32_t width, int32_t height,
                          int32_t view_transform, float exposure_scale, uint8_t* out, uint64_t cap,
                          uint64_t* len);

/* Channel type of "OPEN_EXR" frames of ctx: 0 = the scene's render.exr_depth
 * (16 when the scene has none; the default), 16 = HALF, 32 = FLOAT. Replaces
 * Blender's image_settings.color_depth for OpenEXR, "Float (Half)" / "Float
 * (Full)", behind write_still (render-timing-script.py:83-92). A FLOAT file
 * holds the film's means bit for bit: no clamp, no rounding, subnormals kept;
 * the layout is otherwise the HALF file's (ZIP, 16 scanlines a chunk), coded on
 * the device (exr.hip) with chunks of twice the bytes. HALF stays the default
 * although Blender itself picks 32 when a project of another depth is switched
 * to OpenEXR. PNG and JPEG frames are unaffected. rr_create reads RR_EXR_DEPTH
 * (0, 16 or 32) from the environment the same way. Applies to frames submitted
 * after the call. A FLOAT frame wider than 2^18 pixels, or with a stream of
 * 2 GB and more, is refused with RR_EINVAL when submitted. RR_EINVAL for a
 * NULL ctx or another depth. */
int rr_set_exr_depth(rr_ctx* ctx, int32_t depth);

/* rr_debug_exr_device with FLOAT channels (the path rr_set_exr_depth 32
 * selects): spp = 1, alpha from the image; the file holds the floats given.
 * *len receives the file size; the bytes are copied to out if cap >= *len.
 * Exported for round-trip tests. */
int rr_debug_exr32_device(rr_ctx* ctx, const float* rgba, int32_t width, int32_t height,
                          uint8_t* out, uint64_t cap, uint64_t* len);

/* Colour mode of the files of ctx: Blender's image_settings.color_mode behind
 * write_still (render-timing-script.py:83-92). RR_COLOR_SCENE: the scene's
 * render.color_mode ("BW", "RGB" or "RGBA"), and where the scene has none the
 * layout each format had before there was a setting: JPEG three components,
 * PNG RGBA, OPEN_EXR A, B, G, R. The values of the others are the channels the
 * file holds.
 *  - RR_COLOR_RGBA: alpha is 1 (255 / 65535 / 1.0). JPEG has no alpha and
 *    writes RGB, as Blender does.
 *  - RR_COLOR_RGB: PNG colour type 2; OPEN_EXR channels B, G, R.
 *  - RR_COLOR_BW: Rec.709 luma, l = 0.2126 r + 0.7152 g + 0.0722 b, each
 *    product and sum a float32 operation of its own, left to right. 8-bit
 *    files (JPEG, 8-bit PNG) take it of the RGBA8 image after the view
 *    transform, c / 255 a channel: code 0 for l <= 0, 255 for l > 1 - 0.5/255,
 *    else (uint8)(255 l + 0.5). 16-bit PNG takes it of the display-referred
 *    floats before quantisation; OPEN_EXR of the film's linear means, into one
 *    channel "Y". PNG colour type 0; JPEG a single-component baseline file
 *    with 8x8 MCUs whose Y is the grey code (not the JFIF 0.299/0.587/0.114
 *    mix).
 * rr_create reads RR_COLOR_MODE ("BW", "RGB", "RGBA" or empty) from the
 * environment the same way. Applies to frames submitted after the call; frames
 * in flight keep the mode of their submit. RR_EINVAL for a NULL ctx or another
 * value. */
#define RR_COLOR_SCENE 0
#define RR_COLOR_BW 1
#define RR_COLOR_RGB 3
#define RR_COLOR_RGBA 4
int rr_set_color_mode(rr_ctx* ctx, int32_t mode);

/* rr_encode_image in a colour mode (RR_COLOR_SCENE: rr_encode_image's own
 * files). "JPEG": BW or RGB (RGBA writes RGB); "PNG": colour types 0 / 2 / 6. */
int rr_encode_image_mode(const uint8_t* rgba8, int32_t width, int32_t height,
                         const char* out_path_no_ext, const char* format,
                         int32_t jpeg_quality, int32_t color_mode, uint64_t* bytes_written);

/* Encode an image of the caller's with the device coder of a format, depth and
 * colour mode, through the enqueue, wrap and file code rendered frames take.
 * format "JPEG" (depth 8), "PNG" at depth 8 and "TARGA" / "TARGA_RAW" / "IRIS" / "WEBP" (depth 8
 * and no other) take an RGBA8 image (image_is_float 0); "PNG" at depth 16, "OPEN_EXR" at depth 16 (HALF) or 32
 * (FLOAT) and "HDR" (depth 32 and no other) take width * height * 4 floats
 * (image_is_float 1) as means, spp = 1, alpha 1. depth 0: 8 for PNG, TARGA, IRIS and WEBP,
 * 16 for OPEN_EXR, 32 for HDR. view_transform and
 * exposure_scale: 16-bit PNG only, as for rr_debug_png16_device; jpeg_quality:
 * JPEG only. A size outside the coder's range is RR_EINVAL before anything is
 * launched. *len receives the file size; the bytes are copied to out if
 * cap >= *len. Exported for round-trip tests. */
int rr_debug_encode_device(rr_ctx* ctx, const char* format, int32_t depth, int32_t color_mode,
                           const void* image, int32_t image_is_float, int32_t width, int32_t height,
                           int32_t view_transform, float exposure_scale, int32_t jpeg_quality,
                           uint8_t* out, uint64_t cap, uint64_t* len);

/* The host "HDR" coder (no context, no device needed), the reference for the
 * device coder's bytes: the Radiance RGBE file of width * height * 4 floats
 * taken as means (alpha ignored), in color_mode (RR_COLOR_SCENE and
 * RR_COLOR_RGBA: RGB; RR_COLOR_BW: R = G = B = luma). *bytes receives the file
 * size; the bytes are copied to out if cap >= *bytes. RR_EINVAL for a body
 * bound of 2 GB and more. Exported for tests. */
int rr_debug_hdr_host(const float* rgba, int32_t width, int32_t height, int32_t color_mode,
                      uint8_t* out, uint64_t cap, uint64_t* bytes);

/* The sRGB table of the 16-bit PNG path (host only, no device needed): *n
 * receives the number of floats (intervals + 1), which are copied to table if
 * cap >= *n. Entry i = 1.055 (i / (n - 1))^(1 / 2.4) - 0.055, computed in
 * double. Exported so that tests restate the table read, not the table. */
int rr_debug_srgb16_table(float* table, int32_t cap, int32_t* n);

/* Thread-local message of the last failure on this thread (ctx may be NULL). */
const char* rr_last_error(rr_ctx* ctx);

/* Warning of ctx's last completed frame ("" if none), e.g. a Filmic view
 * transform rendered as Standard because no OCIO LUTs are configured. Valid
 * until the next call on ctx. ctx NULL: the warning of this thread's last host
 * encode (rr_encode_image, rr_encode_image_mode), "" if none. */
const char* rr_last_warning(rr_ctx* ctx);

/* Blender colour-management directory (datafiles/colormanagement: config.ocio
 * and luts/) whose Filmic LUTs (filmic_desat65cube.spi3d,
 * filmic_to_0-70_1-03.spi1d) implement RR_VIEW_FILMIC and RR_VIEW_FILMIC_LOG
 * on ctx. NULL or "": no LUTs (frames of the Filmic family fall back to
 * Standard, flagged). The looks' curves (filmic_to_1.20_1-00.spi1d,
 * filmic_to_0.99_1-0075.spi1d, filmic_to_0-85_1-011.spi1d,
 * filmic_to_0-60_1-04.spi1d, filmic_to_0-48_1-09.spi1d,
 * filmic_to_0-35_1-30.spi1d) and filmic_false_color.spi3d are loaded from the
 * same place when present; an absent one only makes its look or view
 * unavailable. rr_create reads the RR_OCIO_DIR environment variable the same
 * way. RR_ENOENT / RR_EINVAL if the two base files are missing or any file
 * found is malformed (ctx keeps no LUTs then). */
int rr_set_ocio_config(rr_ctx* ctx, const char* dir);

/* The look of ctx's Filmic frames (Blender's view_settings.look): "None",
 * "Very High Contrast", "High Contrast", "Medium High Contrast", "Medium
 * Contrast", "Medium Low Contrast", "Low Contrast", "Very Low Contrast", each
 * also with Blender's "Filmic - " prefix. NULL or "": the scene's render.look.
 * A look puts its 1D curve in the place of Filmic's base curve ("Medium
 * Contrast" is the base curve: the bits of "None"). With a view other than
 * RR_VIEW_FILMIC the look is ignored, and with its curve's file not loaded the
 * frame renders without the look; both are flagged
 * (view_transform_substituted, rr_last_warning). rr_create reads RR_LOOK from
 * the environment the same way. Applies to frames submitted after the call
 * and to rr_debug_view_device / rr_debug_png16_device /
 * rr_debug_encode_device; frames in flight keep theirs. RR_EINVAL for a NULL
 * ctx or an unknown name. */
int rr_set_look(rr_ctx* ctx, const char* name);

/* Display gamma of ctx's frames (Blender's view_settings.gamma), for every
 * view transform: after the view transform d' = d^(1 / gamma), 0 for d <= 0,
 * by fixed polynomials of log2 and exp2 (the same bits on host and device),
 * before BW luma and quantisation. 0: the scene's render.gamma. 1 skips the
 * step. OPEN_EXR files are linear and unaffected. rr_create reads
 * RR_DISPLAY_GAMMA from the environment the same way. Applies as rr_set_look
 * does. RR_EINVAL for a NULL ctx, gamma < 0 or gamma > 5 (Blender's range). */
int rr_set_display_gamma(rr_ctx* ctx, float gamma);

/* Dither of ctx's 8-bit images (Blender's image_settings.dither_intensity
 * behind write_still, render-timing-script.py:83-92): noise added to the
 * display-referred values, after the view transform and the display gamma,
 * before they are quantised to bytes. For the pixel in column x (0 = left) and
 * row r (0 = top) of a W x H frame, with intensity g:
 *   yb = H - 1 - r                      (Blender's rows run bottom-up)
 *   s = (float)x * (1.0f / (float)W),  t = (float)yb * (1.0f / (float)H)
 *   h0 = fract(sin_fixed(s * 12.9898f + t * 78.233f) * 43758.5453f)
 *   h1 = fract(sin_fixed(s * 19.9898f + t * 119.233f) * 798.5453f)
 *   n = h0 + h1 - 0.5f                  (triangle-shaped, in [-0.5, 1.5))
 *   code_k = quantize8(d_k + n * 0.0033f * g)   the same n for R, G, B; alpha 255
 * each product and sum a float32 operation of its own, left to right, and
 * sin_fixed a sine of fixed float32 operations (rr_debug_sin_fixed), so host
 * and device give the same bits. The rule is restated from Blender 3.6's
 * imbuf and not pinned against Blender's own files.
 * intensity: a value in [0, 2] (Blender's range; 0: none), or RR_DITHER_SCENE
 * for the scene's render.dither_intensity (0 where the scene has none). A new
 * context's value is 0 whatever the scene says. It applies to whatever the
 * 8-bit image feeds: JPEG files, 8-bit PNG files (host and device coder,
 * BW luma included, which is taken of the dithered image), the rgba8 of
 * rr_render_frame_to_memory and rr_debug_view_device (where RR_DITHER_SCENE
 * means none). 16-bit PNG and OPEN_EXR files are not dithered. A frame with an
 * intensity above 0 takes the view pass whatever its view; at 0 a frame's
 * device work is what it was before there was a setting. rr_create reads
 * RR_DITHER (a number, or "scene") from the environment the same way. Applies
 * to frames submitted after the call; frames in flight keep theirs. RR_EINVAL
 * for a NULL ctx, NaN or any other value. */
#define RR_DITHER_SCENE (-1.0f)
int rr_set_dither(rr_ctx* ctx, float intensity);

/* The n of rr_set_dither for every pixel of a w x h image, evaluated on the
 * host (no device needed; write_still's dither, render-timing-script.py:83-92):
 * out receives w * h floats, rows top to bottom. RR_EINVAL for a NULL out or a
 * size below 1. Exported for tests. */
int rr_debug_dither_noise(int32_t w, int32_t h, float* out /* w*h, rows top to bottom */);

/* out[i] = sin_fixed(in[i]), the sine of rr_set_dither (write_still's dither,
 * render-timing-script.py:83-92), evaluated on the host: the argument less the
 * nearest multiple of pi/2 (pi/2 in three parts), then a polynomial of sin or
 * cos on [-pi/4, pi/4]. Within 2^-18 of sin for |in[i]| <= 256 (the dither's
 * arguments stay below 139.3); 0 for |in[i]| > 8192 and NaN. Exported for
 * tests. */
int rr_debug_sin_fixed(const float* in, uint64_t n, float* out);

/* Compression of ctx's "PNG" files: Blender's image_settings.compression
 * behind write_still (render-timing-script.py:83-92), a percentage 0 .. 100
 * (Blender's default is 15).
 *  - RR_PNG_COMPRESSION_LEGACY (the default): the files as they were before
 *    there was a setting: filter type 1 (Sub) on every row, the host coder at
 *    zlib level 1. Byte for byte.
 *  - RR_PNG_COMPRESSION_SCENE: the scene's render.png_compression; legacy
 *    where the scene has none.
 *  - 0 .. 100: every row takes libpng's adaptive filter, which Blender leaves
 *    at libpng's default: for byte x of a row with a the byte one pixel before
 *    it, b the byte above it in the image and c the byte above a (0 where
 *    absent), the residuals mod 256 of type 0 None x, 1 Sub x - a, 2 Up x - b,
 *    3 Average x - ((a + b) >> 1), 4 Paeth x - paeth(a, b, c); a type's score is
 *    the sum over the row of r < 128 ? r : 256 - r; the row takes the smallest,
 *    types tried in the order 0 .. 4, a later one only when strictly smaller
 *    (in an image of one row or one pixel's width Average is not tried, as in
 *    libpng, which leaves out the types whose neighbours such an image lacks).
 *    In all three PNG coders (host, device 8-bit, device 16-bit), at both
 *    depths and in every colour mode. The rule is pinned against libpng
 *    1.6.37's own files; that Blender 3.6 links a libpng with this default is
 *    not pinned.
 *    The host coder deflates at Blender's zlib level, (int)(percent /
 *    11.1111f) clamped to 0 .. 9 (a formula restated from memory): 0 writes
 *    stored blocks. The device coders have one effort level: 0 .. 100 all give
 *    the adaptive filters in front of the coder as it is, so a device-coded
 *    file at 0 is smaller than Blender's and decodes to the same pixels.
 * JPEG and OPEN_EXR files are unaffected. rr_create reads RR_PNG_COMPRESSION
 * (a number, or "scene") from the environment the same way; a bad value fails
 * rr_create with RR_EINVAL. Applies to frames submitted after the call and to
 * rr_debug_encode_device / rr_debug_png_device / rr_debug_png16_device (where
 * RR_PNG_COMPRESSION_SCENE means legacy); frames in flight keep theirs.
 * RR_EINVAL for a NULL ctx or any other value. */
#define RR_PNG_COMPRESSION_LEGACY (-1)
#define RR_PNG_COMPRESSION_SCENE (-2)
int rr_set_png_compression(rr_ctx* ctx, int32_t percent);

/* rr_encode_image_mode's "PNG" with a compression setting (write_still,
 * render-timing-script.py:83-92): the host coder of rr_set_png_compression.
 * compression 0 .. 100, or RR_PNG_COMPRESSION_LEGACY for rr_encode_image_mode's
 * bytes; RR_PNG_COMPRESSION_SCENE is RR_EINVAL here. */
int rr_encode_image_png(const uint8_t* rgba8, int32_t width, int32_t height,
                        const char* out_path_no_ext, int32_t color_mode,
                        int32_t compression, uint64_t* bytes_written);

/* The filter type rr_set_png_compression's rule gives every row of an image
 * of `rows` raw scanlines of row_bytes bytes, bpp bytes a pixel (1 .. 8),
 * evaluated on the host (no device needed; write_still's PNG filter,
 * render-timing-script.py:83-92). Exported so that tests tie the C statement
 * to numpy and to libpng. RR_EINVAL for a NULL array or a size below 1. */
int rr_debug_png_filters(const uint8_t* raw, int32_t row_bytes, int32_t rows,
                         int32_t bpp, uint8_t* types /* rows */);

/* The compression a scene file asks for (host only; write_still's
 * image_settings.compression, render-timing-script.py:83-92): 0 .. 100, or
 * RR_PNG_COMPRESSION_LEGACY for a scene without render.png_compression. */
int rr_debug_scene_png_compression(rr_scene* scene, int32_t* compression);

/* Compression of ctx's "OPEN_EXR" files: Blender's image_settings.exr_codec
 * behind write_still (render-timing-script.py:83-92).
 *  - RR_EXR_CODEC_SCENE (the default): the scene's render.exr_codec (one of
 *    Blender's names "NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44",
 *    "B44A", "DWAA", "DWAB"), and ZIP where the scene has none: the files as
 *    they were before there was a setting, byte for byte.
 *  - RR_EXR_CODEC_ZIP: zlib over chunks of 16 scanlines (exr.hip).
 *  - RR_EXR_CODEC_NONE: a chunk per scanline, its planes (A, B, G, R / B, G, R
 *    / Y) as little-endian halfs or floats, unprocessed.
 *  - RR_EXR_CODEC_RLE: a chunk per scanline; its n bytes reordered (even-
 *    indexed bytes first) and differenced as for ZIP, then run-length packets:
 *    the byte count - 1 (0 .. 127) and a value for a run of count bytes, the
 *    byte -count (as a signed char, count 1 .. 127) and count bytes for a
 *    literal. Runs start from 3 equal bytes. A scanline whose packets are not
 *    shorter than n is stored as its n unprocessed bytes.
 *  - RR_EXR_CODEC_PXR24: zlib over chunks of 16 scanlines of byte planes of
 *    differences between neighbouring pixels: HALF channels their 16 bits
 *    (lossless), FLOAT channels rounded to 24 bits (sign, exponent, 15
 *    mantissa bits; lossy, as in OpenEXR). A chunk whose stream is not smaller
 *    than its unprocessed scanlines is stored as those: full floats at FLOAT.
 *  - RR_EXR_CODEC_ZIPS, _PIZ, _B44, _B44A, _DWAA, _DWAB: not built. The file
 *    is written as ZIP, which is lossless and which every reader reads, and
 *    rr_last_warning names the codec asked for. The frame never fails.
 * NONE, RLE and PXR24 are coded on the device (exr_codec.hip, exr.hip), at
 * both depths and in every colour mode; the sizes refused are those of ZIP at
 * the same depth. Pinned: the file structure, OpenEXR's decoder contract (a
 * negative count copies -count bytes, otherwise count + 1 copies of the next
 * byte; a chunk of the raw size is raw) and the bytes against a numpy
 * restatement. Not pinned (no OpenEXR library was at hand): which bytes go
 * into which RLE packet (the project's own rule, exr_rle_rule.h; any decoder
 * returns the same bytes), the 24-bit rounding (pxr24_rule.h, restated from
 * OpenEXR's floatToFloat24 from memory), and the numbers of Blender's DNA
 * that tools/blend_export.py maps to the names.
 * rr_create reads RR_EXR_CODEC (one of the names above; empty: the scene's)
 * from the environment the same way; any other text fails rr_create with
 * RR_EINVAL. Applies to frames submitted after the call and to
 * rr_debug_encode_device("OPEN_EXR", 16 | 32, ...), where RR_EXR_CODEC_SCENE
 * means ZIP; frames in flight keep the codec of their submit. PNG, JPEG and
 * the other formats are unaffected. RR_EINVAL for a NULL ctx or any other
 * value. */
#define RR_EXR_CODEC_SCENE 0
#define RR_EXR_CODEC_NONE 1
#define RR_EXR_CODEC_RLE 2
#define RR_EXR_CODEC_ZIPS 3
#define RR_EXR_CODEC_ZIP 4
#define RR_EXR_CODEC_PIZ 5
#define RR_EXR_CODEC_PXR24 6
#define RR_EXR_CODEC_B44 7
#define RR_EXR_CODEC_B44A 8
#define RR_EXR_CODEC_DWAA 9
#define RR_EXR_CODEC_DWAB 10
int rr_set_exr_codec(rr_ctx* ctx, int32_t codec);

/* The codec a scene file asks for (host only; write_still's
 * image_settings.exr_codec, render-timing-script.py:83-92): an
 * RR_EXR_CODEC_* value, RR_EXR_CODEC_ZIP for a scene without
 * render.exr_codec. */
int rr_debug_scene_exr_codec(rr_scene* scene, int32_t* codec);

/* The 24-bit form PXR24 files hold of FLOAT samples (write_still's OPEN_EXR
 * files, render-timing-script.py:83-92), evaluated on the host by the rule the
 * device coder uses (pxr24_rule.h): out[i] = the 24 bits of in[i]; a reader
 * returns out[i] << 8 as the float's bits. Exported so that tests tie the C
 * statement to numpy. RR_EINVAL for a NULL array with n > 0. */
int rr_debug_float24(const float* in, uint64_t n, uint32_t* out);

/* The run-length packets an RLE chunk holds for n bytes that are already
 * reordered and differenced (write_still's OPEN_EXR files,
 * render-timing-script.py:83-92), by the host statement of exr_rle_rule.h.
 * *len receives the packets' length; they are copied to out if cap >= *len.
 * Exported so that tests tie the C statement to numpy. RR_EINVAL for a NULL
 * array or n = 0. */
int rr_debug_exr_rle(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* len);

/* Run the 8-bit view pass (the one frames of the Filmic family and frames
 * with a display gamma or a dither take after rendering) on a float RGBA image
 * of the caller's (width * height * 4 floats, taken as means: spp = 1): value *
 * exposure_scale, view_transform (RR_VIEW_STANDARD .. RR_VIEW_FALSE_COLOR)
 * with ctx's look, display gamma and dither, 8-bit quantisation, alpha 255, into
 * rgba8_out (width * height * 4 bytes). A view or look whose LUT is not loaded
 * is RR_EINVAL here. Exported for tests. */
int rr_debug_view_device(rr_ctx* ctx, const float* rgba, int32_t width, int32_t height,
                         int32_t view_transform, float exposure_scale, uint8_t* rgba8_out);

/* out[i] = in[i]^(1 / gamma) as rr_set_display_gamma defines it, evaluated on
 * the host (no device needed), gamma 1 included (which frames skip). RR_EINVAL
 * for gamma <= 0 or gamma > 5. Exported for tests. */
int rr_debug_display_gamma(const float* in, uint64_t n, float gamma, float* out);

/* The view settings a scene file asks for (host only): its view transform
 * (RR_VIEW_*; Standard for a view this renderer does not know), its look's
 * name without prefix (copied to look if cap exceeds its length; "None" for
 * an unknown look) and its display gamma. Any pointer may be NULL. */
int rr_debug_scene_view(rr_scene* scene, int32_t* view_transform, char* look, int32_t cap, float* gamma);

void rr_scene_free(rr_scene* scene);
void rr_destroy(rr_ctx* ctx);

/* ------------------------------------------------------------------------ *
 * Inspection entry points. Not on the production path; they expose the
 * intermediate state of a frame so the parity tests (tests/) can compare every
 * stage with the CPU oracle (oracle/) on identical inputs.
 * ------------------------------------------------------------------------ */

#define RR_CAM_FLOATS 16   /* pos3 right3 up3 back3 half_w half_h clip_start clip_end */
#define RR_LIGHT_FLOATS 12 /* type pos3 dir3 radius intensity3 pad */
#define RR_MAT_FLOATS 12   /* base3 metallic specular roughness ior emission3 model pad */
#define RR_RENDER_INTS 10  /* W H spp max_bounces seed view_transform spp_per_chunk bvh_width
                              max_diffuse_bounces max_glossy_bounces */
#define RR_RENDER_FLOATS 4 /* clamp_indirect filter_width exposure_scale pad */

int rr_debug_counts(rr_scene* scene, int32_t* n_triangles, int32_t* n_lights,
                    int32_t* n_materials, int32_t* n_objects);

/* The scene's triangles in object space as loaded (generators expanded):
 * tri_local9 n*9 floats (v0 v1 v2), tri_object n object indices (the matrix
 * of rr_debug_object_matrix that places it). Either pointer may be NULL.
 * Test infrastructure: pins the device's world transform (k_transform)
 * against a host restatement; no reference counterpart. */
int rr_debug_scene_mesh(rr_scene* scene, float* tri_local9, int32_t* tri_object);

/* Evaluate the frame on the device (animation, world transform, LBVH) and read
 * back what the integrator consumes. Any output pointer may be NULL. */
int rr_debug_frame_state(rr_ctx* ctx, rr_scene* scene, int32_t frame_index,
                         const rr_render_params* params, float* tris_world /* n*9 */,
                         int32_t* tri_material /* n */, float* camera /* RR_CAM_FLOATS */,
                         float* lights /* n_lights*RR_LIGHT_FLOATS */,
                         float* materials /* n_mat*RR_MAT_FLOATS */, float* world /* 3 */,
                         int32_t* render_ints /* RR_RENDER_INTS */,
                         float* render_floats /* RR_RENDER_FLOATS */);

/* Hierarchy of the frame (rr_debug_bvh_hier): sorted Morton keys and primitive order (n each), internal
 * node children (2*(n-1); leaf = ~sorted_index) and child boxes (12*(n-1):
 * lmin3 lmax3 rmin3 rmax3). n == 1 yields one root whose two children are leaf 0. */
int rr_debug_bvh(rr_ctx* ctx, rr_scene* scene, int32_t frame_index, uint32_t* keys,
                 uint32_t* order, int32_t* children, float* boxes);

/* rr_debug_bvh of a chosen hierarchy: hier 2 = Karras LBVH, 3 = PLOC, 0 = the
 * one the frame kernels use (what rr_debug_bvh returns). */
int rr_debug_bvh_hier(rr_ctx* ctx, rr_scene* scene, int32_t frame_index, int32_t hier, uint32_t* keys,
                      uint32_t* order, int32_t* children, float* boxes);

/* Quantised 6-wide hierarchy of the frame (the PLOC hierarchy collapsed into
 * 6-wide nodes, the hierarchy the split path of large scenes traverses; built
 * on demand here). *nq receives the node count; if children / nodes16 are
 * non-NULL they receive 6*nq child refs (>= 0 node, < 0 ~position in the
 * hierarchy's triangle array, 0x7fffffff unused slot — spelled out from the
 * node's implicit references) and the 16 32-bit words of each 64-byte node:
 * origin x y z (float), exponent bytes (e+128 per axis) | internal-slot mask
 * << 24, first internal child, first leaf triangle, lo x / lo y / lo z / hi x /
 * hi y / hi z grid coordinates of children 0..3 (one byte each), children 4
 * and 5 as byte pairs (lo x, lo y), (lo z, hi x), (hi y, hi z), one zero word;
 * tri_orig (n triangles) the original triangle id at each position of that
 * array. Call once with NULL arrays to size them. */
int rr_debug_qbvh(rr_ctx* ctx, rr_scene* scene, int32_t frame_index, int32_t* nq,
                  int32_t* children, uint32_t* nodes16, int32_t* tri_orig);

/* Trace a batch of rays against the frame's hierarchy. bvh_width: 2 (LBVH),
 * 4 (the quantised 6-wide collapse), 5 (the same hierarchy walked by the camera
 * kernel's 64-ray packets, with 4 packet-stack entries in LDS so that the
 * stack's HBM part is used; closest hit only, occluded = 255), 6 (the
 * 6-wide per-lane walk with one LDS stack entry per lane, so that its grouped
 * entries live in the HBM part), 7 (the camera kernel's default packet walk,
 * one box test per child for the whole packet — packet_trace_beam — with the
 * same 4-entry LDS stack as 5; exact only for packets whose rays share one
 * origin, as camera rays do; closest hit only) or 0 (whichever
 * the frame kernels use for this scene, render_ints[7] of rr_debug_frame_state). rays: n*8 floats
 * (o.xyz, tmin, d.xyz, tmax). hits: n*4 floats (t, u, v, 0), prims: n original
 * triangle ids (-1 miss), occluded: n bytes (any-hit result). */
int rr_debug_trace(rr_ctx* ctx, rr_scene* scene, int32_t frame_index, int32_t bvh_width,
                   int32_t n_rays, const float* rays, float* hits, int32_t* prims,
                   uint8_t* occluded);

/* BSDF sampling at one shading point, as the frame kernels sample it: the
 * material (RR_MAT_FLOATS, rr_debug_frame_state layout), unit normal n3 and
 * view direction wo3; per draw i the three numbers u[3i..3i+2] (lobe pick,
 * disk u1, u2). Outputs per draw: wi3, f3 (BSDF value), pdf and ok (0 the
 * path ends, 1 diffuse lobe, 2 glossy lobe). */
int rr_debug_bsdf_sample(rr_ctx* ctx, const float* mat12, const float* n3, const float* wo3, int32_t n,
                         const float* u, float* wi3, float* f3, float* pdf, int32_t* ok);

/* The tile kernel's scheduling record of the last frame enqueued (LDS-resident
 * scenes): per screen tile (8x8 pixels, row-major), the real-time ticks
 * (100 MHz) its work units took in that frame's k_tiles launch (0 for tiles
 * outside the scene's screen box), and the box tiles' hand-out order that
 * launch used (built from the launch before it; its first entries are the
 * box tiles). Up to `capacity` entries of each; *n_tiles = the length of the
 * slot's buffers (at least the frame's tile count; 0: no tile frame yet).
 * unit_log (may be null): when that frame was rendered with
 * RR_FLAG_COUNT_TRAVERSAL, per box work unit u (hand-out number, below
 * unit_capacity and 65536) its start and end real-time ticks (2 per unit;
 * 0, 0: not logged). */
int rr_debug_tile_costs(rr_ctx* ctx, int32_t capacity, uint32_t* costs, int32_t* order, int32_t* n_tiles,
                        uint64_t* unit_log, int32_t unit_capacity);

/* The per-sample path's square roots and reciprocals (rr_device.h sqrt_rn /
 * sqrt_any / rcp_rn) against the device's correctly rounded sqrtf and
 * 1.0f / x, over the float bit patterns lo .. lo + n - 1: counts5[0] =
 * sqrt_rn mismatches with the argument in its range (+-0 or [2^-96, FLT_MAX];
 * must be 0), [1] = sqrt_rn mismatches outside it (not called there), [2] =
 * sqrt_any mismatches (must be 0), [3] = rcp_rn mismatches with |x| in
 * [2^-126, 2^126) (must be 0), [4] = rcp_rn mismatches outside it. Test
 * infrastructure for the bit-exactness claim; no reference counterpart. */
int rr_debug_fastmath_check(rr_ctx* ctx, uint32_t lo, uint64_t n, uint64_t* counts5);

/* Host animation evaluation: object_to_world matrix (row-major 4x4, f64) of
 * object `object_index` at (possibly fractional) frame. */
int rr_debug_object_matrix(rr_scene* scene, int32_t object_index, double frame,
                           double* m16);

#ifdef __cplusplus
}
#endif

#endif /* RR_H */
