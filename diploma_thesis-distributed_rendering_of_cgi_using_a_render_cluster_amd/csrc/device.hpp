// Host-side interface of the device module: buffers in HBM and the launch
// sequences of the LBVH build (bvh.hip) and the path integrator (wavefront.hip:
// the split path and the frame dispatcher; tiles.hip: the tile path).
// Every piece of device state has one owner, and the functions below take the
// state they work on as parameters: the context owns DevPaths (shared queues
// and tables) and one DevFrame for the inspection entry points, a frame slot
// owns a DevFrame and a DevBuild, a scene owns its DevMesh and a DevBuild.
// DESIGN.md §3 has the table, §4 the layout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "region_rule.h"
#include "rr.h"
#include "rr_device.h"

namespace rr {

struct HipError : std::runtime_error {
    int code;
    HipError(const std::string& what, int c) : std::runtime_error(what), code(c) {}
};

#define RR_HIP(call)                                                                             \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess)                                                                    \
            throw ::rr::HipError(std::string(#call) + ": " + hipGetErrorString(_e), (int)_e);   \
    } while (0)

// Grow-only device allocation with one owner: freed with it, moved but never
// copied. The long-lived owners still release() in an order of their own, with
// their device current (rr_destroy); the destructor is for the locals of the
// inspection entry points, which an exception would otherwise leak.
template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) {
        o.ptr = nullptr;
        o.cap = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            ptr = o.ptr;
            cap = o.cap;
            o.ptr = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void ensure(size_t n) {
        if (n <= cap) return;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        if (n == 0) return;
        RR_HIP(hipMalloc(&ptr, n * sizeof(T)));
        cap = n;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// A scene's uploaded triangles, object space: written once (upload_scene),
// read by every hierarchy build of the scene.
struct DevMesh {
    int n_tris = 0;
    int n_objs = 0;
    DevBuf<float4> tri_local;  // 3 per triangle, object space
    DevBuf<int32_t> tri_obj;
    DevBuf<int32_t> tri_mat;
    bool uploaded = false;
    void release();
};

// The products of one hierarchy build of a mesh: transforms, world triangles,
// build scratch, the acceleration structure and what it was built for. A
// scene owns one set; every frame slot owns one more for its k_tiles frames.
struct DevBuild {
    DevBuf<float> obj_xform;   // 12 per object
    DevBuf<float4> tri_world;  // 3 per triangle, world space (this frame)
    // LBVH build scratch
    DevBuf<uint32_t> bounds;    // 6 ordered-uint words (centroid-sum AABB)
    DevBuf<uint32_t> keys[2], vals[2];
    DevBuf<uint32_t> hist;      // 256 * nblocks
    DevBuf<uint32_t> scan_part; // partial sums of the scan
    DevBuf<int2> children;      // n-1
    DevBuf<int32_t> node_parent;  // n-1 : parent*2+side, -1 root
    DevBuf<int32_t> leaf_parent;  // n
    DevBuf<uint32_t> flags;       // n-1 arrival counters
    DevBuf<int2> range;           // n-1 : (first sorted leaf, leaf count) under each node
    // acceleration structure consumed by traversal
    DevBuf<BvhNode> nodes;  // max(n-1, 1)
    DevBuf<TriPack> tris;   // n, leaf order (after a BVH4 collapse: the BVH4's leaf order)
    DevBuf<QNode6> qnodes;     // quantised 6-wide collapse of `nodes` (split path), <= n-1
    DevBuf<float4> tnrm;       // split path, per triangle in leaf order: unit geometric normal, material id (shading)
    DevBuf<TriPack> qtris;     // collapse scratch: the triangles in the collapse's leaf order (swapped into `tris`)
    DevBuf<int32_t> q_src;     // wide node -> its BVH2 root (collapse scratch)
    DevBuf<uint32_t> q_cnt;    // per frontier node: internal children (scanned in place)
    DevBuf<uint32_t> q_tcnt;   // per frontier node: leaf children (scanned in place)
    DevBuf<int32_t> q_ctl;     // current level [lo, hi), first triangle of the level
    int nq = 0;                // wide nodes
    bool has4 = false;
    // PLOC build (large scenes): cluster ping-pong, neighbours, scan flags, counters
    DevBuf<float4> ploc_cl[2];
    DevBuf<int32_t> ploc_nn;
    DevBuf<uint32_t> ploc_keep, ploc_mrg;
    DevBuf<int32_t> ploc_ctl;
    bool ploc = false;  // the current nodes come from PLOC (else the Karras LBVH)
    std::vector<float> cached_xform;  // obj_xform of the current build
    bool built = false;
    void release();  // back to the unbuilt state
};

// Optional per-launch HIP-event timing (RR_FLAG_PROFILE_KERNELS), on the
// stream the kernels run on.
struct KernelProfiler {
    bool on = false;
    std::vector<hipEvent_t> pool;
    std::vector<int> cls;  // class of event pair i
    size_t used = 0;       // events in use (pairs * 2)
    void reset(bool enable) {
        on = enable;
        used = 0;
        cls.clear();
    }
    void begin(hipStream_t st, int c) {
        if (!on) return;
        while (pool.size() < used + 2) {
            hipEvent_t e;
            RR_HIP(hipEventCreate(&e));
            pool.push_back(e);
        }
        cls.push_back(c);
        RR_HIP(hipEventRecord(pool[used], st));
    }
    void end(hipStream_t st) {
        if (!on) return;
        RR_HIP(hipEventRecord(pool[used + 1], st));
        used += 2;
    }
    // after the stream has been synchronised
    void collect(double* ms, int32_t* launches) {
        for (size_t i = 0; i < cls.size(); ++i) {
            float t = 0.f;
            RR_HIP(hipEventElapsedTime(&t, pool[2 * i], pool[2 * i + 1]));
            ms[cls[i]] += t;
            launches[cls[i]] += 1;
        }
    }
    void release() {
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

// Shared by all frames of a context: the split path's queues (sized for the
// largest chunk seen) and the read-only tables. Only split-path frames use the
// queues, and such a frame always waits for its predecessor.
struct DevPaths {
    size_t cap = 0;
    DevBuf<float4> rad;                        // per path (p-indexed) radiance record
    DevBuf<float4> ps_o[2], ps_d[2], ps_t[2];  // segmented path queue, ping-pong per bounce
    DevBuf<float4> sh_o, sh_d, sh_c;           // segmented shadow queue
    DevBuf<float2> hits;                       // split path: (t, leaf index) per queue entry
    DevBuf<uint32_t> qctr;                     // split path: grouped queue append counters
    DevBuf<float4> film_part;  // open sample group's partial sum between chunks (k_accumulate)
    DevBuf<float> filter_table;
    DevBuf<float> srgb_lut;
    int grid_blocks = 0;  // persistent grid for path kernels
    void ensure_paths(size_t n);  // wavefront.hip
    void release();
};

// The device state of one frame. Every frame slot owns one, so frames in
// flight together share no buffer they write; the context owns one more (the
// home set) for the inspection entry points. The device code takes the one to
// work on as a parameter.
struct DevFrame {
    DevBuf<int32_t> counters;  // per chunk, per bounce b: {paths entering b+1, shadow rays of b}
    DevBuf<int32_t> spill;     // traversal stack spill
    DevBuf<float4> film;
    DevBuf<uint8_t> rgba8;
    DevBuf<float> tile_slab;   // k_tiles: per sliced tile, one group sum plane per sample group
    DevBuf<uint32_t> tile_ctrs;  // k_tiles: work-unit counters, one 128-B line per shard
    // kept from frame to frame: the next order is built from the owner's last costs
    DevBuf<uint32_t> tile_cost;  // k_tiles: per screen tile, the real-time ticks its units took (last launch); then,
                                 // per screen tile, the samples its covered body ran (counting launches, tiles.hip)
    DevBuf<int32_t> tile_order;  // k_tiles: box tiles by descending tile_cost (k_tile_order)
    DevBuf<float> lights, materials;
    DevBuf<float> mat_lut;             // material tables (build_material_lut), uploaded when they change
    std::vector<float> mat_lut_cached;
    DevBuf<unsigned long long> trav_counts;  // RR_FLAG_COUNT_TRAVERSAL: kTravWords
    KernelProfiler prof;
    // scratch of the device coders: JPEG coefficients and entropy coder (jpeg.hip), deflate (a frame has one format)
    DevBuf<int16_t> jpeg_coeffs;
    DevBuf<uint32_t> jpeg_blk, jpeg_scratch;
    DevBuf<uint32_t> deflate_scratch;
    // PNG frames with the adaptive filter (rr_set_png_compression): a filter type per image row, and at 16 bits
    // the raw big-endian scanlines (png16.hip k_png16_raw); grow-only, untouched by legacy frames
    DevBuf<uint8_t> png_ftype, png_raw;
    // TARGA, HDR, IRIS and WEBP frames, and OPEN_EXR frames of the codecs NONE and RLE (tga.hip, hdr.hip, iris.hip,
    // webp.hip, exr_codec.hip): the dense body and the coder's records, carved by the coder's *_carve;
    // grow-only. The coders of a frame's files run one after another on its stream, so they share it
    // (and the scratch above), sized for the largest before the first is enqueued (frame.hpp reserve_coder)
    DevBuf<uint32_t> body_scratch;
    // Reduced outputs (rr_frame_output.reduce; reduce.hip): per factor 2, 4, 8 the reduced film, sums as
    // `film` holds, and the 8-bit image the view pass makes of it; allocated at the first frame that needs them
    struct Reduced {
        DevBuf<float4> film;
        DevBuf<uint8_t> rgba8;
    } reduced[3];
    static int reduced_slot(int k) { return k == 2 ? 0 : k == 4 ? 1 : 2; }
    // A region frame (rr_set_region; region.hip): the windowed film, sums as `film` holds, and the 8-bit image
    // the view pass makes of it; what the reductions and the coders of such a frame read instead of film / rgba8
    DevBuf<float4> window_film;
    DevBuf<uint8_t> window_rgba8;
    // written by render_frame_device, about the frame it enqueued
    int tile_slices = 0;       // k_tiles units per box tile (0: not k_tiles)
    bool unit_logged = false;  // its k_tiles launch wrote the unit log (trav_counts)
    void ensure_spill(int grid_blocks);  // the traversal stack spill area of a persistent grid
    void release();
};

// How render_frame_device renders a frame.
struct FrameOpts {
    bool count_traversal = false;  // RR_FLAG_COUNT_TRAVERSAL
    bool force_wavefront = false;  // RR_FLAG_WAVEFRONT: LDS-resident scenes take the split path, not k_tiles
    bool tile_whole = false;       // k_tiles: one work unit per tile (the frame overlaps a pending one)
    // a region frame (rr_set_region): the split path traces and accumulates the region's pixels alone, the tile
    // path runs the 8 x 8 tiles that meet the region alone (partial tiles whole); either leaves the film outside
    // unwritten. Inside the frame, not empty.
    bool region_on = false;
    RegionRect region;
};

// Frame constants passed by value to the path kernels.
struct FrameConsts {
    float3 cam_pos, cam_right, cam_up, cam_back;
    float half_w, half_h, clip_start, clip_end;
    float inv_w2, inv_h2;  // 2/W, 2/H
    int W, H, npix;
    // pixel index -> (x, y); split-path index p = pixel * spp_chunk + sample ->
    // (pixel, sample): pixel-major, so the samples of a pixel are neighbours in
    // every per-path array (set per chunk, render_split)
    FastDiv div_w, div_spp;
    int spp_total, spp_chunk, first_sample, max_bounces, n_lights;
    int max_diffuse, max_glossy;  // per-lobe bounce caps (>= 1, setup_frame)
    uint32_t seed;
    float clamp_indirect, exposure_scale, inv_spp;
    int view_transform;
    float3 world;
    int n_tris, n_mats;
    // bound on |subpixel offset| of a camera sample (filter support + 1 px of
    // rounding slack): k_tiles' whole-tile culling test
    float filter_reach;
};

// The split path's constants: the frame's, and the pixels it enumerates. Its path index is p = dense pixel *
// spp_chunk + sample with the dense pixel in [0, npix); a region frame (rw > 0) counts the region's pixels
// row-major, npix = rw * region rows, and region_pix maps a dense pixel to the full-frame pixel that the camera
// ray, the RNG key and the film use, so a region's samples are the full frame's. rw = 0: dense = full.
struct SplitConsts : FrameConsts {
    int rx0 = 0, ry0 = 0, rw = 0;
    FastDiv div_rw;
};

// LBVH build for the current obj_xform (uploaded by the caller).
// Stream-ordered; no host synchronisation inside.
// want4: also collapse it into the BVH4 the split path traverses.
// want_ploc: build the PLOC hierarchy instead (large scenes; not with want4).
void build_lbvh(const DevMesh& m, DevBuild& s, hipStream_t st, KernelProfiler* prof = nullptr, bool want4 = false,
                bool want_ploc = false);

// Per-frame constants (lights, materials, object transforms; up to
// kUploadMax floats in all) copied into device buffers by one kernel whose
// arguments carry the data (bvh.hip k_upload). A hipMemcpyAsync from pinned
// host memory is a GPU read over PCIe, and such a read queues behind the
// previous frame's 6 MB of device-to-host output writes (PCIe keeps reads
// behind posted writes): measured 112 us per frame on 04vs. Kernel arguments
// are written by the host into device memory, so nothing waits.
constexpr int kUploadMax = 720;
// RR_FLAG_COUNT_TRAVERSAL words: [0..5] traversal totals (nodes, triangles per
// class); k_tiles' counting launch: [6] shader-clock ticks and [7] real-time
// ticks after the scene staging, [8] waves, [9] real-time ticks from entry,
// [10] ~first entry, [11] last end, [12] last entry, [13] ~first end
// (frame.cpp fill_stats). (Traversal-stack drops are counted in every
// frame, in the chunk counters: drops_slot.)
constexpr int kTravWords = 14;
// k_tiles' counting launch also logs each box unit u < kUnitLog: words
// kTravWords + 2u / + 2u + 1 = its start / end real-time ticks (rr_debug_tile_costs)
constexpr int kUnitLog = 1 << 16;
struct UploadSeg {
    float* dst;
    int n;
};
bool upload_by_kernarg(const float* src, const UploadSeg* segs, int nseg, hipStream_t st);

// Whether the path kernels take the LDS-resident (fused, BVH2) variant for a
// scene of these sizes; otherwise the split path over the BVH4 in HBM.
bool scene_in_lds(int n_tris, int n_mats, int n_lights);

// Whether render_frame_device renders this frame with k_tiles (one launch over
// all samples; LDS-resident scene). Such a frame touches only per-frame-slot
// buffers and read-only tables, so it may run beside the other slot's frame.
bool frame_uses_tiles(const FrameConsts& base, bool force_wavefront);
// The pixels a tile-path frame runs: the frame's, or of a region frame those of the tiles that meet the region
// (partial tiles count whole, cut only at the frame's edges).
long long tiles_pixels_run(int W, int H, bool region_on, const RegionRect& r);

// Render all chunks of one frame: film accumulate + tonemap to rgba8.
// counters_per_chunk receives the device counter layout for stats.
void render_frame_device(const DevMesh& m, DevBuild& s, DevPaths& p, DevFrame& f, const FrameConsts& base,
                         int n_chunks, FrameOpts o, hipStream_t st);
// The k_tiles frame of render_frame_device (frame_uses_tiles holds; tiles.hip):
// k_tile_order, k_tiles over all samples, k_tiles_fold when tiles are sliced.
void render_tiles_device(const DevMesh& m, DevBuild& s, DevPaths& p, DevFrame& f, const FrameConsts& base,
                         int n_chunks, FrameOpts o, hipStream_t st);

// Trace a batch of rays (debug / parity entry point).
void trace_batch_device(const DevMesh& m, DevBuild& s, DevPaths& p, DevFrame& f, int n, const float4* d_rays,
                        float4* d_hits, int32_t* d_prims, uint8_t* d_occ, hipStream_t st, int width);

// BSDF sampling batch at one shading point (debug / parity entry point).
void bsdf_batch_device(const float* d_mat12, const float* d_lut, const float n3[3], const float wo3[3], int n,
                       const float* d_u, float* d_wi, float* d_f, float* d_pdf, int32_t* d_ok, hipStream_t st);

// sqrt_rn / sqrt_any / rcp_rn (rr_device.h) against sqrtf and 1.0f / x over
// the float bit patterns [lo, lo + n) on the device; d_counts: 5 words
// (rr_debug_fastmath_check).
void fastmath_check_device(uint32_t lo, uint64_t n, unsigned long long* d_counts, hipStream_t st);

// Device JPEG encode (jpeg.hip): the forward transform (tab = dct | qinv luma |
// qinv chroma) + Huffman coding
// of the coefficients into the entropy-coded segment of the file (rows, RSTn
// markers, EOI), written to pinned host memory as [uint64 length][8 B pad]
// [bytes]. d_huff: 4 x 256 packed code | len << 16 (DC luma, AC luma, DC
// chroma, AC chroma; image_io jpeg_huff_tables).
constexpr int kJpegBlockMaxBytes = 216;  // >= the longest coded 8x8 block (1 + 63 x 26 + 27 bits)
struct JpegDevBufs {
    uint32_t* acbits;    // per block: AC bits
    uint32_t* blk_off;   // per block: bit offset in its row
    uint32_t* row_bits;  // mcuy
    uint32_t* ready;     // mcuy: stuffed row length + 1 once counted (k_jpeg_finish)
    uint32_t* scratch;   // mcuy x jpeg_row_scratch_words
};
// grey: a one-component file (rr_set_color_mode BW): MCUs of one 8x8 block, Y
// the grey code of grey.h; else six blocks of a 16x16 MCU.
size_t jpeg_mcu_rows(int H, bool grey);
size_t jpeg_block_count(int W, int H, bool grey);
size_t jpeg_row_scratch_words(int W, bool grey);
size_t jpeg_stream_max_bytes(int W, int H, bool grey);
void jpeg_encode_device(const uint8_t* d_rgba, int W, int H, bool grey, const float* d_tab, const uint32_t* d_huff,
                        int16_t* d_coeffs, JpegDevBufs& b, uint8_t* host_out, hipStream_t st);

// The formats coded by the device deflate coder (deflate.hpp): each has
// a plan (false: the size is outside what the encoder takes, W above the bound
// named below or a stream of 2 GB and more) and an encode call that runs its
// front end, the coder's stages and the gather into pinned host memory:
// host_out = [uint64 length][8 B pad][bytes], host_tab = the bands' table
// (DeflatePlan::own_stream). scratch: deflate_scratch_words(p) words.
struct DeflatePlan;

// 8-bit PNG (png.hip): the Sub-filtered RGBA8 frame as one zlib stream, 78 01 +
// deflate data (image_io png_wrap_stream). W <= 2^20.
// C: channels of the file (rr_set_color_mode): 4 RGBA, 3 RGB, 1 grey; rows of C W + 1 bytes.
bool png_plan(int W, int H, int C, DeflatePlan& p);
void png_encode_device(const uint8_t* d_rgba, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* host_out,
                       uint32_t* host_tab, hipStream_t st);
// The same file with libpng's adaptive filter on every row (rr_set_png_compression
// 0 .. 100; png_filter.h): same plan. ftype: p.H bytes, the rows' filter types.
void png_encode_device_adaptive(const uint8_t* d_rgba, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* ftype,
                                uint8_t* host_out, uint32_t* host_tab, hipStream_t st);

// OpenEXR (exr.hip): the film's means as half-float A, B, G, R planes in ZIP
// chunks of kDeflateBandRows scanlines (half conversion, plane split, byte
// reorder, predictor); the bytes are the chunks' pieces: deflate data without
// zlib framing, or the raw chunk bytes (image_io exr_wrap_stream). W <= 2^19
// (band positions in 32-bit counters).
// C: 4 the planes A, B, G, R; 3: B, G, R; 1: Y, the Rec.709 luma of the means; 2C W bytes a scanline.
bool exr_plan(int W, int H, int C, DeflatePlan& p);
size_t exr_stream_max_bytes(const DeflatePlan& p);  // every chunk raw
// film: W x H float4 sums, scaled by inv_spp; alpha_one: 1 A = 1.0 (rendered frames), 0 film.w * inv_spp, 2 a mask:
// A = 1.0 where film.w != 0 and 0 elsewhere (an uncropped region frame's windowed film).
void exr_encode_device(const float4* d_film, float inv_spp, int alpha_one, int C, const DeflatePlan& p,
                       uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st);
// The same file with FLOAT channels: the means' own bits (no clamp, no
// rounding), chunks of 16W bytes a scanline; exr_stream_max_bytes and the table
// as above. W <= 2^18 (a band has twice the bytes).
bool exr32_plan(int W, int H, int C, DeflatePlan& p);
void exr32_encode_device(const float4* d_film, float inv_spp, int alpha_one, int C, const DeflatePlan& p,
                         uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st);
// The same files with PXR24 chunks (rr_set_exr_codec; exr.hip Pxr24Front): zlib
// over 16 scanlines of byte planes of pixel differences, depth 16 the halfs'
// own bits, 32 the floats' 24-bit form (pxr24_rule.h; 3 C W bytes a scanline in
// the stream, DeflatePlan::raw_stride = 4 C W in a raw chunk). The ranges of
// exr_plan / exr32_plan; exr_stream_max_bytes and the table as above.
bool pxr24_plan(int W, int H, int C, int depth, DeflatePlan& p);
void pxr24_encode_device(const float4* d_film, float inv_spp, int alpha_one, int C, int depth, const DeflatePlan& p,
                         uint32_t* scratch, uint8_t* host_out, uint32_t* host_tab, hipStream_t st);

// The view settings of a frame as kernel arguments (view.hpp FilmicDev::args):
// the Filmic LUTs of one device and the display gamma. lut1 is the curve the
// frame's look selects (the base curve for None and Medium Contrast); fcube
// the false-colour cube (RR_VIEW_FALSE_COLOR only). Views outside the Filmic
// family leave the LUT fields zero. dither: the intensity of the 8-bit image's
// dither (rr_set_dither; view_device only, the 16-bit front end does not read
// it). It stands where the struct had four bytes of padding, so the other
// fields, and the kernel arguments behind the struct, keep their offsets.
struct FilmicArgs {
    const float4* cube;
    const float* lut1;
    int n3, n1, comps;
    float lo1, hi1;
    float dither;  // 0: none
    const float4* fcube;
    int nf;
    float inv_gamma;  // 1 / display gamma; 0: gamma 1, no gamma step
};

// Device 16-bit PNG encode (png16.hip): the film's display-referred image as
// RGBA with 16-bit big-endian samples, A = 65535. Front end (mean, exposure,
// clamp, view transform, quantize16, Sub filter over 8-byte pixels, Adler
// sums) as one zlib stream; host_out and host_tab as png_encode_device writes
// them (image_io png_wrap_stream, depth 16). W <= 2^19 (band positions in
// 32-bit counters).
// C as for png_plan: rows of 2C W + 1 bytes.
bool png16_plan(int W, int H, int C, DeflatePlan& p);
struct Png16Front {
    const float4* film;  // W x H sums
    float inv_spp, exposure_scale;
    int view_transform;  // RR_VIEW_STANDARD / RAW, or one of the Filmic family (`filmic` holds the LUTs)
    const float* srgb16;  // kSrgb16LutSize + 2 floats (scene.hpp build_srgb16_lut)
    FilmicArgs filmic;    // the LUTs, and for every view the display gamma
    // an uncropped region frame's windowed film: a pixel with film.w == 0 lies outside the region and is written
    // (0, 0, 0, 0), any other as usual with A = 65535 (the extended front end alone reads it)
    int alpha_mask = 0;
};
void png16_encode_device(const Png16Front& f, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* host_out,
                         uint32_t* host_tab, hipStream_t st);
// The same file with the adaptive filter (as png_encode_device_adaptive). raw:
// 2C W H bytes, the raw scanlines (below 2 GB, as the plan's stream is);
// ftype: p.H bytes.
void png16_encode_device_adaptive(const Png16Front& f, int C, const DeflatePlan& p, uint32_t* scratch, uint8_t* raw,
                                  uint8_t* ftype, uint8_t* host_out, uint32_t* host_tab, hipStream_t st);

// Per chunk: one pair per bounce b = 0..max_bounces {paths entering b+1,
// shadow rays of b}, one pair of slack, then the words below.
int counters_per_chunk(int max_bounces);
// Word of a chunk's counters holding the camera rays traced (counters_per_chunk).
RR_HD int camera_traced_slot(int max_bounces) { return 2 * (max_bounces + 2); }
// Traversal-stack pushes dropped for want of room (every frame; a dropped push
// is a missed subtree, rr_frame_stats.stack_drops).
RR_HD int drops_slot(int max_bounces) { return 2 * (max_bounces + 2) + 1; }
// k_tiles: continuations / shadow rays traversed (two words; the others left
// a hull side of their triangle, hull_flags, and were resolved without one).
RR_HD int escaped_slot(int max_bounces) { return 2 * (max_bounces + 2) + 2; }
int device_cu_count();

}  // namespace rr
