// Host side of the wavefront path tracer: the frame
// dispatcher and the split path of large scenes, whose kernels are in
// split_kernels.hpp. Per chunk of spp_chunk samples x all pixels
// (render_split), one stream of launches with no host round trip:
//   k_trace_primary_packet  camera rays (K6 raygen + K7 closest hit), walked
//              as packets of 64 pixel-major paths -> hits[path];
//   k_shade_primary         bounce 0 (K9): writes the path's radiance record
//              and appends, through wave-level ballot/popcount compaction (K8)
//              into grouped queues, only what continues: the next ray +
//              throughput to the path queue, the NEE ray to the shadow queue;
//   per bounce b:
//   k_shadow_refill         (K10 any-hit) over the shadow queue of bounce b:
//              adds the unoccluded NEE contribution to the radiance record;
//   k_trace_extend          (K7) over the path queue entering bounce b + 1
//              -> hits[slot];
//   k_shade_extend          (K9 + K8) shades bounce b + 1 from hits[slot] and
//              appends the next queues;
//   k_accumulate (K11 + K12 on the last chunk): film += chunk radiance in
//              sample order, then mean -> exposure -> view transform -> 8-bit.
// The trace kernels are persistent: their waves take chunks of 64 queue
// positions from per-XCD counters and refill idle lanes (trace_refill); every
// count they need is read on the device.
//
// HBM per camera path: 8 B hit write + read, 12 B radiance write, 12 B
// accumulate read; per continuing path per bounce: 48 B state write + read,
// 8 B hit write + read, 24 B radiance RMW; per shadow ray: 48 B write + read
// (+24 B RMW when unoccluded). The arithmetic is the uncontracted, libm-free
// form of rr_device.h and matches oracle/rr_oracle.c bit for bit.
//
// LDS-resident scenes render through the tile path (tiles.hip,
// render_tiles_device, which includes the same kernel header); what both
// paths share is in paths.hpp. The debug entry points (rr_debug_trace and
// friends) launch from here too.
//
// Replaces the per-pixel, per-sample path integration of Cycles behind
// bpy.ops.render.render (the reference's scripts/render-timing-script.py:90).
#pragma clang fp contract(off)

#include <cstdlib>
#include <string>

#include "split_kernels.hpp"

namespace rr {

int device_cu_count() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        RR_HIP(hipGetDevice(&dev));
        RR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (cus <= 0) cus = 256;
    }
    return cus;
}

// Per chunk, one pair per bounce b = 0..max_bounces: {paths entering bounce
// b+1, shadow rays of bounce b}, written by the consuming kernels, +1 pair of
// slack, then camera rays traced (not culled, tested against at least one
// triangle), traversal-stack drops, and k_tiles' escaped continuations and
// escaped shadow rays (device.hpp camera_traced_slot .. escaped_slot).
int counters_per_chunk(int max_bounces) { return 2 * (max_bounces + 2) + 4; }

namespace {
// Launch geometry of the split (trace / shade) path of large scenes.
struct SplitGrids {
    int trace_e, shadow, shade_p, shade_e, packet;
    void (*kte)(SceneArgs, PathQueue, QueueIn, float2*, int32_t*, unsigned long long*, uint32_t*);
    void (*kts)(SceneArgs, ShadowQueue, QueueIn, Rad, int32_t*, unsigned long long*, uint32_t*);
    void (*ktpk)(SplitConsts, SceneArgs, int, float2*, uint32_t*, int32_t*, unsigned long long*, uint32_t*);  // packets
    explicit SplitGrids(bool count) {
        kte = count ? k_trace_extend<true> : k_trace_extend<false>;
        kts = count ? k_shadow_refill<true> : k_shadow_refill<false>;
        ktpk = count ? k_trace_primary_packet<true> : k_trace_primary_packet<false>;
        trace_e = grid_for(kte, 0, kTraceBlock);
        shadow = grid_for(kts, 0, kTraceBlock);
        packet = grid_for(ktpk, 0);
        shade_p = grid_for(k_shade_primary, 0);
        shade_e = grid_for(k_shade_extend, 0);
    }
};
// Slots per append group for a producer of `grid` blocks over at most `work`
// items: each wave emits at most ceil(work / threads) * 64 per queue, and a
// group holds ceil(waves / kQGroups) waves.
inline uint32_t group_cap(long work, int grid) {
    const long waves = (long)grid * kWavesPerBlock;
    const long per_wave = ((work + (long)grid * kBlock - 1) / ((long)grid * kBlock)) * 64;
    return (uint32_t)(((waves + kQGroups - 1) / kQGroups) * per_wave);
}
int accum_grid() {
    static const int g = resident_grid(k_accumulate);
    return g;
}
// Host side of deal_ctrs: the camera packets deal from word 2 of the bounce-0
// path queue's counter lines (written by k_shade_primary after them, word 0).
inline uint32_t* deal_host(uint32_t* q, int word) { return q + word; }
}  // namespace

void DevPaths::ensure_paths(size_t n) {
    if (grid_blocks == 0) grid_blocks = device_cu_count() * kMaxBlocksPerCu;
    n += (size_t)grid_blocks * kBlock + n / 64;  // group round-up slack (group_cap)
    if (n > cap) {
        for (DevBuf<float4>* b : {&rad, &ps_o[0], &ps_d[0], &ps_t[0], &ps_o[1], &ps_d[1], &ps_t[1], &sh_o, &sh_d,
                                  &sh_c})
            b->ensure(n);
        hits.ensure(n);
        cap = n;
    }
}

void DevPaths::release() {
    for (DevBuf<float4>* b : {&rad, &ps_o[0], &ps_d[0], &ps_t[0], &ps_o[1], &ps_d[1], &ps_t[1], &sh_o, &sh_d,
                              &sh_c, &film_part})
        b->release();
    hits.release(); qctr.release();
    filter_table.release(); srgb_lut.release();
    cap = 0;
}

void DevFrame::ensure_spill(int grid_blocks) { spill.ensure((size_t)kSpillLane * grid_blocks * kBlock); }

void DevFrame::release() {
    counters.release(); spill.release(); film.release(); rgba8.release();
    tile_slab.release(); tile_ctrs.release(); tile_cost.release(); tile_order.release();
    lights.release(); materials.release();
    mat_lut.release();
    mat_lut_cached.clear();
    trav_counts.release();
    prof.release();
    jpeg_coeffs.release(); jpeg_blk.release(); jpeg_scratch.release(); deflate_scratch.release();
    png_ftype.release(); png_raw.release();
    body_scratch.release();
    window_film.release(); window_rgba8.release();
}

namespace {
// Large scenes: per chunk trace_primary_packet -> shade_primary -> for each
// bounce b: shadow(b), trace_extend(b+1), shade_extend(b+1) -> accumulate.
// Radiance additions per path happen in the oracle's order.
// Camera rays are always traced as packets of 64 pixel-major positions (the
// samples of one or two pixels: nearly one ray). Per frame slice (02 / 03 at
// 64 spp, C5 at 16 spp), camera-ray traversal: 8x8-tile packets of one sample
// 16.1 / 20.6 ms and per-lane walks C5 20.4 ms (sample-major) or 17.7 ms
// (pixel-major); pixel-major packets 12.5 / 14.1 / 15.6 ms, the fastest on all
// three (before the beam, packet_trace_beam). The per-lane camera kernel
// (k_trace_primary) and the round-3 rule "packets only where a triangle covers
// two pixels" were removed with their A/B switch.
void render_split(DevPaths& p, DevFrame& f, const SplitConsts& base, int n_chunks, hipStream_t st, const SceneArgs& sa,
                  unsigned long long* tc, PathQueue pq[2], const ShadowQueue& sq, const float4* tnrm) {
    KernelProfiler& pr = f.prof;
    const SplitGrids G(tc != nullptr);
    const int npix = base.npix;
    const int cpc = counters_per_chunk(base.max_bounces);
    // group counters: [chunk][bounce 0..max][path | shadow][kQGroups * kQStride]
    const size_t per_q = (size_t)kQGroups * kQStride;
    const size_t per_chunk = (size_t)(base.max_bounces + 1) * 2 * per_q;
    p.qctr.ensure(per_chunk * n_chunks);
    RR_HIP(hipMemsetAsync(p.qctr.ptr, 0, per_chunk * n_chunks * sizeof(uint32_t), st));
    for (int c = 0; c < n_chunks; ++c) {
        SplitConsts fc = base;
        fc.first_sample = c * base.spp_chunk;
        fc.spp_chunk = base.spp_chunk;
        if (fc.first_sample + fc.spp_chunk > base.spp_total) fc.spp_chunk = base.spp_total - fc.first_sample;
        fc.div_spp = FastDiv::make((uint32_t)fc.spp_chunk);
        const int np = npix * fc.spp_chunk;
        uint32_t* tot = reinterpret_cast<uint32_t*>(f.counters.ptr + (size_t)cpc * c);
        uint32_t* tail = tot + camera_traced_slot(base.max_bounces);  // traced, drops (device.hpp)
        uint32_t* qc = p.qctr.ptr + per_chunk * c;
        auto qpath = [&](int b) { return qc + ((size_t)b * 2 + 0) * per_q; };    // paths entering b+1
        auto qshadow = [&](int b) { return qc + ((size_t)b * 2 + 1) * per_q; };  // shadow rays of b
        const int gsp = clamp_grid(np, G.shade_p), gse = clamp_grid(np, G.shade_e);
        const uint32_t cap_p = group_cap(np, gsp), cap_e = group_cap(np, gse);
        if ((size_t)std::max(cap_p, cap_e) * kQGroups > p.cap)
            throw std::runtime_error("queue capacity exceeded (split path)");
        pr.begin(st, RR_K_PRIMARY);
        G.ktpk<<<clamp_grid(np, G.packet), kBlock, 0, st>>>(fc, sa, np, p.hits.ptr, deal_host(qpath(0), 2), f.spill.ptr,
                                                           tc, tail);
        pr.end(st);
        pr.begin(st, RR_K_SHADE);
        k_shade_primary<<<gsp, kBlock, 0, st>>>(fc, sa, np, p.hits.ptr, Rad{reinterpret_cast<float*>(p.rad.ptr)}, pq[1],
                                                sq, QueueOut{qpath(0), qshadow(0), cap_p}, tnrm);
        pr.end(st);
        uint32_t cap_prev = cap_p;  // group capacity of the producer of the current queues
        for (int b = 0; b <= base.max_bounces; ++b) {
            pr.begin(st, RR_K_SHADOW);
            G.kts<<<clamp_grid(np, G.shadow, kTraceBlock), kTraceBlock, 0, st>>>(
                sa, sq, QueueIn{qshadow(b), cap_prev, tot + 2 * b + 1}, Rad{reinterpret_cast<float*>(p.rad.ptr)},
                f.spill.ptr, tc, tail);
            pr.end(st);
            if (b == base.max_bounces) break;
            const int nb = b + 1;  // bounce being traced and shaded
            const QueueIn qin{qpath(b), cap_prev, tot + 2 * b};
            pr.begin(st, RR_K_EXTEND);
            G.kte<<<clamp_grid(np, G.trace_e, kTraceBlock), kTraceBlock, 0, st>>>(sa, pq[nb & 1], qin, p.hits.ptr,
                                                                                f.spill.ptr, tc, tail);
            pr.end(st);
            pr.begin(st, RR_K_SHADE);
            k_shade_extend<<<gse, kBlock, 0, st>>>(fc, nb, sa, pq[nb & 1], QueueIn{qpath(b), cap_prev, nullptr},
                                                   p.hits.ptr, Rad{reinterpret_cast<float*>(p.rad.ptr)}, pq[(nb + 1) & 1], sq,
                                                   QueueOut{qpath(nb), qshadow(nb), cap_e}, tnrm);
            pr.end(st);
            cap_prev = cap_e;
        }
        const int ga = clamp_grid(npix, accum_grid());
        pr.begin(st, RR_K_ACCUM);
        k_accumulate<<<ga, kBlock, 0, st>>>(fc, Rad{reinterpret_cast<float*>(p.rad.ptr)}, f.film.ptr, p.film_part.ptr, c == 0 ? 1 : 0, c == n_chunks - 1 ? 1 : 0,
                                            p.srgb_lut.ptr, reinterpret_cast<uchar4*>(f.rgba8.ptr));
        pr.end(st);
    }
}
}  // namespace

void render_frame_device(const DevMesh& m, DevBuild& s, DevPaths& p, DevFrame& f, const FrameConsts& base, int n_chunks,
                         FrameOpts o, hipStream_t st) {
    const int npix = base.npix;
    // the pixels the split path enumerates: the frame's, or a region's alone
    SplitConsts sc;
    static_cast<FrameConsts&>(sc) = base;
    sc.div_rw = FastDiv::make(1u);
    if (o.region_on) {
        sc.rx0 = o.region.x0;
        sc.ry0 = o.region.y0;
        sc.rw = o.region.w();
        sc.div_rw = FastDiv::make((uint32_t)sc.rw);
        sc.npix = o.region.w() * o.region.h();
    }
    const size_t npaths = (size_t)sc.npix * base.spp_chunk;
    f.tile_slices = 0;
    f.unit_logged = false;
    if (frame_uses_tiles(base, o.force_wavefront)) {  // one launch: all samples of every tile
        render_tiles_device(m, s, p, f, base, n_chunks, o, st);
        return;
    }
    f.film.ensure((size_t)npix);
    f.rgba8.ensure((size_t)npix * 4);
    const int cpc = counters_per_chunk(base.max_bounces);
    f.counters.ensure((size_t)cpc * n_chunks);
    RR_HIP(hipMemsetAsync(f.counters.ptr, 0, sizeof(int32_t) * cpc * n_chunks, st));
    if (base.n_tris <= 0) {  // nothing to hit: every sample is the world term
        f.prof.begin(st, RR_K_ACCUM);
        k_world<<<clamp_grid(npix, accum_grid()), kBlock, 0, st>>>(base, f.film.ptr, p.srgb_lut.ptr,
                                                                   reinterpret_cast<uchar4*>(f.rgba8.ptr));
        f.prof.end(st);
        RR_HIP(hipGetLastError());
        return;
    }
    p.ensure_paths(npaths);
    f.ensure_spill(p.grid_blocks);
    if (n_chunks > 1) p.film_part.ensure((size_t)sc.npix);
    unsigned long long* tc = nullptr;
    if (o.count_traversal) {
        f.trav_counts.ensure(kTravWords);
        RR_HIP(hipMemsetAsync(f.trav_counts.ptr, 0, kTravWords * sizeof(unsigned long long), st));
        tc = f.trav_counts.ptr;
    }
    PathQueue pq[2] = {{p.ps_o[0].ptr, p.ps_d[0].ptr, p.ps_t[0].ptr}, {p.ps_o[1].ptr, p.ps_d[1].ptr, p.ps_t[1].ptr}};
    ShadowQueue sq{p.sh_o.ptr, p.sh_d.ptr, p.sh_c.ptr};
    const SceneArgs sa{s.nodes.ptr, s.qnodes.ptr, s.tris.ptr, f.materials.ptr, f.lights.ptr, p.filter_table.ptr,
                       f.mat_lut.ptr, std::max(m.n_tris - 1, 1), m.n_tris, base.n_mats, base.n_lights, s.nq};
    render_split(p, f, sc, n_chunks, st, sa, tc, pq, sq, s.has4 ? s.tnrm.ptr : nullptr);
    RR_HIP(hipGetLastError());
}

namespace {
// sqrt_rn / sqrt_any / rcp_rn against the device's correctly rounded sqrtf
// and 1.0f / x over the float bit patterns [lo, lo + n): counts[0] = sqrt_rn
// mismatches with the argument in its range (+-0 or [2^-96, FLT_MAX]),
// counts[1] = sqrt_rn mismatches outside it, counts[2] = sqrt_any mismatches
// anywhere, counts[3] = rcp_rn mismatches with |x| in [2^-126, 2^126),
// counts[4] = rcp_rn mismatches outside (NaN equals NaN). 16 patterns a lane.
__global__ void k_debug_fastmath(uint32_t lo, uint64_t n, unsigned long long* __restrict__ counts) {
    unsigned long long c[5] = {0, 0, 0, 0, 0};
    const uint64_t first = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 16;
    auto same = [](float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); };
    for (uint64_t k = first; k < first + 16 && k < n; ++k) {
        const float x = __uint_as_float((uint32_t)(lo + k));
        const float ref = sqrtf(x);
        const bool in = (x >= 0x1p-96f && x <= 3.40282347e38f) || x == 0.0f;
        if (!same(sqrt_rn(x), ref)) ++c[in ? 0 : 1];
        if (!same(sqrt_any(x), ref)) ++c[2];
        const bool rin = fabsf(x) >= 0x1p-126f && fabsf(x) < 0x1p126f;
        if (!same(rcp_rn(x), 1.0f / x)) ++c[rin ? 3 : 4];
    }
    for (int i = 0; i < 5; ++i)
        if (c[i]) atomicAdd(&counts[i], c[i]);
}
}  // namespace

void fastmath_check_device(uint32_t lo, uint64_t n, unsigned long long* d_counts, hipStream_t st) {
    RR_HIP(hipMemsetAsync(d_counts, 0, 5 * sizeof(unsigned long long), st));
    const uint64_t per_block = (uint64_t)kBlock * 16;
    for (uint64_t off = 0; off < n; off += per_block << 16) {  // <= 65536 blocks per launch
        const uint64_t m = std::min<uint64_t>(n - off, per_block << 16);
        k_debug_fastmath<<<(unsigned)((m + per_block - 1) / per_block), kBlock, 0, st>>>((uint32_t)(lo + off), m,
                                                                                      d_counts);
    }
    RR_HIP(hipGetLastError());
}

void bsdf_batch_device(const float* d_mat12, const float* d_lut, const float n3[3], const float wo3[3], int n,
                       const float* d_u, float* d_wi, float* d_f, float* d_pdf, int32_t* d_ok, hipStream_t st) {
    if (n > 0)
        k_debug_bsdf<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(d_mat12, d_lut, mk3(n3[0], n3[1], n3[2]),
                                                                   mk3(wo3[0], wo3[1], wo3[2]), n, d_u, d_wi, d_f,
                                                                   d_pdf, d_ok);
    RR_HIP(hipGetLastError());
}

void trace_batch_device(const DevMesh& m, DevBuild& s, DevPaths& p, DevFrame& f, int n, const float4* d_rays,
                        float4* d_hits, int32_t* d_prims, uint8_t* d_occ, hipStream_t st, int width) {
    p.ensure_paths(1);
    f.ensure_spill(p.grid_blocks);
    const int g = (int)std::min<long>((n + kBlock - 1) / kBlock, p.grid_blocks);
    if (width == 5 || width == 7) {  // packet walk (7: beam) with a 4-entry stack: the HBM part runs
        if (!s.has4) throw std::runtime_error("BVH4 not built");
        if (n > 0) {
            if (width == 7)
                k_debug_packet<4, true><<<g, kBlock, 0, st>>>(s.qnodes.ptr, s.tris.ptr, m.n_tris, n, d_rays, d_hits,
                                                              d_prims, d_occ, f.spill.ptr);
            else
                k_debug_packet<4><<<g, kBlock, 0, st>>>(s.qnodes.ptr, s.tris.ptr, m.n_tris, n, d_rays, d_hits,
                                                        d_prims, d_occ, f.spill.ptr);
        }
    } else if (width == 4 || width == 6) {  // 6: the same walk with one LDS stack entry per lane
        if (!s.has4) throw std::runtime_error("BVH4 not built");
        if (n > 0) {
            if (width == 6)
                k_debug_trace4<1><<<g, kBlock, 0, st>>>(s.qnodes.ptr, s.tris.ptr, m.n_tris, n, d_rays, d_hits, d_prims,
                                                        d_occ, f.spill.ptr);
            else
                k_debug_trace4<kLdsStack><<<g, kBlock, 0, st>>>(s.qnodes.ptr, s.tris.ptr, m.n_tris, n, d_rays, d_hits,
                                                                d_prims, d_occ, f.spill.ptr);
        }
    } else if (n > 0)
        k_debug_trace<<<g, kBlock, 0, st>>>(s.nodes.ptr, s.tris.ptr, m.n_tris, n, d_rays, d_hits, d_prims, d_occ,
                                            f.spill.ptr);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
