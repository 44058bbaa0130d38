// Device side of the split path of large scenes (host side: wavefront.hip,
// render_split): the grouped queues, the chunk dealer, lane refill, the packet
// walks of camera rays, the trace / shade / accumulate / world kernels and the
// debug kernels of rr_debug_trace. Everything has internal linkage. Two units
// include it: wavefront.hip, which launches the kernels, and tiles.hip, which
// only needs them emitted ahead of k_tiles (see there).
#pragma once

#include "paths.hpp"

namespace rr {

namespace {

// Radiance record per path, 3 floats (12 B: dwordx3 loads/stores; a float4
// record moved 33 % more bytes through the primary / accumulate stream).
struct Rad {
    float* p;
    RR_D float3 get(size_t i) const {
        const float* q = p + 3 * i;
        return make_float3(q[0], q[1], q[2]);
    }
    RR_D void put(size_t i, float3 v) const {
        float* q = p + 3 * i;
        q[0] = v.x;
        q[1] = v.y;
        q[2] = v.z;
    }
};

// Dense queue state (SoA, ping-pong per bounce).
struct PathQueue {
    float4* o;  // origin.xyz, path id (int bits)
    float4* d;  // direction.xyz, lobe bounce counters (int bits)
    float4* t;  // throughput.xyz, 1 when the ray leaves a hull side of its triangle (hull_flags), else 0
};
struct ShadowQueue {
    float4* o;  // origin.xyz, path id (int bits)
    float4* d;  // direction.xyz, tmax
    float4* c;  // contribution.xyz, hull escape flag as in PathQueue::t
};

template <typename FloatP>
__device__ __forceinline__ void camera_ray(const FrameConsts& fc, FloatP filt, int pix,
                                           uint32_t key, float3& o, float3& d, float& tmin, float& tmax,
                                           const ScreenCull* cull = nullptr, bool* culled = nullptr) {
    const int py = (int)fc.div_w.div((uint32_t)pix);
    camera_ray_xy(fc, filt, pix - py * fc.W, py, key, o, d, tmin, tmax, cull, culled);
}

RR_D uint32_t wave_id() { return blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); }

RR_D GlobalView global_view(const SceneArgs& a) { return {a.nodes, a.tris, a.mats, a.lights, a.filter, a.mat_lut}; }

// ------------------------------------------------------------------------
// Split path for scenes that do not fit in LDS (C4/C5-sized BVHs): traversal
// and shading run as separate kernels so that the traversal kernels carry only
// the ray + traversal state (≤ 64 VGPRs, 8 waves per SIMD to hide the
// L2/MALL/HBM latency of the node fetches) and keep their lanes busy with
// lane refill: each wave owns a sequence of 64-ray chunks of the ray queue
// (trace_refill) and, when fewer than kRefillBelow of its lanes are still
// traversing, hands the idle lanes the next rays of its sequence (ballot
// prefix, no atomics). Finished rays write a hit record (t, leaf index) at
// their queue slot, which the shading kernel consumes in the same order.
//
// Queues here are GROUPED: a shading wave appends its ballot-compacted rays
// to group g = wave % kQGroups with one atomicAdd on that group's counter
// (counters 128 B apart). One counter per queue serialised the appends
// (device-scope atomics on one address: ~11 ns each, measured as >80 % of the
// shading kernels' time); 64 groups spread them over 64 lines. A consumer wave
// reads the 64 group counts into registers (one load per lane, no LDS, no
// barrier) and walks the groups in time order (QueueMap::slot_t, one shuffle
// per position). Queue order may vary between runs; what each
// path computes (and the per-path order of radiance additions) does not, so
// images stay bit-identical to the tile path's and the oracle's.
#ifndef RR_REFILL_BELOW
#define RR_REFILL_BELOW 52
#endif
constexpr int kRefillBelow = RR_REFILL_BELOW;
// Waves per SIMD of the trace kernels (their launch bounds: <= 64 VGPRs):
// 8 against 7 measured 02 / 03 frames at 64 spp -3.7 / -3.8 %, C5 at 16 spp
// -2.7 % (with the quantised wide hierarchy and windowed ray order; over round
// 1's BVH2 walk C5 had been slower at 8, 102 -> 113 ms).
#ifndef RR_TRACE_WAVES
#define RR_TRACE_WAVES 8
#endif
constexpr int kTraceWaves = RR_TRACE_WAVES;
// Threads per block of the per-lane trace kernels (k_trace_extend,
// k_shadow_refill). With 1024 two blocks fill a CU at 8 waves per SIMD, so the
// CU's 160 KB of LDS holds two copies of the hierarchy's top (kTopNodes) next
// to the blocks' stacks instead of eight, and the top can be deeper (512 nodes
// then, 768 now); measured against 256-thread blocks with 128 top nodes (per
// frame slice, 02 / 03 at 64 spp, C5 at 16 spp): 115.4 / 128.4 / 103.0 against
// 115.5 / 129.1 / 103.2 ms with the static deal, and 1024 with 128 nodes the
// same; with the dynamic deal (ChunkDealer) 84.2 / 89.8 / 73.7 against
// 84.8 / 90.2 / 74.5 ms (means of two rounds), so 1024.
#ifndef RR_TRACE_BLOCK
#define RR_TRACE_BLOCK 1024
#endif
constexpr int kTraceBlock = RR_TRACE_BLOCK;
constexpr int kTraceWavesPerBlock = kTraceBlock / 64;
// Hierarchy of the split path: the PLOC BVH2 collapsed to the quantised 6-wide
// hierarchy (measured, as a 4-wide one, against walking the PLOC BVH2 itself,
// C5 / 02 / 03 frames at 16 / 64 / 64 spp: 191 -> 139, 174 -> 149, 192 -> 160
// ms). Its walk is TravStateQ6D (rr_device.h: postponed leaf tests; the
// measurements against testing leaves at once are there).
constexpr int kQGroups = 64;   // append groups per queue (one lane each in QueueMap)
constexpr int kQStride = 32;   // words between group counters (128 B)

// map(k) -> slot is called by every lane of the wave (converged: QueueMap
// shuffles); ray_of(slot, ...) and done(k, slot, hit) per lane.
// Positions 0..count-1 are dealt to the waves in chunks of 64 in round-robin
// order (ChunkDealer: each XCD's waves take the XCD's share of that order from
// a counter of their own), so at any time the rays in flight on the
// whole chip come from one window of about 64 x waves positions: for camera
// rays one band of the image, for queued rays the entries the producer
// kernel appended at about the same time (QueueMap::slot_t). Rays of one
// window share most of the nodes they visit, and the window's working set
// stays in L2 (measured on C5: a contiguous range per wave spread the rays in
// flight over the whole frame). map(k) may return kNoSlot (a gap): that
// position holds no ray.
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
// This wave's rank with the waves ordered XCD by XCD (blocks b and b + 8 share
// an XCD, MI355X_MICROARCH.md): consecutive chunks go to one XCD, so each
// XCD's L2 serves one eighth of the window instead of all of it. kWpb: waves
// per block of the kernel.
template <int kWpb = kWavesPerBlock>
RR_D int xcd_wave_rank() {
    const int G = (int)gridDim.x, bx = (int)blockIdx.x, xcd = bx & 7;
    return __builtin_amdgcn_readfirstlane((xcd * (G >> 3) + min(xcd, G & 7) + (bx >> 3)) * kWpb +
                                          (int)(threadIdx.x >> 6));  // wave-uniform: SGPR
}
// Chunks of 64 positions (or packets) dealt to the waves of a trace kernel.
// The order is the round-robin one (wave w of nw: chunks w, w + nw, w + 2 nw,
// ...), dealt dynamically: the waves of one XCD take that XCD's share of it
// (chunks r nw + first .. r nw + first + n - 1 of round r, where first / n are
// the XCD's wave ranks) from a counter of its own, one atomic per chunk, so a
// wave whose rays finished early takes more instead of idling while the chip
// drains. Chunk ids of one wave still increase, and every id below the end
// is taken by some wave of its XCD. Against the static deal (each wave its own
// fixed chunks, no counter) per 02 / 03 / C5 frame slice, two interleaved
// rounds: 101.7 / 108.8 / 90.8 -> 84.6 / 90.0 / 73.8 ms
// (profiles/r4_ab_dynamic_dealing.txt). Every caller passes counters now. The
// static deal of a null `ctrs` is still here for one reason: the camera kernel
// takes `ctrs` as an argument, and without this branch its instructions change
// (profiles/split_cleanup.md), which wants a measurement of its own.
template <int kWpb>
struct ChunkDealer {
    uint32_t* ctr;  // this XCD's counter (null: static)
    int nw, w;      // waves of the launch, this wave's rank (xcd_wave_rank)
    int first, n;   // ranks of this XCD's waves
    int taken;      // static: chunks taken so far
    RR_D void init(uint32_t* ctrs) {
        const int G = (int)gridDim.x, xcd = (int)blockIdx.x & 7;
        nw = G * kWpb;
        w = xcd_wave_rank<kWpb>();
        first = (xcd * (G >> 3) + min(xcd, G & 7)) * kWpb;
        n = ((G >> 3) + (xcd < (G & 7) ? 1 : 0)) * kWpb;
        ctr = ctrs ? ctrs + xcd * kQStride : nullptr;
        taken = 0;
    }
    RR_D int take() {  // every lane of the wave (wave-uniform result)
        if (!ctr) return (taken++) * nw + w;
        uint32_t t = 0;
        if ((threadIdx.x & 63) == 0) t = atomicAdd(ctr, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)t, 0));
        return (int)(t / (uint32_t)n) * nw + first + (int)(t % (uint32_t)n);
    }
};
// The dealer's counters of a consumer of the grouped queue q: word `word` of
// the first 8 group-counter lines (the producer uses word 0 of each).
RR_D uint32_t* deal_ctrs(const uint32_t* q, int word) { return const_cast<uint32_t*>(q) + word; }

// Top of the quantised hierarchy in LDS for the trace kernels (Q6Nodes): the
// first kTopNodes nodes (breadth-first numbering: the four top levels of the
// 6-wide hierarchy and part of the fifth), copied by the block at launch.
// 768 nodes = 48 KB beside the 32 KB of 8-entry traversal stacks of a
// 1,024-thread block keep two blocks (8 waves per SIMD) per CU (rr_device.h
// kTraceLdsStack has the measurement; 256-thread blocks get 128 nodes = 8 KB).
// In the oracle's walk (tools/collapse_study.py) the nodes below 128 take 10.3
// of 02's 18.8 node visits per camera ray, 8.7 of 03's 19.9, 8.6 of C5's 16.9
// (below 512: 12.6, 10.6, 9.5). The copy against none, measured with 128 nodes
// of the 4-wide hierarchy per frame slice (C5 at 16 spp / 02 / 03 at 64 spp):
// 105.8 -> 101.4, 110.5 -> 107.0, 118.2 -> 115.9 ms.
#ifndef RR_TOP_NODES
#define RR_TOP_NODES (kTraceBlock >= 1024 ? 768 : 128)  // 768 with 8-entry LDS stacks (rr_device.h kTraceLdsStack)
#endif
constexpr int kTopNodes = RR_TOP_NODES;
static_assert((kTraceLdsStack * kTraceBlock * 4 + 64 * kTopNodes) * (2048 / kTraceBlock) <= 160 * 1024,
              "trace kernels: stack + top copy of 8 waves per SIMD must fit the CU's LDS");
RR_D Q6Nodes stage_top(const SceneArgs& sa, rr_f4v* top_shared) {
    lds_f4w* top = (lds_f4w*)top_shared;
    const int n = kTopNodes > 0 ? min(sa.n_qnodes, kTopNodes) : 0;
    const rr_f4v* src = reinterpret_cast<const rr_f4v*>(sa.qnodes);
    for (int i = threadIdx.x; i < 4 * n; i += kTraceBlock) top[i] = src[i];
    __syncthreads();
    return Q6Nodes{sa.qnodes, top, n};
}
// TS: TravStateQ6D (its box margins are per node; the BVH2 walk TravState needs
// the scene radius in start() and so does not compile here). Blocks of
// kTraceBlock threads; deal: the dealer's counters (deal_ctrs).
template <typename TS, typename NodeP, typename TriP, typename Stack, typename MapFn, typename RayFn, typename DoneFn>
RR_D void trace_refill(NodeP nodes, TriP tris, int n_tris, int count, Stack& st, TravCount& cnt,
                       uint32_t* deal, MapFn&& map, RayFn&& ray_of, DoneFn&& done) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    ChunkDealer<kTraceWavesPerBlock> dl;
    dl.init(deal);
    // chunks holding this wave's sequence positions next .. next + 63: c0 the
    // current one, c1 the one after (taken ahead, so its atomic is in flight
    // while the wave traces)
    int c0 = dl.take(), c1 = dl.take();
    int next = 0;  // wave-uniform cursor into this wave's sequence
    // position of the q-th ray of this wave's sequence (next <= q < next + 64)
    auto gpos = [&](int q) { return ((q >> 6) == (next >> 6) ? c0 : c1) * 64 + (q & 63); };
    TS ts;
    int j = -1;
    uint32_t js = 0;  // queue slot of ray j
    for (;;) {
        const uint64_t idle = __ballot(j < 0);
        if (gpos(next) < count && idle) {  // wave-uniform
            const int k = gpos(next + (int)__popcll(idle & below));
            const uint32_t ks = map(k < count ? k : count - 1);
            if (j < 0 && k < count && ks != kNoSlot) {
                float3 o, d;
                float tmin, tmax;
                ray_of(ks, o, d, tmin, tmax);
                ts.start(o, d, tmin, tmax);
                st.sp = 0;
                if (n_tris > 0) {
                    j = k;
                    js = ks;
                } else {
                    done(k, ks, ts.h);
                }
            }
            const int n0 = next;
            next += (int)__popcll(idle);
            if ((next >> 6) != (n0 >> 6)) {
                c0 = c1;
                c1 = dl.take();
            }
        }
        if (!__ballot(j >= 0)) {
            if (gpos(next) >= count) break;
            continue;
        }
        for (;;) {
            if (j >= 0 && ts.step(nodes, tris, st, cnt)) {
                done(j, js, ts.h);
                j = -1;
            }
            const int na = (int)__popcll(__ballot(j >= 0));
            if (na == 0 || (gpos(next) < count && na < kRefillBelow)) break;
        }
    }
}

RR_D float2 pack_hit(const Hit& h) { return make_float2(h.t, i2f(h.idx)); }
RR_D Hit unpack_hit(float2 v) {
    Hit h;
    h.t = v.x;
    h.idx = f2i(v.y);
    h.u = h.v = 0.0f;
    h.orig = -1;
    return h;
}

// Grouped queue: counters (kQGroups, kQStride words apart) + group capacity.
struct QueueIn {
    const uint32_t* ctr;
    uint32_t cap;       // slots per group
    uint32_t* total;    // block 0 records the queue length (ray statistics), may be null
};

// Per-wave view of a grouped queue: lane g holds group g's count; slot_t(m)
// maps a position to a queue slot with one shuffle (every lane of the wave
// must call it, each with its own m).
struct QueueMap {
    int cnt;     // this lane's group count
    int total;
    int span;    // positions of slot_t: 64 groups x the largest group count rounded up to 64
    uint32_t cap;
    RR_D void init(const QueueIn& q) {
        const int lane = threadIdx.x & 63;
        const int c = (int)q.ctr[lane * kQStride];
        int sum = c, mx = c;
        for (int off = 1; off < 64; off <<= 1) {
            sum += __shfl_xor(sum, off);
            mx = max(mx, __shfl_xor(mx, off));
        }
        cnt = c;
        total = sum;
        span = ((mx + 63) & ~63) * 64;
        cap = q.cap;
        if (q.total && blockIdx.x == 0 && threadIdx.x == 0) *q.total = (uint32_t)total;
    }
    // Time order: chunks of 64 entries, chunk c = entries 64 (c / 64) ..
    // 64 (c / 64) + 63 of group c % 64 (kNoSlot past that group's count).
    // Every producer wave appends its batch to its group in one piece as it
    // goes, so a chunk holds the rays of about one producer batch (coherent
    // within the consumer wave), and equal offsets in different groups were
    // appended at about the same time, by waves working on one window of their
    // own input (measured on C5 at 16 spp: extend 53.7 -> 49.9 ms, shadow
    // 42.8 -> 39.9 ms against each wave walking a contiguous range of the
    // group-concatenated order).
    // The trace kernels take this order as it is. Sorting each window of 4096
    // positions by a direction bin first (round 6: octahedral map, 16 / 64 /
    // 256 bins in Morton order, a stable per-window multisplit kernel, bit-exact
    // frames) was measured and rejected, profiles/r6_ab_ray_sort.txt (C5 at 16
    // spp, 02 / 03 at 64 spp, best solo slice of two interleaved rounds):
    // extension rays sorted, 64 bins, extension traversal + sort 28.21 -> 32.08
    // / 34.06 -> 36.83 / 37.83 -> 40.73 ms (+14 / +8 / +8 %); 16 / 256 bins +10
    // / +17 % on C5; shadow rays sorted 21.54 -> 22.30 / 26.41 -> 27.06 / 28.27
    // -> 29.02 ms; both, whole slices 68.8 -> 72.9 / 78.3 -> 81.8 / 85.1 ->
    // 88.8 ms. A producer batch is the continuing samples of ONE pixel: their
    // rays leave one point of one surface, and most bounce rays end nearby, so
    // the walk's lower levels (where the per-ray node and triangle fetches are)
    // are shared by the rays of a batch, whatever their directions. Grouping by
    // direction trades that origin coherence for a far-field coherence the
    // short diffuse rays rarely use (the same finding as round 4's global
    // origin-cell x octant buckets, +10 to +13 %). The sort's code is gone.
    RR_D uint32_t slot_t(int m) const {
        const int c = m >> 6;
        const int g = c & 63, off = ((c >> 6) << 6) + (m & 63);
        return off < __shfl(cnt, g) ? (uint32_t)g * cap + (uint32_t)off : kNoSlot;
    }
};

// Queue records (path and shadow queue) are written once, with non-temporal
// stores, and read by the next kernels: a frame's queues never fit in L2 or
// the MALL, so the hint only keeps them from evicting what the shading reads
// (shading 12.6 / 13.1 / 10.8 -> 11.4 / 12.0 / 9.9 ms per 02 / 03 / C5 slice,
// profiles/r4_ab_nt_queue_stores.txt). Hit records are stored and every record
// is loaded plainly: non-temporal hit stores and non-temporal loads by a
// record's last reader gained nothing (profiles/r4_ab_nt_queue_hits.txt) and
// were removed with the switch that selected them.
__device__ __forceinline__ void q_put(float4* p, float4 v) {
    const rr_f4v w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<rr_f4v*>(p));
}

// Grouped append: one atomicAdd per queue per wave on its group's counter.
struct QueueOut {
    uint32_t* ctr_path;    // path queue group counters
    uint32_t* ctr_shadow;  // shadow queue group counters
    uint32_t cap;          // slots per group (both queues)
};

__device__ __forceinline__ void emit_grouped(const ShadeOut& so, int pid, PathQueue out, ShadowQueue sq,
                                             const QueueOut& qo) {
    const uint64_t mc = __ballot(so.cont), ms = __ballot(so.shadow);
    const int lane = threadIdx.x & 63;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const uint32_t g = wave_id() % kQGroups;
    uint32_t bc = 0, bs = 0;
    if (lane == 0) {
        if (mc) bc = atomicAdd(qo.ctr_path + g * kQStride, (uint32_t)__popcll(mc));
        if (ms) bs = atomicAdd(qo.ctr_shadow + g * kQStride, (uint32_t)__popcll(ms));
    }
    bc = g * qo.cap + (uint32_t)__shfl((int)bc, 0);
    bs = g * qo.cap + (uint32_t)__shfl((int)bs, 0);
    if (so.cont) {
        const uint32_t s1 = bc + (uint32_t)__popcll(mc & below);
        q_put(out.o + s1, make_float4(so.o.x, so.o.y, so.o.z, i2f(pid)));
        q_put(out.d + s1, make_float4(so.d.x, so.d.y, so.d.z, i2f((int)so.lob)));
        q_put(out.t + s1, make_float4(so.T.x, so.T.y, so.T.z, so.esc ? 1.0f : 0.0f));
    }
    if (so.shadow) {
        const uint32_t s2 = bs + (uint32_t)__popcll(ms & below);
        q_put(sq.o + s2, make_float4(so.so.x, so.so.y, so.so.z, i2f(pid)));
        q_put(sq.d + s2, make_float4(so.sd.x, so.sd.y, so.sd.z, so.sdist));
        q_put(sq.c + s2, make_float4(so.sc.x, so.sc.y, so.sc.z, so.esc ? 1.0f : 0.0f));
    }
}

// Minimum waves per SIMD of the split path's shading kernels (their launch
// bounds; 1: the compiler's choice, 90 / 91 VGPRs = 5 waves). A/B switch: 6
// waves (80 VGPRs, 3 / 6 spill slots) made shading 10.3 / 10.4 / 34.2 ->
// 13.2 / 13.3 / 44.1 ms per 02 / 03 / C5 slice (profiles/r6_ab_shadow_beam.txt,
// sw6).
#ifndef RR_SHADE_WAVES
#define RR_SHADE_WAVES 1
#endif
constexpr int kShadeWaves = RR_SHADE_WAVES;

// Path index of the split path: p = pixel * spp_chunk + sample (FrameConsts
// div_spp), pixel-major, so that the 64 lanes of a chunk trace (and shade)
// samples of one or two pixels: nearly the same ray, the same nodes and
// triangles, which one wave's loads fetch together, and the rays in flight on
// the chip cover a band of pixels spp_chunk times narrower than in
// sample-major order. The per-path arrays (hits, radiance) are indexed by p.
RR_D void path_of(const FrameConsts& fc, uint32_t p, int& pix, int& sl) {
    pix = (int)fc.div_spp.div(p);
    sl = (int)p - pix * fc.spp_chunk;
}

// The full-frame pixel of a dense pixel of the split path (SplitConsts): itself, or on a region frame the
// region's pixel in row-major order. Wave-uniform branch on a kernel argument.
// RR_SPLIT_CONSTS: the constants these kernels take. tiles.hip, which compiles them only for their effect on
// k_tiles' code and never launches them, sets FrameConsts: with it the mapping is the identity and that unit's
// code is what it was before there were regions.
#ifndef RR_SPLIT_CONSTS
#define RR_SPLIT_CONSTS SplitConsts
#endif
RR_D int region_pix(const FrameConsts&, int dense) { return dense; }
RR_D int region_pix(const SplitConsts& fc, int dense) {
    if (fc.rw == 0) return dense;
    const int ry = (int)fc.div_rw.div((uint32_t)dense);
    return (fc.ry0 + ry) * fc.W + fc.rx0 + (dense - ry * fc.rw);
}

// Packet traversal with per-lane box tests: the camera kernel's walk until
// the beam (packet_trace_beam below) replaced it there. It stays because
// rr_debug_trace width 5 and its tests run it over arbitrary rays
// (k_debug_packet<kStack, false>), which the beam cannot take: those need not
// share an origin. One wave walks the quantised 6-wide hierarchy for the rays
// of its 64 lanes together, visiting the union of the nodes they need one node
// at a time. The node index is wave-uniform, so the 64 B node (and every leaf
// triangle) comes in through scalar loads, once per wave instead of once per
// lane, and each lane runs the same box and triangle tests as its own walk
// (q6_box_hits, leaf_test) against its own ray, with its own closest-hit bound.
// A lane tests every leaf the wave visits whose box its ray passes, so it
// meets every triangle its own walk would; the accept rule (smaller t, then
// smaller original id) makes the closest hit the same. Children are visited
// nearest first for the first lane that enters the node. For coherent rays
// this trades extra node visits per ray for one memory request per visit
// instead of 64 (measured per 02 / 03 frame at 64 spp: camera-ray traversal
// 24.2 -> 14.6, 21.8 -> 15.0 ms). It loses where the rays of a tile part ways
// early: C5, about one triangle per pixel, 23.6 -> 33.5 ms at 16 spp; and the
// shadow rays of camera hits (per-lane 39.7 / 46.8 ms, packets 121 / 86 ms on
// C5 / 02) are not coherent enough for it at all.
// act: the lane has a ray; stk: this wave's kStack LDS entries, gstk: its
// kPacketSpill further entries in HBM (the per-lane traversal stacks' spill
// area, which no other kernel uses while the packets trace: the stack's tail
// of a deep hierarchy), drops: the frame's drop counter (null: not counted).
// The stack pointer is wave-uniform, so both parts take one address per push.
// A push beyond both parts (a hierarchy some 880 levels deep) is dropped and
// counted at once.
constexpr int kPacketStack = 128;             // a node pushes <= 5: about 25 levels of the 6-wide hierarchy in LDS
constexpr int kPacketSpill = kSpillStack * 64;  // per wave in HBM (DevFrame::spill holds kSpillStack per lane)
template <bool kCount, int kStack = kPacketStack>
RR_D void packet_trace(const QNode6* __restrict__ nodes, const TriPack* __restrict__ tris, lds_int* stk,
                       int* __restrict__ gstk, uint32_t* __restrict__ drops, bool act, float3 o, float3 d, float tmin,
                       Hit& h, TravCount& cnt) {
    if (!__ballot(act)) return;
    const float3 iq = mk3(q4_rcp(d.x), q4_rcp(d.y), q4_rcp(d.z));
    const Shear sh = make_shear(d);
    int node = 0, sp = 0;
    for (;;) {
        const bool live = act;
        const QNode6 nd = nodes[node];  // wave-uniform: scalar loads
        const uint32_t imask = q6_inner(nd);
        float tn[kQWidth];
        const uint32_t hm = live ? q6_box_hits(nd, o, iq, tmin, h.t, tn) : 0u;
        if (kCount && live) ++cnt.nodes;
        // leaf children in slot order (a lane tests those its ray enters)
#pragma unroll
        for (int c = 0; c < kQWidth; ++c) {
            if (((imask >> c) & 1u) || !__ballot((hm >> c) & 1u)) continue;
            const int ti = (int)nd.a.y + c - __builtin_popcount(imask & ((1u << c) - 1u));
            const TriPack tp = load_tri(tris, ti);
            if ((hm >> c) & 1u) {
                if (kCount) ++cnt.tris;
                leaf_test(tp, ti, sh, o, tmin, h);
            }
        }
        // internal children some lane enters: the representative lane's nearest next
        uint32_t inner = 0;
#pragma unroll
        for (int c = 0; c < kQWidth; ++c)
            if (((imask >> c) & 1u) && __ballot((hm >> c) & 1u)) inner |= 1u << c;
        if (!inner) {
            if (sp == 0) break;
            --sp;
            node = __builtin_amdgcn_readfirstlane(sp < kStack ? stk[sp] : gstk[sp - kStack]);
            continue;
        }
        const uint64_t any = __ballot(hm != 0u);
        const int rl = (int)__builtin_ctzll(any);
        const uint32_t rh = (uint32_t)__builtin_amdgcn_readlane((int)hm, rl);
        int best = -1;
        float bt = 0.0f;
#pragma unroll
        for (int c = 0; c < kQWidth; ++c) {
            if (!((inner >> c) & 1u)) continue;
            const float tc = ((rh >> c) & 1u)
                                 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tn[c]), rl))
                                 : __builtin_huge_valf();
            if (best < 0 || tc < bt) {
                best = c;
                bt = tc;
            }
        }
        const int base = (int)nd.a.x;
#pragma unroll
        for (int c = kQWidth - 1; c >= 0; --c)
            if (c != best && ((inner >> c) & 1u)) {
                const int x = base + __builtin_popcount(imask & ((1u << c) - 1u));
                if (sp < kStack) {
                    stk[sp++] = x;
                } else if (sp < kStack + kPacketSpill) {
                    gstk[sp - kStack] = x;
                    ++sp;
                } else if (drops && (threadIdx.x & 63) == 0) {
                    atomicAdd(drops, 1u);  // a missed subtree
                }
            }
        node = __builtin_amdgcn_readfirstlane(base + __builtin_popcount(imask & ((1u << best) - 1u)));
    }
}

// Camera packets with one box test per child for the whole packet (the beam):
// what k_trace_primary_packet runs. Against packet_trace, camera traversal per
// 02 / 03 / C5 frame slice 10.06 / 11.08 / 11.48 -> 7.26 / 8.02 / 9.95 ms,
// whole slices -2.6 / -3.0 / -1.5 % (profiles/r5_ab_camera_beam.txt).
// Camera rays share their origin exactly (camera_ray_xy:
// fc.cam_pos, a pinhole) and their directions differ by a pixel's footprint, so
// the per-lane box tests of packet_trace compute 64 nearly equal answers per
// child. Here lanes 0..5 test child 0..5 once for the packet over the interval
// of the lanes' reciprocal directions: per axis the plane distances of the
// quantised box, widened by twice the node's margin m (q6_planes widens them
// by m), times the end of the interval that gives the smallest near / largest
// far distance; a child passes when the largest near (and the smallest tmin)
// is at most the smallest far (and the largest closest hit so far). The
// per-lane test's rounding stays under m/8 |iq| (every plane distance is at
// most 2^19 m, kBoxMargin), and so does this test's, so every child some
// lane's own test opens is opened (a superset; an axis whose reciprocals
// change sign in the packet does not cull). Leaf children that pass are
// tested by every lane that has a ray, with the lane's own watertight test and
// accept rule: each ray meets at least the triangles its own walk would test,
// and a triangle it meets beyond them is one whose box its own test rejects
// (so no hit of it is accepted), so the closest hit is the same (bit-exact).
// Internal children that pass are visited nearest first by the packet's near
// distance, the others pushed as in packet_trace (same stack and HBM part).
template <bool kCount, int kStack = kPacketStack>
RR_D void packet_trace_beam(const QNode6* __restrict__ nodes, const TriPack* __restrict__ tris, lds_int* stk,
                            int* __restrict__ gstk, uint32_t* __restrict__ drops, bool act, float3 o, float3 d,
                            float tmin, Hit& h, TravCount& cnt) {
    const uint64_t am = __ballot(act);
    if (!am) return;
    const int rl = (int)__builtin_ctzll(am);
    const float ox = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, o.x), rl));
    const float oy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, o.y), rl));
    const float oz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, o.z), rl));
    const int lane = (int)(threadIdx.x & 63);
    const Shear sh = make_shear(d);
    const float3 iq = mk3(q4_rcp(d.x), q4_rcp(d.y), q4_rcp(d.z));
    // packet intervals over the active lanes (wave-uniform)
    auto wred = [&](float x, bool mx) {
        x = act ? x : (mx ? -__builtin_huge_valf() : __builtin_huge_valf());
        for (int off = 32; off > 0; off >>= 1) {
            const float y = __shfl_xor(x, off);
            x = mx ? fmaxf(x, y) : fminf(x, y);
        }
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
    };
    const float ilx = wred(iq.x, false), ily = wred(iq.y, false), ilz = wred(iq.z, false);
    const float ihx = wred(iq.x, true), ihy = wred(iq.y, true), ihz = wred(iq.z, true);
    const float t_lo = wred(tmin, false);
    float t_hi = wred(h.t, true);
    int node = 0, sp = 0;
    for (;;) {
        const QNode6 nd = nodes[node];  // wave-uniform: scalar loads
        const uint32_t imask = q6_inner(nd);
        if (kCount && act) ++cnt.nodes;
        // this lane's child (lanes 0..5) against the packet
        bool pass = false;
        float tnear = 0.0f;
        if (lane < kQWidth) {
            const uint32_t eb = (uint32_t)f2i(nd.org.w);
            const float dx = nd.org.x - ox, dy = nd.org.y - oy, dz = nd.org.z - oz;
            const float m2 = 2.0f * fmaf(fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz)), kBoxMargin,
                                         ldexpf(255.0f * kBoxMargin, (int)((nd.c.w >> 8) & 255u) - 128));
            const int c = lane;
            const int s8 = c < 4 ? 8 * c : 0;
            const int s16 = c == 5 ? 8 : 0;
            // children 0..3: a byte of a.z, a.w, b.x (lo) / b.y, b.z, b.w (hi); 4, 5: byte pairs of c.x .. c.z
            const uint32_t qlx = c < 4 ? (nd.a.z >> s8) & 255u : ((nd.c.x & 0xffffu) >> s16) & 255u;
            const uint32_t qly = c < 4 ? (nd.a.w >> s8) & 255u : ((nd.c.x >> 16) >> s16) & 255u;
            const uint32_t qlz = c < 4 ? (nd.b.x >> s8) & 255u : ((nd.c.y & 0xffffu) >> s16) & 255u;
            const uint32_t qhx = c < 4 ? (nd.b.y >> s8) & 255u : ((nd.c.y >> 16) >> s16) & 255u;
            const uint32_t qhy = c < 4 ? (nd.b.z >> s8) & 255u : ((nd.c.z & 0xffffu) >> s16) & 255u;
            const uint32_t qhz = c < 4 ? (nd.b.w >> s8) & 255u : ((nd.c.z >> 16) >> s16) & 255u;
            // per axis: near / far distance over the packet's reciprocal interval [il, ih]
            auto axis = [&](float dd, int e, uint32_t ql, uint32_t qh, float il, float ih, float& nr, float& fr) {
                const float lo = dd + ldexpf((float)ql, e) - m2, hi = dd + ldexpf((float)qh, e) + m2;
                if (il > 0.0f) {  // every lane's iq >= 0: lo is the near plane
                    nr = lo * (lo >= 0.0f ? il : ih);
                    fr = hi * (hi >= 0.0f ? ih : il);
                } else if (ih < 0.0f) {  // every lane's iq < 0: hi is the near plane
                    nr = hi * (hi >= 0.0f ? il : ih);
                    fr = lo * (lo >= 0.0f ? ih : il);
                } else {
                    nr = -__builtin_huge_valf();
                    fr = __builtin_huge_valf();
                }
            };
            float n0, f0, n1, f1, n2, f2;
            axis(dx, (int)(eb & 255u) - 128, qlx, qhx, ilx, ihx, n0, f0);
            axis(dy, (int)((eb >> 8) & 255u) - 128, qly, qhy, ily, ihy, n1, f1);
            axis(dz, (int)((eb >> 16) & 255u) - 128, qlz, qhz, ilz, ihz, n2, f2);
            tnear = fmaxf(fmaxf(n0, n1), fmaxf(n2, t_lo));
            const float tfar = fminf(fminf(f0, f1), fminf(f2, t_hi));
            pass = tnear <= tfar && ((nd.c.w >> c) & 1u);
        }
        const uint32_t hm = (uint32_t)__ballot(pass);
        // leaf children that pass: every lane with a ray tests its ray
        uint32_t leaves = hm & ~imask;
        if (leaves) {
            do {
                const int c = __builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const int ti = (int)nd.a.y + c - __builtin_popcount(imask & ((1u << c) - 1u));
                const TriPack tp = load_tri(tris, ti);
                if (act) {
                    if (kCount) ++cnt.tris;
                    leaf_test(tp, ti, sh, o, tmin, h);
                }
            } while (leaves);
            t_hi = wred(h.t, true);  // the packet's largest closest hit so far
        }
        const uint32_t inner = hm & imask;
        if (!inner) {
            if (sp == 0) break;
            --sp;
            node = __builtin_amdgcn_readfirstlane(sp < kStack ? stk[sp] : gstk[sp - kStack]);
            continue;
        }
        // nearest internal child by the packet's near distance (ties: lower slot) next
        int best = -1;
        float bt = 0.0f;
        for (uint32_t r = inner; r; r &= r - 1u) {
            const int c = __builtin_ctz(r);
            const float tc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tnear), c));
            if (best < 0 || tc < bt) {
                best = c;
                bt = tc;
            }
        }
        const int base = (int)nd.a.x;
        for (int c = kQWidth - 1; c >= 0; --c)
            if (c != best && ((inner >> c) & 1u)) {
                const int x = base + __builtin_popcount(imask & ((1u << c) - 1u));
                if (sp < kStack) {
                    stk[sp++] = x;
                } else if (sp < kStack + kPacketSpill) {
                    gstk[sp - kStack] = x;
                    ++sp;
                } else if (drops && lane == 0) {
                    atomicAdd(drops, 1u);  // a missed subtree
                }
            }
        node = __builtin_amdgcn_readfirstlane(base + __builtin_popcount(imask & ((1u << best) - 1u)));
    }
}

// Camera paths as packets: raygen + closest hit -> hits[p]. A wave traces 64
// consecutive path indices (path_of: the samples of one or two pixels) with
// packet_trace_beam; packets are dealt to
// the waves as trace_refill deals chunks (ChunkDealer, counters `deal`). An
// 8x8 tile of one sample per packet (round 3) measured 16.1 / 20.6 ms per
// 02 / 03 frame slice against 12.5 / 14.1.
template <bool kCount>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_trace_primary_packet(
    RR_SPLIT_CONSTS fc, SceneArgs sa, int np, float2* __restrict__ hits, uint32_t* __restrict__ deal,
    int32_t* __restrict__ spill, unsigned long long* __restrict__ tc, uint32_t* __restrict__ tail) {
    __shared__ int stack_all[kWavesPerBlock * kPacketStack];
    lds_int* stk = lds_slot(stack_all) + (threadIdx.x >> 6) * kPacketStack;
    int* const gstk = spill + (size_t)wave_id() * kPacketSpill;
    TravCount cnt;
    const ScreenCull cull = screen_cull(fc, sa.nodes);
    const int lane = threadIdx.x & 63;
    const int npk = (np + 63) / 64;
    ChunkDealer<kWavesPerBlock> dl;
    dl.init(deal);
    uint32_t n_traced = 0;
    for (int q = dl.take(); q < npk;) {
        const int qn = dl.take();  // the next packet, taken while this one traces
        const int p = q * 64 + lane;
        const bool valid = p < np;
        int pix, sl;
        path_of(fc, (uint32_t)(valid ? p : 0), pix, sl);
        pix = region_pix(fc, pix);
        const int py = (int)fc.div_w.div((uint32_t)pix), px = pix - py * fc.W;
        float3 o = mk3(0.0f, 0.0f, 0.0f), d = o;
        float tmin = 0.0f, tmax = -1.0f;
        bool culled = true;
        if (valid) {
            const uint32_t key = path_key(fc.seed, (uint32_t)pix, (uint32_t)(fc.first_sample + sl));
            camera_ray_xy(fc, sa.filter, px, py, key, o, d, tmin, tmax, &cull, &culled);
        }
        n_traced += valid && !culled ? 1u : 0u;
        Hit h;
        set_miss(h, tmax);
        packet_trace_beam<kCount>(sa.qnodes, sa.tris, stk, gstk, tail + 1, valid && !culled && fc.n_tris > 0, o, d,
                                  tmin, h, cnt);
        if (valid) hits[p] = pack_hit(h);
        q = qn;
    }
    for (int off = 32; off > 0; off >>= 1) n_traced += (uint32_t)__shfl_xor((int)n_traced, off);
    if (lane == 0 && n_traced) atomicAdd(tail, n_traced);
    if (kCount) flush_counts(tc, 0, cnt.nodes, cnt.tris);
}

// Camera paths: shade bounce 0 from hits[p]; appends the bounce-1 path queue
// and the bounce-0 shadow queue.
// In path-index order (pixel-major), so the bounce-0 shadow rays and the
// bounce-1 paths are queued with the samples of one pixel side by side.
__global__ __launch_bounds__(kBlock, kShadeWaves) void k_shade_primary(RR_SPLIT_CONSTS fc, SceneArgs sa, int np,
                                                          const float2* __restrict__ hits, Rad rad,
                                                          PathQueue out, ShadowQueue sq, QueueOut qo,
                                                          const float4* __restrict__ tnrm) {
    GlobalView v = global_view(sa);
    v.nrm = tnrm;
    const int stride = gridDim.x * kBlock;
    for (int b0 = blockIdx.x * kBlock; b0 < np; b0 += stride) {
        const int p = b0 + (int)threadIdx.x;
        ShadeOut so;
        so.cont = so.shadow = false;
        if (p < np) {
            int pix, sl;
            path_of(fc, (uint32_t)p, pix, sl);
            pix = region_pix(fc, pix);
            const uint32_t key = path_key(fc.seed, (uint32_t)pix, (uint32_t)(fc.first_sample + sl));
            float3 o, d;
            float tmin, tmax;
            camera_ray(fc, v.filter, pix, key, o, d, tmin, tmax);
            const Hit h = unpack_hit(hits[p]);
            float3 L = mk3(0.0f, 0.0f, 0.0f);
            shade(fc, 0, v, o, d, mk3(1.0f, 1.0f, 1.0f), 0u, h, key, L, so);
            rad.put(p, L);
        }
        emit_grouped(so, p, out, sq, qo);
    }
}

// Extension rays entering bounce b: closest hit -> hits[slot].
template <bool kCount>
__global__ __launch_bounds__(kTraceBlock, kTraceWaves) void k_trace_extend(SceneArgs sa, PathQueue in, QueueIn qi,
                                                                         float2* __restrict__ hits,
                                                                         int32_t* __restrict__ spill,
                                                                         unsigned long long* __restrict__ tc,
                                                                         uint32_t* __restrict__ tail) {
    __shared__ int lds_stack[kTraceLdsStack * kTraceBlock];
    __shared__ rr_f4v top_nodes[4 * (kTopNodes > 0 ? kTopNodes : 1)];
    const Q6Nodes nodes = stage_top(sa, top_nodes);
    QueueMap qm;
    qm.init(qi);
    TravStackT<kTraceBlock, kTraceLdsStack, kStackCap - kTraceLdsStack> st{lds_slot(lds_stack), spill,
                                                                        (int)(gridDim.x * kTraceBlock), 0, tail + 1};
    TravCount cnt;
    trace_refill<TravStateQ6D<false, kCount>>(
        nodes, sa.tris, sa.n_tris, qm.span, st, cnt, deal_ctrs(qi.ctr, 1), [&](int m) { return qm.slot_t(m); },
        [&](uint32_t i, float3& o, float3& d, float& tmin, float& tmax) {
            o = xyz(in.o[i]);
            d = xyz(in.d[i]);
            tmin = 0.0f;
            tmax = kFltMax;
        },
        [&](int, uint32_t i, const Hit& h) { hits[i] = pack_hit(h); });
    if (kCount) flush_counts(tc, 2, cnt.nodes, cnt.tris);
}

// Bounce b: shade from hits[slot], in the queue's time order (slot_t); appends
// the next path queue and this bounce's shadow queue.
__global__ __launch_bounds__(kBlock, kShadeWaves) void k_shade_extend(RR_SPLIT_CONSTS fc, int bounce, SceneArgs sa, PathQueue in,
                                                         QueueIn qi, const float2* __restrict__ hits,
                                                         Rad rad, PathQueue out, ShadowQueue sq,
                                                         QueueOut qo, const float4* __restrict__ tnrm) {
    QueueMap qm;
    qm.init(qi);
    const int count = qm.span;
    GlobalView v = global_view(sa);
    v.nrm = tnrm;
    const int stride = gridDim.x * kBlock;
    int pid = 0;
    for (int b0 = blockIdx.x * kBlock; b0 < count; b0 += stride) {
        const int j = b0 + (int)threadIdx.x;
        ShadeOut so;
        so.cont = so.shadow = false;
        const uint32_t i = qm.slot_t(j < count ? j : count - 1);  // all lanes (shuffles)
        if (j < count && i != kNoSlot) {
            const float4 a = in.o[i], b = in.d[i], c = in.t[i];
            pid = f2i(a.w);
            const Hit h = unpack_hit(hits[i]);
            int pix, sl;
            path_of(fc, (uint32_t)pid, pix, sl);
            pix = region_pix(fc, pix);
            const uint32_t key = path_key(fc.seed, (uint32_t)pix, (uint32_t)(fc.first_sample + sl));
            float3 L = rad.get(pid);
            shade(fc, bounce, v, xyz(a), xyz(b), xyz(c), (uint32_t)f2i(b.w), h, key, L, so);
            rad.put(pid, L);
        }
        emit_grouped(so, pid, out, sq, qo);
    }
}

// Shadow rays with lane refill: unoccluded -> radiance += contribution.
template <bool kCount>
__global__ __launch_bounds__(kTraceBlock, kTraceWaves) void k_shadow_refill(SceneArgs sa, ShadowQueue sq, QueueIn qi,
                                                                          Rad rad,
                                                                          int32_t* __restrict__ spill,
                                                                          unsigned long long* __restrict__ tc,
                                                                          uint32_t* __restrict__ tail) {
    __shared__ int lds_stack[kTraceLdsStack * kTraceBlock];
    __shared__ rr_f4v top_nodes[4 * (kTopNodes > 0 ? kTopNodes : 1)];
    const Q6Nodes nodes = stage_top(sa, top_nodes);
    QueueMap qm;
    qm.init(qi);
    TravStackT<kTraceBlock, kTraceLdsStack, kStackCap - kTraceLdsStack> st{lds_slot(lds_stack), spill,
                                                                        (int)(gridDim.x * kTraceBlock), 0, tail + 1};
    TravCount cnt;
    trace_refill<TravStateQ6D<true, kCount>>(
        nodes, sa.tris, sa.n_tris, qm.span, st, cnt, deal_ctrs(qi.ctr, 1), [&](int m) { return qm.slot_t(m); },
        [&](uint32_t i, float3& o, float3& d, float& tmin, float& tmax) {
            const float4 a = sq.o[i], b = sq.d[i];
            o = xyz(a);
            d = xyz(b);
            tmin = 0.0f;
            tmax = b.w;
        },
        [&](int, uint32_t i, const Hit& h) {
            if (h.idx >= 0) return;
            const int pid = f2i(sq.o[i].w);
            const float4 c = sq.c[i];
            float3 L = rad.get(pid);
            L.x = L.x + c.x;
            L.y = L.y + c.y;
            L.z = L.z + c.z;
            rad.put(pid, L);
        });
    if (kCount) flush_counts(tc, 4, cnt.nodes, cnt.tris);
}

// K11 (+K12 on the last chunk): film += radiance of this chunk's samples in
// sample order; then mean -> exposure -> view transform -> 8-bit.
// Film sum in the grouped order (kFilmGroup, rr_device.h): the open group's
// partial sum crosses chunk boundaries in `part` (touched only by frames of
// several chunks).
__global__ __launch_bounds__(kBlock) void k_accumulate(RR_SPLIT_CONSTS fc, Rad rad,
                                                       float4* __restrict__ film, float4* __restrict__ part,
                                                       int first_chunk, int last_chunk, const float* __restrict__ srgb,
                                                       uchar4* __restrict__ out) {
    for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < fc.npix; pix += gridDim.x * kBlock) {
        const int fpix = region_pix(fc, pix);  // the film's pixel; the records and `part` are dense
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), P = acc;
        if (!first_chunk) {
            acc = film[fpix];
            P = part[pix];
        }
        // the pixel's records are contiguous (path index pixel-major): read
        // four at a time as three float4 when the chunk allows it
        auto add = [&](int s, float x, float y, float z) {
            const int gs = fc.first_sample + s;
            if (gs > 0 && (gs & (kFilmGroup - 1)) == 0) {  // close the group
                acc.x = acc.x + P.x;
                acc.y = acc.y + P.y;
                acc.z = acc.z + P.z;
                P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            P.x = P.x + x;
            P.y = P.y + y;
            P.z = P.z + z;
        };
        const size_t r0 = (size_t)pix * fc.spp_chunk;
        int s = 0;
        if ((fc.spp_chunk & 3) == 0) {
            const float4* q = reinterpret_cast<const float4*>(rad.p + 3 * r0);
            for (; s < fc.spp_chunk; s += 4, q += 3) {
                const float4 a = q[0], b = q[1], c = q[2];
                add(s, a.x, a.y, a.z);
                add(s + 1, a.w, b.x, b.y);
                add(s + 2, b.z, b.w, c.x);
                add(s + 3, c.y, c.z, c.w);
            }
        }
        for (; s < fc.spp_chunk; ++s) {
            const float3 L = rad.get(r0 + s);
            add(s, L.x, L.y, L.z);
        }
        if (last_chunk) {
            acc.x = acc.x + P.x;
            acc.y = acc.y + P.y;
            acc.z = acc.z + P.z;
            out[fpix] = tonemap(fc, acc, srgb);
        } else {
            part[pix] = P;
        }
        film[fpix] = acc;
    }
}

// Scenes without triangles: every camera sample misses, its radiance is the
// world term (T = 1 at bounce 0, no clamp); the film is that term summed in
// the grouped order (in order within groups of kFilmGroup, the group sums in
// order), then tonemapped: what the oracle's radiance() gives for an empty
// hierarchy.
__global__ __launch_bounds__(kBlock) void k_world(FrameConsts fc, float4* __restrict__ film,
                                                  const float* __restrict__ srgb, uchar4* __restrict__ out) {
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int g0 = 0; g0 < fc.spp_total; g0 += kFilmGroup) {
        float3 P = mk3(0.0f, 0.0f, 0.0f);
        const int g1 = min(fc.spp_total, g0 + kFilmGroup);
        for (int s = g0; s < g1; ++s) add_to(P, fc.world);
        acc.x = acc.x + P.x;
        acc.y = acc.y + P.y;
        acc.z = acc.z + P.z;
    }
    const uchar4 px = tonemap(fc, acc, srgb);
    for (int pix = blockIdx.x * kBlock + threadIdx.x; pix < fc.npix; pix += gridDim.x * kBlock) {
        film[pix] = acc;
        out[pix] = px;
    }
}

__global__ void k_debug_trace(const BvhNode* __restrict__ nodes, const TriPack* __restrict__ tris, int n_tris,
                              int n, const float4* __restrict__ rays, float4* __restrict__ hits,
                              int32_t* __restrict__ prims, uint8_t* __restrict__ occ,
                              int32_t* __restrict__ spill) {
    __shared__ int lds_stack[kLdsStack * kBlock];
    const int gtid = blockIdx.x * kBlock + threadIdx.x;
    const int nthreads = gridDim.x * kBlock;
    TravStack st{lds_slot(lds_stack), spill, nthreads, 0, nullptr};
    TravCount cnt;
    for (int i = gtid; i < n; i += nthreads) {
        const float4 o = rays[2 * i], d = rays[2 * i + 1];
        Hit h;
        traverse<false>(nodes, tris, n_tris, xyz(o), xyz(d), o.w, d.w, st, h, cnt);
        hits[i] = make_float4(h.t, h.u, h.v, 0.0f);
        prims[i] = h.orig;
        Hit h2;
        occ[i] = traverse<true>(nodes, tris, n_tris, xyz(o), xyz(d), o.w, d.w, st, h2, cnt) ? 1 : 0;
    }
}

// BSDF sampling at one shading point for n draws (parity with oracle
// orc_bsdf_sample): the material as the frame kernels load it (mat_derive),
// the view terms once (bsdf_view), then bsdf_sample per (ul, u1, u2).
// ok: 0 the path ends, 1 diffuse lobe, 2 glossy lobe.
// f3: the BSDF value f (f * cosL / cosL, as the oracle's export reports it).
__global__ void k_debug_bsdf(const float* __restrict__ mat12, const float* __restrict__ lut, float3 N, float3 wo,
                             int n, const float* __restrict__ u, float* __restrict__ wi3, float* __restrict__ f3,
                             float* __restrict__ pdf, int32_t* __restrict__ ok) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Mat m = load_mat(mat12, 0);
    mat_derive(m);
    const BsdfView vw = bsdf_view(m, lut, N, wo);
    float3 wi = mk3(0.0f, 0.0f, 0.0f), f = wi;
    float p = 0.0f;
    bool glossy = false;
    const bool good = bsdf_sample(m, lut, vw, N, wo, u[3 * i], u[3 * i + 1], u[3 * i + 2], wi, f, p, glossy);
    if (good) {
        const float cosL = dot3(N, wi);
        f = mk3(f.x / cosL, f.y / cosL, f.z / cosL);
    }
    wi3[3 * i] = wi.x; wi3[3 * i + 1] = wi.y; wi3[3 * i + 2] = wi.z;
    f3[3 * i] = f.x; f3[3 * i + 1] = f.y; f3[3 * i + 2] = f.z;
    pdf[i] = p;
    ok[i] = good ? (glossy ? 2 : 1) : 0;
}

// rr_debug_trace width 5: the camera kernel's packet walk over arbitrary rays
// (64 per wave, closest hit) with a kStack-entry LDS packet stack, small enough
// to fill on any real hierarchy, so the stack's HBM part is exercised (the
// per-lane spill area, one kPacketSpill part per wave). Closest hit only:
// occluded is set to 255.
template <int kStack, bool kBeam = false>
__global__ __launch_bounds__(kBlock) void k_debug_packet(const QNode6* __restrict__ nodes,
                                                         const TriPack* __restrict__ tris, int n_tris, int n,
                                                         const float4* __restrict__ rays, float4* __restrict__ hits,
                                                         int32_t* __restrict__ prims, uint8_t* __restrict__ occ,
                                                         int32_t* __restrict__ spill) {
    __shared__ int stack_all[kWavesPerBlock * kStack];
    lds_int* stk = lds_slot(stack_all) + (threadIdx.x >> 6) * kStack;
    TravCount cnt;
    for (int b0 = blockIdx.x * kBlock; b0 < n; b0 += gridDim.x * kBlock) {  // block-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = make_float4(0.0f, 0.0f, 1.0f, -1.0f);
        if (i < n) {
            o = rays[2 * i];
            d = rays[2 * i + 1];
        }
        Hit h;
        set_miss(h, d.w);
        if constexpr (kBeam)  // the camera kernel's walk: rays of a packet must share their origin
            packet_trace_beam<false, kStack>(nodes, tris, stk, spill + (size_t)wave_id() * kPacketSpill, nullptr,
                                             i < n && n_tris > 0, xyz(o), xyz(d), o.w, h, cnt);
        else
            packet_trace<false, kStack>(nodes, tris, stk, spill + (size_t)wave_id() * kPacketSpill, nullptr,
                                        i < n && n_tris > 0, xyz(o), xyz(d), o.w, h, cnt);
        if (i >= n) continue;
        hits[i] = make_float4(h.t, h.u, h.v, 0.0f);
        prims[i] = h.orig;
        occ[i] = 255;
    }
}

// rr_debug_trace widths 4 and 6: the trace kernels' walk (TravStateQ6D, called
// as trace_refill's inner loop calls it: step() by the lanes that still have a
// ray) over arbitrary rays, closest hit then any hit.
// kL: LDS stack entries per lane (kLdsStack; 1 for width 6, which puts nearly
// every stack entry in the HBM part; the HBM part holds the rest of kStackCap)
template <int kL>
__global__ void k_debug_trace4(const QNode6* __restrict__ nodes, const TriPack* __restrict__ tris, int n_tris,
                               int n, const float4* __restrict__ rays, float4* __restrict__ hits,
                               int32_t* __restrict__ prims, uint8_t* __restrict__ occ,
                               int32_t* __restrict__ spill) {
    __shared__ int lds_stack[kL * kBlock];
    const int gtid = blockIdx.x * kBlock + threadIdx.x;
    const int nthreads = gridDim.x * kBlock;
    TravStackT<kBlock, kL> st{lds_slot(lds_stack), spill, nthreads, 0, nullptr};
    TravCount cnt;
    for (int i = gtid; i < n; i += nthreads) {
        const float4 o = rays[2 * i], d = rays[2 * i + 1];
        TravStateQ6D<false> ts;
        ts.start(xyz(o), xyz(d), o.w, d.w);
        st.sp = 0;
        if (n_tris > 0)
            while (!ts.step(nodes, tris, st, cnt)) {
            }
        hits[i] = make_float4(ts.h.t, ts.h.u, ts.h.v, 0.0f);
        prims[i] = ts.h.orig;
        TravStateQ6D<true> ta;
        ta.start(xyz(o), xyz(d), o.w, d.w);
        st.sp = 0;
        if (n_tris > 0)
            while (!ta.step(nodes, tris, st, cnt)) {
            }
        occ[i] = ta.h.idx >= 0 ? 1 : 0;
    }
}

}  // namespace

}  // namespace rr
