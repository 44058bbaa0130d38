// The tile path: LDS-resident scenes rendered by k_tiles, with
// its scene staging, camera masks, out-of-line continuation, k_tile_order,
// k_tiles_fold and the host launch (render_tiles_device). What it shares with
// the split path of large scenes (wavefront.hip) is in paths.hpp.
//
// A translation unit of its own because the Makefile builds this one without
// SLP vectorisation. Paired fp32 ops
// (v_pk_mul/add_f32) need their operands in aligned register pairs, and in the
// tile kernel's 128-VGPR budget the moves that build those pairs cost more
// VALU issue than the pairing saves: 04vs frame 5 2.33 -> 2.18 ms. The split
// path kernels keep SLP (k_trace_primary +46 % without it, 02 frame 60).
// Same arithmetic op for op either way (-ffp-contract=off in both TUs);
// k_tile_order and k_tiles_fold compile to the same instructions with and
// without it.
#pragma clang fp contract(off)

#include "paths.hpp"

// The split path's kernels are compiled into this unit too, ahead of the tile
// code, and never launched from it: shade<GlobalView> of k_shade_extend emits
// k_tiles' force-inlined helpers ahead of it, and without that the four
// k_tiles come out with other scheduling (profiles/tiles_split.md). Dropping
// this include is a change of k_tiles' code and wants its own measurement.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // those kernels, unused here
// with the frame's own constants: a region frame's pixel mapping (SplitConsts) is wavefront.hip's alone, and
// these copies stay the kernels k_tiles was measured beside
#define RR_SPLIT_CONSTS FrameConsts
#include "split_kernels.hpp"
#pragma clang diagnostic pop

namespace rr {

namespace {

// The frame constants shade() reads, for the out-of-line continuation of the
// tile kernel's paths (tiles_continue): passed by value, because a reference
// to the kernel's FrameConsts argument would put the whole struct in scratch.
struct ShadeConsts {
    float3 world;
    float clamp_indirect;
    int max_bounces, max_diffuse, max_glossy, n_lights, n_tris;
};

RR_D void lds_copy(lds_f4w* dst, const float4* __restrict__ src, int n4) {
    const rr_f4v* s = reinterpret_cast<const rr_f4v*>(src);
    for (int i = threadIdx.x; i < n4; i += kBlock) dst[i] = s[i];
}
// Hull flags of an LDS-resident scene's triangle i (oracle/rr_oracle.c
// tri_hull, the same float operations): bit 0 when every vertex of every
// triangle lies behind triangle i's plane on its front side (the cross(e1, e2)
// direction, e1 = v1 - v0, e2 = v2 - v0), up to 2^-12 of the vertex's distance
// from v0 times |n|_1; bit 1
// the same for the back side. A ray leaving the triangle on a side whose bit is
// set moves away from a plane the whole scene lies behind: it meets nothing, so
// its continuation misses and its shadow ray is unoccluded without a traversal
// (the tests skipped could only report rounding-level grazing hits). On 04vs /
// 01 (a cube) every face is such a side: no secondary ray is traversed. Kept in
// bits kHullShift.. of the staged material word (shade() reads that word anyway).
RR_D uint32_t hull_flags(lds_tri* tris, int n_tris, int i) {
    const TriPack s = load_tri(tris, i);
    const float3 v0 = xyz(s.p0), n = cross3(sub3(xyz(s.p1), v0), sub3(xyz(s.p2), v0));
    const float an = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
    bool front = true, back = true;
    for (int j = 0; j < n_tris; ++j) {
        const TriPack e = load_tri(tris, j);
        const float3 w[3] = {xyz(e.p0), xyz(e.p1), xyz(e.p2)};
        for (int k = 0; k < 3; ++k) {
            const float3 r = sub3(w[k], v0);
            const float h = dot3(n, r);
            const float lim = an * (fabsf(r.x) + fabsf(r.y) + fabsf(r.z)) * 0x1p-12f;
            front = front && h <= lim;
            back = back && -h <= lim;
        }
    }
    return (front ? 1u : 0u) | (back ? 2u : 0u);
}

// Screen rectangle of a triangle (pixels, one pixel of slack) and its three
// edge lines e[k] = (nx, ny, c): nx*x + ny*y + c >= 0 inside, |n| = 1, so the
// value is a signed distance in pixels. A triangle at or behind the camera
// plane, or degenerate on screen, keeps the unbounded rectangle / edges that
// every point satisfies. Returns whether the edge lines are the triangle's own
// and good to a small fraction of a pixel (every projected vertex within 2^16
// pixels of the origin: fp32 rounding of the line's offset stays below 2^-5 px).
RR_D bool tri_screen_rect(const FrameConsts& fc, const float3 p[3], float r[4], float e[3][3]) {
    float x0 = kFltMax, x1 = -kFltMax, y0 = kFltMax, y1 = -kFltMax;
    float fx[3], fy[3];
    for (int k = 0; k < 3; ++k) e[k][0] = e[k][1] = 0.0f, e[k][2] = 1.0f;
    for (int k = 0; k < 3; ++k) {
        const float3 v = sub3(p[k], fc.cam_pos);
        const float depth = -dot3(v, fc.cam_back);
        if (!(depth > 1.0e-4f)) {  // at or behind the camera plane: no bound, every tile keeps it
            r[0] = r[2] = -kFltMax;
            r[1] = r[3] = kFltMax;
            return false;
        }
        const float sx = dot3(v, fc.cam_right) / depth;
        const float sy = dot3(v, fc.cam_up) / depth;
        fx[k] = (sx / fc.half_w + 1.0f) * ((float)fc.W * 0.5f);
        fy[k] = (1.0f - sy / fc.half_h) * ((float)fc.H * 0.5f);
        x0 = fminf(x0, fx[k]);
        x1 = fmaxf(x1, fx[k]);
        y0 = fminf(y0, fy[k]);
        y1 = fmaxf(y1, fy[k]);
    }
    r[0] = x0 - 1.0f;  // a pixel of slack covers rounding, as screen_rect's
    r[1] = x1 + 1.0f;
    r[2] = y0 - 1.0f;
    r[3] = y1 + 1.0f;
    const float area = (fx[1] - fx[0]) * (fy[2] - fy[0]) - (fy[1] - fy[0]) * (fx[2] - fx[0]);
    if (!(fabsf(area) > 1.0e-3f)) return false;  // (near-)degenerate on screen: edges stay open
    const float sgn = area > 0.0f ? 1.0f : -1.0f;
    for (int k = 0; k < 3; ++k) {
        const int a = k, b = (k + 1) % 3;
        float nx = -(fy[b] - fy[a]) * sgn, ny = (fx[b] - fx[a]) * sgn;  // towards the third vertex
        const float len = sqrtf(nx * nx + ny * ny);
        nx = nx / len;
        ny = ny / len;
        e[k][0] = nx;
        e[k][1] = ny;
        e[k][2] = -(nx * fx[a] + ny * fy[a]);
    }
    return fmaxf(fmaxf(fabsf(x0), fabsf(x1)), fmaxf(fabsf(y0), fabsf(y1))) <= 0x1p16f;
}

RR_D float l1norm(float3 a) { return fabsf(a.x) + fabsf(a.y) + fabsf(a.z); }

// Inverse-depth plane of a triangle: along the camera ray through the sample
// position (fx, fy) (pixels, camera_ray_xy's), the triangle's plane lies at
// depth z along the camera axis with 1 / z = w(fx, fy) = pl[0] fx + pl[1] fy +
// pl[2], affine because the ray is cam_pos + z (sx right + sy up - back) with
// sx, sy affine in fx, fy: n . (z s) = n . (p0 - cam_pos) = d0, so
// w = n . s / d0. w <= 0: the ray does not meet the plane in front of the
// camera. tile_mask compares these planes with an error allowance of
// 2^-10 M, M = |pl[0]| W + |pl[1]| H + |pl[2]| >= (|n.right| half_w +
// |n.up| half_h + |n.back|) / |d0|, which bounds |w| on the screen. The plane
// stays (0, 0, 0) — tile_mask then neither lets the triangle hide another nor
// drops it — unless the fp32 error of the coefficients is far below that
// allowance:
//   * the edges meet at a fair angle, |n|_1 >= 2^-4 |e1|_1 |e2|_1: the cross
//     product's rounding (four roundings per product pair, the pairs sum to
//     at most |e1|_1 |e2|_1: <= 2^-22 |e1|_1 |e2|_1; e1, e2 are single
//     subtractions of the staged vertices) is below 2^-18 |n|_1;
//   * the plane passes the camera at a fair distance, |d0| >= 2^-4 |n|_2
//     |p0 - cam_pos|_2 (p0 is seen more than 3.5 degrees off the plane): d0
//     is good to 2^-13 relative;
//   * the sensor's half extents lie in [2^-4, 1.5]: M >= 2^-4 |n|_2 / |d0|
//     and |s| <= 2.4, so the 2^-18 |n|_1 |s| / |d0| that n's rounding moves w
//     by is below 2^-12 M.
RR_D void tri_inv_depth_plane(const FrameConsts& fc, const float3 p[3], float pl[3]) {
    pl[0] = pl[1] = pl[2] = 0.0f;
    const float3 e1 = sub3(p[1], p[0]), e2 = sub3(p[2], p[0]);
    const float3 n = cross3(e1, e2), a = sub3(p[0], fc.cam_pos);
    const float an = l1norm(n), d0 = dot3(n, a);
    if (!(an >= 0x1p-4f * (l1norm(e1) * l1norm(e2)))) return;
    if (!(fabsf(d0) >= 0x1p-4f * (sqrtf(dot3(n, n)) * sqrtf(dot3(a, a)))) || !(fabsf(d0) > 0.0f)) return;
    if (!(fminf(fc.half_w, fc.half_h) >= 0x1p-4f) || !(fmaxf(fc.half_w, fc.half_h) <= 1.5f)) return;
    const float gx = dot3(n, fc.cam_right) * fc.half_w, gy = dot3(n, fc.cam_up) * fc.half_h;
    const float gz = -dot3(n, fc.cam_back);
    const float q0 = gx * fc.inv_w2 / d0, q1 = -(gy * fc.inv_h2) / d0, q2 = ((gz - gx) + gy) / d0;
    if (!(fabsf(q0) < 0x1p100f && fabsf(q1) < 0x1p100f && fabsf(q2) < 0x1p100f)) return;  // (also NaN)
    pl[0] = q0;
    pl[1] = q1;
    pl[2] = q2;
}

// Camera-ray data of one triangle (sorted index i), staged next to the scene
// by the kernels that trace camera rays of LDS-resident scenes: every camera
// ray starts at the camera, so woop_test's vertices relative to the origin,
// v - o, are computed once per block (the same float operations, so
// camera_hit's t / u / v are bit-identical to woop_test's) — in each of the
// three axis permutations of rot3, so that a ray reads its own (kz) with a
// per-lane LDS address instead of permuting per test (18 selects per triangle
// test) — and the triangle's screen rectangle (tri_screen_rect) bins it to the
// 8x8 tiles whose samples can hit it.
//   [13i + 3kz + k] = (rot3(v_k - o, kz), orig id for k = 0, else 0), kz, k = 0..2
//   [13i + 9] = (x0, x1, y0, y1), [13i + 10..12] = the screen edge lines
//   (nx, ny, c, pl[k]): their fourth words hold the inverse-depth plane
//   (tri_inv_depth_plane; zeros when the edge lines are open)
// Camera-ray data per triangle in LDS: the vertices relative to the camera in
// the three permutations (9 float4), the screen rectangle, the three screen
// edge lines with the inverse-depth plane in their spare words.
constexpr int kCamF4 = 13;
constexpr int kCamRect = 9;  // float4 offset of the screen rectangle, the edge lines follow
RR_D void stage_camera(lds_f4w* q, lds_tri* tris, int n_tris, const FrameConsts& fc) {
    for (int i = threadIdx.x; i < n_tris; i += kBlock) {
        const TriPack tp = load_tri(tris, i);
        const float3 pts[3] = {xyz(tp.p0), xyz(tp.p1), xyz(tp.p2)};
        float r[4], e[3][3], pl[3] = {0.0f, 0.0f, 0.0f};
        if (tri_screen_rect(fc, pts, r, e)) tri_inv_depth_plane(fc, pts, pl);
        for (int k = 0; k < 3; ++k) {
            const float3 a = sub3(pts[k], fc.cam_pos);
            for (int kz = 0; kz < 3; ++kz) {
                const float3 r = rot3(a, kz);
                rr_f4v x;
                x.x = r.x; x.y = r.y; x.z = r.z; x.w = k == 0 ? tp.p0.w : 0.0f;
                q[kCamF4 * i + 3 * kz + k] = x;
            }
        }
        rr_f4v c;
        c.x = r[0]; c.y = r[1]; c.z = r[2]; c.w = r[3];
        q[kCamF4 * i + kCamRect] = c;
        for (int k = 0; k < 3; ++k) {
            rr_f4v l;
            l.x = e[k][0]; l.y = e[k][1]; l.z = e[k][2]; l.w = pl[k];
            q[kCamF4 * i + kCamRect + 1 + k] = l;
        }
    }
}

// Stages the scene at the start of dynamic LDS (all threads call; ends with a
// barrier). `shading`: also materials, lights and the filter table. Returns the
// view; `used` receives the float4 slots taken (LDS layout: scene_lds_f4()).
// kCam: also stage the camera-ray data (stage_camera, from *cam_fc) after the
// scene. A compile-time switch, not a null test on cam_fc: comparing the
// address of the kernel's FrameConsts argument with null kept the whole
// struct in scratch (180 B per lane, every field read with a scratch load).
template <bool kCam = false>
RR_D LdsView stage_scene(lds_f4w* base, const SceneArgs& a, bool shading, int& used,
                         const FrameConsts* cam_fc = nullptr) {
    lds_f4w* q = base;
    LdsView v;
    v.nodes = (lds_node*)q;
    lds_copy(q, reinterpret_cast<const float4*>(a.nodes), 4 * a.n_nodes);
    q += 4 * a.n_nodes;
    v.tris = (lds_tri*)q;
    lds_copy(q, reinterpret_cast<const float4*>(a.tris), kTriF4 * a.n_tris);
    q += kTriF4 * a.n_tris;
    v.mats = v.lights = v.filter = v.lut = nullptr;
    if (shading) {
        v.mats = (lds_float*)q;
        lds_copy(q, reinterpret_cast<const float4*>(a.mats), 3 * a.n_mats);
        q += 3 * a.n_mats;
        v.lights = (lds_float*)q;
        lds_copy(q, reinterpret_cast<const float4*>(a.lights), 3 * a.n_lights);
        q += 3 * a.n_lights;
        v.filter = (lds_float*)q;
        lds_copy(q, reinterpret_cast<const float4*>(a.filter), kFilterN / 4);
        q += kFilterN / 4;
        v.lut = (lds_float*)q;
        lds_copy(q, reinterpret_cast<const float4*>(a.mat_lut), kMatLutStride / 4 * a.n_mats);
        q += kMatLutStride / 4 * a.n_mats;
    }
    if (shading || kCam) __syncthreads();  // the copies above are visible
    if (shading) {  // per-triangle unit normals, material ids and hull flags (shade() reads no TriPack)
        v.nrm = q;
        for (int i = threadIdx.x; i < a.n_tris; i += kBlock) {
            const TriPack tp = load_tri(v.tris, i);
            const float3 n = norm3(cross3(sub3(xyz(tp.p1), xyz(tp.p0)), sub3(xyz(tp.p2), xyz(tp.p0))));
            rr_f4v x;
            x.x = n.x; x.y = n.y; x.z = n.z;
            x.w = i2f(f2i(tp.p1.w) | (int)(hull_flags(v.tris, a.n_tris, i) << kHullShift));
            q[i] = x;
        }
        q += a.n_tris;
        v.matd = q;  // derived material records (view_mat)
        for (int i = threadIdx.x; i < a.n_mats; i += kBlock) {
            Mat m = load_mat(v.mats, i);
            mat_derive(m);
            rr_f4v r0, r1, r2, r3;
            r0.x = m.base.x; r0.y = m.base.y; r0.z = m.base.z; r0.w = m.roughness;
            r1.x = m.emission.x; r1.y = m.emission.y; r1.z = m.emission.z; r1.w = i2f(m.model);
            r2.x = m.alpha; r2.y = m.a2; r2.z = m.kd0; r2.w = i2f(m.spec_on);
            r3.x = m.cspec0.x; r3.y = m.cspec0.y; r3.z = m.cspec0.z; r3.w = 0.0f;
            q[kMatDF4 * i] = r0;
            q[kMatDF4 * i + 1] = r1;
            q[kMatDF4 * i + 2] = r2;
            q[kMatDF4 * i + 3] = r3;
        }
        q += kMatDF4 * a.n_mats;
        // the shading frame (T, B) = make_onb(N) of both sides of each
        // triangle, computed here once instead of per sample (the same
        // operations, so the same bits): side s at [kOnbF4 i + 2 s] = (T, B.x),
        // [kOnbF4 i + 2 s + 1] = (B.y, B.z, -, -)
        v.onb = q;
        __syncthreads();  // the normals above are visible
        for (int j = threadIdx.x; j < 2 * a.n_tris; j += kBlock) {
            const int i = j >> 1, side = j & 1;
            const float4 nm = lds_ld4(v.nrm + i);
            const float3 n = side ? mk3(-nm.x, -nm.y, -nm.z) : xyz(nm);
            float3 t, b;
            make_onb(n, t, b);
            rr_f4v x, y;
            x.x = t.x; x.y = t.y; x.z = t.z; x.w = b.x;
            y.x = b.y; y.y = b.z; y.z = 0.0f; y.w = 0.0f;
            q[kOnbF4 * i + 2 * side] = x;
            q[kOnbF4 * i + 2 * side + 1] = y;
        }
        q += kOnbF4 * a.n_tris;
    }
    if constexpr (kCam) {
        v.cam = q;
        stage_camera(q, v.tris, a.n_tris, *cam_fc);
        q += kCamF4 * a.n_tris;
    }
    used = (int)(q - base);
    __syncthreads();
    return v;
}

// Closest hit of a camera ray (origin fc.cam_pos) over the triangles whose bits
// are set in the wave-uniform mask {m0, m1} (sorted indices 0..127): woop_test
// with the staged vertices relative to the camera, closest_tri's accept rule. The
// rule is order-independent (smaller t, then smaller original id), so the
// result equals testing every triangle whenever the mask holds every triangle
// the ray can hit (tile_mask). LDS-resident scenes trace camera rays this way
// instead of walking the LBVH; oracle/rr_oracle.c brute-forces them the same.
template <bool kCount>
RR_D void camera_tris(const LdsView& v, uint64_t m0, uint64_t m1, const Shear& sh, int kz, float tmin, Hit& h,
                      TravCount& cnt) {
    for (int w = 0; w < 2; ++w) {
        uint64_t m = w ? m1 : m0;
        while (m) {
            const int i = (int)__builtin_ctzll(m) + 64 * w;
            m &= m - 1;
            if (kCount) ++cnt.tris;
            const lds_f4w* q = v.cam + kCamF4 * i + 3 * kz;  // this ray's permutation
            const float4 ca = lds_ld4(q), cb = lds_ld4(q + 1), cc = lds_ld4(q + 2);
            float t, u, vv;
            if (woop_core(sh, xyz(ca), xyz(cb), xyz(cc), t, u, vv)) {
                const int orig = f2i(ca.w);
                if (closer(t, orig, tmin, h)) {
                    h.t = t;
                    h.u = u;
                    h.v = vv;
                    h.idx = i;
                    h.orig = orig;
                }
            }
        }
    }
}
// The closest hit of a camera ray over the tile's mask (camera_tris with the
// ray's own shear axis). A wave-uniform axis (a scalar kz, no per-lane
// permutation or address offset; the camera rays of a tile nearly always share
// it) measured no faster (04vs / 01 pipelined 946 / 965 against 953 / 972
// frames/s) and is not kept.
template <bool kCount>
RR_D void camera_hit(const LdsView& v, uint64_t m0, uint64_t m1, float3 d, float tmin, float tmax, Hit& h,
                     TravCount& cnt) {
    set_miss(h, tmax);
    // camera_ray_xy: d = dw / |dw|
    const Shear sh = make_shear_unit(d);
    camera_tris<kCount>(v, m0, m1, sh, sh.kz, tmin, h, cnt);
}

// Triangles whose screen rectangle meets the sample positions of pixels
// [x0, x1] x [y0, y1] (centres + filter offsets below fc.filter_reach), as a
// wave-uniform 128-bit mask; n_tris <= 128 (every LDS-resident scene).
//
// Occlusion: a triangle that another one hides from every
// sample position of the expanded tile X0..X1 x Y0..Y1 is dropped from the
// mask. Triangle A covers the tile when the tile's worst corner lies inside
// each of A's edge lines by a pixel or more (the slack of the inclusion test,
// on the other side), A's inverse depth w_A (tri_inv_depth_plane) is positive
// over the tile and its depth there lies inside (clip_start, clip_end) — the
// ray parameters are those depths times the ray's length factor, which
// camera_ray_xy puts on tmin / tmax alike. Then every traced ray of the tile
// hits A at a t that `closer` accepts. Of the covering triangles the one with
// the largest lower bound lo_A of w over the tile (the nearest) is taken, and
// every triangle B with 0 < w_B over the tile and upper bound hi_B < lo_A
// goes: wherever a ray meets B, it meets A at a smaller t, so B is never the
// closest hit, and `closer` is order-independent. An affine function takes
// its extrema over a rectangle at the corners; lo / hi are those minus / plus
// 2^-10 (|a| W + |b| H + |c|), which is at least 2^-10 |w| (the relative
// margin that keeps ties, coplanar and interpenetrating triangles in the
// mask) and 2^2 times and more the fp32 error that tri_inv_depth_plane admits
// in the staged coefficients plus that of evaluating them here. A triangle
// without a plane (zeros) has lo = hi = 0: it neither covers nor goes, and A
// itself stays since hi_A >= lo_A.
//
// Covered by one: `covered` receives the covering triangle A
// when the final mask holds A alone, else -1 (wave-uniform). Then every sample
// position of the tile lies a pixel and more inside A's edges, in front of the
// camera and inside the clip range, and nothing else can be hit: the sample
// loop of tiles_body takes its single-triangle body. No arithmetic of its own:
// the index that set `best`, and a popcount.
#ifndef RR_TILES_COVERED
#define RR_TILES_COVERED 1  // 0: the single-triangle body compiled out (the reference of tests and A/B runs);
                            // 2: its per-unit values held in registers (step (b), measured and not kept)
#endif
RR_D void tile_mask(const FrameConsts& fc, const LdsView& v, int n_tris, float x0, float x1, float y0, float y1,
                    uint64_t& m0, uint64_t& m1, int& covered) {
    const float r = fc.filter_reach;
    const float X0 = x0 + 0.5f - r, X1 = x1 + 0.5f + r, Y0 = y0 + 0.5f - r, Y1 = y1 + 0.5f + r;
    const float Wf = (float)fc.W, Hf = (float)fc.H;
    constexpr float kEps = 0x1p-10f;
    uint64_t a = 0, b = 0;
    float best = 0.0f;  // the largest lo_A of a covering triangle (0: none covers)
    int best_i = -1;    // ... and that triangle
    for (int i = 0; i < n_tris; ++i) {
        const float4 q = lds_ld4(v.cam + kCamF4 * i + kCamRect);
        bool in = !(q.y < X0 || q.x > X1 || q.w < Y0 || q.z > Y1);
        bool cov = true;
        float pl[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 3 && in; ++k) {  // the expanded tile wholly outside an edge (+1 px of slack)
            const float4 l = lds_ld4(v.cam + kCamF4 * i + kCamRect + 1 + k);
            const float m = l.x * (l.x > 0.0f ? X1 : X0) + l.y * (l.y > 0.0f ? Y1 : Y0) + l.z;
            in = m >= -1.0f;
            // ... and wholly inside it by a pixel
            cov = cov && l.x * (l.x > 0.0f ? X0 : X1) + l.y * (l.y > 0.0f ? Y0 : Y1) + l.z >= 1.0f;
            pl[k] = l.w;
        }
        if (in) {
            if (i < 64) a |= 1ull << i;
            else b |= 1ull << (i - 64);
            if (cov) {
                const float e = kEps * (fabsf(pl[0]) * Wf + fabsf(pl[1]) * Hf + fabsf(pl[2]));
                const float lo = pl[0] * (pl[0] > 0.0f ? X0 : X1) + pl[1] * (pl[1] > 0.0f ? Y0 : Y1) + pl[2] - e;
                const float hi = pl[0] * (pl[0] > 0.0f ? X1 : X0) + pl[1] * (pl[1] > 0.0f ? Y1 : Y0) + pl[2] + e;
                if (lo > 0.0f && hi * fc.clip_start * (1.0f + kEps) < 1.0f && lo * fc.clip_end > 1.0f + kEps) {
                    if (lo > best) best_i = i;
                    best = fmaxf(best, lo);
                }
            }
        }
    }
    if (best > 0.0f) {
        for (int i = 0; i < n_tris; ++i) {
            const lds_f4w* l = v.cam + kCamF4 * i + kCamRect + 1;
            const float pa = lds_ld4(l).w, pb = lds_ld4(l + 1).w, pc = lds_ld4(l + 2).w;
            const float e = kEps * (fabsf(pa) * Wf + fabsf(pb) * Hf + fabsf(pc));
            const float lo = pa * (pa > 0.0f ? X0 : X1) + pb * (pb > 0.0f ? Y0 : Y1) + pc - e;
            const float hi = pa * (pa > 0.0f ? X1 : X0) + pb * (pb > 0.0f ? Y1 : Y0) + pc + e;
            if (lo > 0.0f && hi < best) {
                if (i < 64) a &= ~(1ull << i);
                else b &= ~(1ull << (i - 64));
            }
        }
    }
    m0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    m1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    covered = -1;
    if (RR_TILES_COVERED && best_i >= 0 && __popcll(m0) + __popcll(m1) == 1) {
        const int only = m0 ? (int)__builtin_ctzll(m0) : 64 + (int)__builtin_ctzll(m1);
        covered = only == __builtin_amdgcn_readfirstlane(best_i) ? only : -1;
    }
}

// K-tiles (LDS-resident scenes): one wave per 8x8 pixel tile
// runs every sample of its 64 pixels to completion — raygen, closest hit,
// shade, the NEE shadow ray traced inline, continuation — adds each path's
// radiance to its pixel's film sum in registers in sample order, then writes
// the film and the tonemapped pixel once. No radiance records, no queues, no
// accumulate pass: the per-path HBM stream of the wavefront kernels (12 B
// record written + read, 48 B per queued ray) disappears. A path's radiance
// additions keep their order (emission(0), NEE(0), emission(1), ...) and the
// film sum runs over samples 0..spp-1 like k_accumulate's, so the result is
// bit-identical to the wavefront kernels and to the oracle.
// Tiles come from an atomic counter (one atomic per wave per tile), those
// overlapping the scene's screen rectangle first: they carry the traversal
// and shading work, so the long tiles start early and the background tiles,
// whose samples are all culled camera rays, fill the tail.
constexpr int kTile = 8;  // 8x8 pixels = one wave
#ifndef RR_TILE_SHARDS
#define RR_TILE_SHARDS 8
#endif
constexpr int kTileShards = RR_TILE_SHARDS;  // k_tiles unit counters (one per block % 8)
constexpr int kTileCtrStride = 32;  // words between them (128 B)

struct TileOrder {
    int tx, n;               // tiles per row, tiles in the frame
    int bx0, by0, bw, bh;    // tile box over the screen rectangle (bw = bh = 0: none)
    // i-th tile: first the box row-major, then the rest row-major (wave-uniform).
    RR_D void at(int i, int& x, int& y) const {
        const int nb = bw * bh;
        if (i < nb) {
            y = i / bw;
            x = bx0 + (i - y * bw);
            y += by0;
            return;
        }
        int j = i - nb;
        const int ntop = by0 * tx;
        if (j < ntop) {
            y = j / tx;
            x = j - y * tx;
            return;
        }
        j -= ntop;
        const int rw = tx - bw, nmid = bh * rw;
        if (j < nmid) {
            const int r = j / rw, cx = j - r * rw;
            y = by0 + r;
            x = cx < bx0 ? cx : cx + bw;
            return;
        }
        j -= nmid;
        y = j / tx;
        x = j - y * tx;
        y += by0 + bh;
    }
};

// Tile box of the pixels whose samples can fall inside the screen rectangle
// (filter offsets are below 2 px). Scheduling only: every sample still takes
// its own culling test, so the box never changes a result.
RR_D TileOrder tile_order(const FrameConsts& fc, const ScreenCull& sc) {
    TileOrder to;
    to.tx = (fc.W + kTile - 1) / kTile;
    const int ty = (fc.H + kTile - 1) / kTile;
    to.n = to.tx * ty;
    to.bx0 = to.by0 = 0;
    to.bw = to.tx;
    to.bh = ty;
    if (!sc.on) return to;  // no rectangle: every tile may carry work
    const float m = fc.filter_reach + 1.0f;
    const float x0 = fmaxf(sc.r[0] - m, 0.0f), x1 = fminf(sc.r[1] + m, (float)fc.W - 1.0f);
    const float y0 = fmaxf(sc.r[2] - m, 0.0f), y1 = fminf(sc.r[3] + m, (float)fc.H - 1.0f);
    if (!(x0 <= x1 && y0 <= y1)) {
        to.bw = to.bh = 0;
        return to;
    }
    to.bx0 = (int)x0 / kTile;
    to.by0 = (int)y0 / kTile;
    to.bw = (int)x1 / kTile - to.bx0 + 1;
    to.bh = (int)y1 / kTile - to.by0 + 1;
    return to;
}

// A region frame (rr_set_region): the tiles that meet the region, in tile coordinates. Only they are work
// units: region_order is the frame's order cut to that rectangle, its tile indices and its box relative to
// the rectangle's corner (TileOrder::at then gives rectangle coordinates; the caller adds x0, y0). Partial
// tiles run whole; the film window (region.hip) drops their pixels outside the region.
struct TileRect {
    int x0, y0, w, h;
};
RR_D TileOrder region_order(const TileOrder& to, const TileRect& rt) {
    TileOrder r;
    r.tx = rt.w;
    r.n = rt.w * rt.h;
    r.bx0 = r.by0 = r.bw = r.bh = 0;
    const int bx0 = max(to.bx0, rt.x0), by0 = max(to.by0, rt.y0);
    const int bx1 = min(to.bx0 + to.bw, rt.x0 + rt.w), by1 = min(to.by0 + to.bh, rt.y0 + rt.h);
    if (to.bw > 0 && to.bh > 0 && bx0 < bx1 && by0 < by1) {
        r.bx0 = bx0 - rt.x0;
        r.by0 = by0 - rt.y0;
        r.bw = bx1 - bx0;
        r.bh = by1 - by0;
    }
    return r;
}

// Whether no sample of tile (tx, ty) can land inside the screen rectangle:
// every subpixel position is px + 0.5 + offset with |offset| < filter_reach
// (which includes a pixel of rounding slack), so each sample's own test in
// camera_ray_xy would cull it. Then every sample's radiance is exactly the
// world term (T = 1 at bounce 0, no clamp).
RR_D bool tile_culled(const FrameConsts& fc, const ScreenCull& sc, int tx, int ty) {
    if (!sc.on) return false;
    const float x0 = (float)(tx * kTile) + 0.5f, y0 = (float)(ty * kTile) + 0.5f;
    const float x1 = x0 + (float)(kTile - 1), y1 = y0 + (float)(kTile - 1);
    const float r = fc.filter_reach;
    return x1 + r < sc.r[0] || x0 - r > sc.r[1] || y1 + r < sc.r[2] || y0 - r > sc.r[3];
}

RR_D int uniform_i(int x) { return __builtin_amdgcn_readfirstlane(x); }
RR_D float uniform_f(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
RR_D ScreenCull uniform_cull(ScreenCull c) {
    c.on = uniform_i(c.on ? 1 : 0) != 0;
    for (int k = 0; k < 4; ++k) c.r[k] = uniform_f(c.r[k]);
    return c;
}
RR_D TileOrder uniform_order(TileOrder t) {
    t.tx = uniform_i(t.tx);
    t.n = uniform_i(t.n);
    t.bx0 = uniform_i(t.bx0);
    t.by0 = uniform_i(t.by0);
    t.bw = uniform_i(t.bw);
    t.bh = uniform_i(t.bh);
    return t;
}

// Per-lane ray counts of the tile kernel, reduced once per wave at exit into
// the chunk-0 counter pairs: {0, 1} = bounce 0, {2, 3} = all later bounces
// (frame.cpp fill_stats sums the pairs); tail = the chunk's words from
// camera_traced_slot on: [0] camera rays traced, [2] / [3] continuations /
// shadow rays traversed (the out-of-line traversals; the other continuations
// and shadow rays left a hull side and were resolved without a traversal,
// rr_frame_stats *_escaped).
RR_D void flush_rays(uint32_t* __restrict__ tot, uint32_t c0, uint32_t s0, uint32_t c1, uint32_t s1,
                     uint32_t* __restrict__ tail, uint32_t t0, uint32_t ext_traced, uint32_t sh_traced) {
    // the counts are wave totals (wave_count, TileTrav::wctr): lane 0 adds them
    const uint32_t v[4] = {c0, s0, c1, s1};
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 4; ++k)
            if (v[k]) atomicAdd(&tot[k], v[k]);
        if (t0) atomicAdd(&tail[0], t0);
        if (ext_traced) atomicAdd(&tail[2], ext_traced);
        if (sh_traced) atomicAdd(&tail[3], sh_traced);
    }
}

// The tile kernel's secondary traversals as out-of-line functions: on the
// scenes it renders they are rare (04vs / 01: a cube, every face a hull side,
// so no shadow or continuation ray is traversed but for the odd path through
// an edge crack), and inlined, their registers and control flow weighed on the
// whole sample loop (A/B, 40 pipelined frames: 04vs 886 -> 907, 01 901 -> 923
// frames/s; solo launches -1 %). Their state goes through the call's stack
// frame; the register budget stays at 4 waves per SIMD (5 measured slower
// solo, +-0 pipelined).
// Everything the out-of-line traversals need, passed by value: the traversal
// stack's LDS and HBM parts (the TravStack is built in the callee), the frame's
// drop counter, this wave's LDS counters (wctr: [0] continuations and [1]
// shadow rays of bounces >= 1, tiles_continue; [2] continuation and [3] shadow
// rays traversed, rr_frame_stats *_escaped) and the counting pass's totals
// (tc, null otherwise). Round 4 passed the stack and the counters by
// reference, which put them (and the LdsView) in scratch: written by every
// wave at launch, and every wave's scratch lines went back to HBM — most of
// k_tiles' 124-140 MB of PMC traffic per launch against 41 MB compulsory.
constexpr int kWctr = 8;  // LDS counter words per wave of k_tiles (TileTrav::wctr)
#ifndef RR_TILES_LOG_ALWAYS
#define RR_TILES_LOG_ALWAYS 0  // diagnostic builds: the unit log in every k_tiles launch, not only counting ones
#endif
struct TileTrav {
    lds_int* lds;
    int* spill;
    int stride;
    uint32_t* drops;
    lds_uint* wctr;  // this wave's kWctr LDS words: [0] / [1] bounce-1.. continuation / shadow rays, [2] / [3]
                     // traversed extension / shadow rays, counting launches: [4..7] their nodes / triangles
    unsigned long long* tc;
};
// Active lanes of the wave whose predicate holds: the tile kernel's ray
// counters are wave totals kept in scalar registers (no per-lane VGPRs live
// across the unit loop).
RR_D uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }
// *p += n by the first active lane (n: a wave total).
RR_D void wave_add(lds_uint* p, uint32_t n) {
    if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(__ballot(true))) *p += n;
}
template <bool kCount>
__device__ __noinline__ bool shadow_trace(LdsView v, int n_tris, float3 so, float3 sd, float dist, TileTrav tt) {
    wave_add(tt.wctr + 3, wave_count(true));
    TravStack st{tt.lds, tt.spill, tt.stride, 0, tt.drops};
    TravCount cnt;
    Hit hs;
    const bool occ = traverse<true, kCount>(v.nodes, v.tris, n_tris, so, sd, 0.0f, dist, st, hs, cnt);
    if (kCount) {  // the wave's LDS words, flushed once per wave (a global atomic per lane and call
                   // serialised the counting launch on one address)
        __hip_atomic_fetch_add(tt.wctr + 6, cnt.nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(tt.wctr + 7, cnt.tris, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return occ;
}
template <bool kCount>
__device__ __noinline__ Hit ext_trace(LdsView v, int n_tris, float3 o, float3 d, TileTrav tt) {
    wave_add(tt.wctr + 2, wave_count(true));
    TravStack st{tt.lds, tt.spill, tt.stride, 0, tt.drops};
    TravCount cnt;
    Hit h;
    traverse<false, kCount>(v.nodes, v.tris, n_tris, o, d, 0.0f, kFltMax, st, h, cnt);
    if (kCount) {
        __hip_atomic_fetch_add(tt.wctr + 4, cnt.nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(tt.wctr + 5, cnt.tris, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return h;
}
// The tile kernel's shadow rays, traced inside shade() (any hit over the
// LDS-resident LBVH).
template <bool kCount>
struct InlineShadow {
    static constexpr bool kInline = true;
    LdsView v;
    int n_tris;
    TileTrav tt;
    RR_D bool operator()(float3 so, float3 sd, float dist) const {
        return shadow_trace<kCount>(v, n_tris, so, sd, dist, tt);
    }
};

// Bounces 1 .. max_bounces of the tile kernel's paths whose camera hit
// continues into the scene (the continuation does not leave a hull side):
// out of line, so that the sample loop holds one shading point, bounce 0,
// with its bounce-dependent terms folded (dimensions, clamp, Russian
// roulette), and carries no bounce loop. On 04vs / 01 (a cube) no path gets
// here but for a camera ray through an edge crack. The same shade() calls in
// the same order as the loop it replaces, so the same bits. Measured against
// the loop (three interleaved rounds, 04vs / 01 frame 5 / 20 at 128 spp):
// solo 1.150 / 1.104 -> 1.068 / 1.021 ms, pipelined 995 / 1,030 -> 1,108 /
// 1,167 frames/s. Returns L; the wave totals of its continuations and shadow
// rays go to this wave's LDS counters tt.wctr[0..1]. (Built without
// -amdgpu-prealloc-sgpr-spill-vgprs, which makes hipcc 7.2 crash on the call.)
template <bool kCount>
__device__ __noinline__ float3 tiles_continue(ShadeConsts sc, LdsView v, float3 o, float3 d, float3 T, uint32_t lob,
                                              uint32_t key, float3 L, TileTrav tt) {
    uint32_t nc = 0, ns = 0;
    bool live = true;
    for (int b = 1; b <= sc.max_bounces; ++b) {
        if (!__any(live)) break;
        bool cont = false, shadow = false;
        if (live) {
            ShadeOut so;
            const Hit h = ext_trace<kCount>(v, sc.n_tris, o, d, tt);
            shade(sc, b, v, o, d, T, lob, h, key, L, so, InlineShadow<kCount>{v, sc.n_tris, tt});
            cont = so.cont;
            shadow = so.shadow;
            if (so.cont && so.esc) {  // leaves a hull side: the world term, as in tiles_body
                add_to(L, clamp_contrib(mul3(so.T, sc.world), sc.clamp_indirect));
                live = false;
            } else if (so.cont) {
                o = so.o;
                d = so.d;
                T = so.T;
                lob = so.lob;
            } else {
                live = false;
            }
        }
        nc += wave_count(cont);
        ns += wave_count(shadow);
    }
    wave_add(tt.wctr, nc);
    wave_add(tt.wctr + 1, ns);
    return L;
}

// RR_TILES_CONT_INPLACE: bit 0 the whole-tile variant, bit 1 the sample-group
// variant take the continuation inside shade() (else after it, from ShadeOut).
#ifndef RR_TILES_CONT_INPLACE
#define RR_TILES_CONT_INPLACE 1
#endif
// The bounce-0 continuation of k_tiles, taken over inside shade(): a ray that
// leaves a hull side of its triangle meets the world (T x world, clamped, as
// bounce 1's shade() would add it, and the path ends); any other goes on out
// of line (tiles_continue).
template <bool kCount>
struct TileCont {
    static constexpr bool kInline = true;
    ShadeConsts sc;
    LdsView v;
    TileTrav tt;
    uint32_t key;
    RR_D void operator()(float3 o, float3 d, float3 T, uint32_t lob, bool esc, float3& L) const {
        if (esc)
            add_to(L, clamp_contrib(mul3(T, sc.world), sc.clamp_indirect));
        else
            L = tiles_continue<kCount>(sc, v, o, d, T, lob, key, L, tt);
    }
};

// Sample-group slices of the box tiles (load balance: a heavy tile does not
// run as one wave's unit at the end of the launch). Slab of tile t: one plane
// per sample group g (group sum, 3 x 64 floats: x, y, z per lane), folded in
// group order by k_tiles_fold after the launch. (An in-launch hand-off — sc1
// stores, a ticket per tile, the last slice folding — measured 0.5 ms slower
// per 04vs frame than this second launch.)
}  // namespace
struct TileSlices {
    int n;             // slices per box tile = sample groups (1: no slicing)
    size_t floats;     // slab floats per tile: 192 * groups
    float* slab;
    const int32_t* order;  // box tiles in hand-out order (k_tile_order)
    uint32_t* cost;        // per screen tile: real-time ticks of its units, for the next launch's order; after
                           // them, per screen tile: samples run by the covered body (counting launches only)
};
namespace {

template <bool kCount, bool kWhole, bool kRegion = false>
RR_D void tiles_body(const FrameConsts& fc, const LdsView& v, uint32_t* __restrict__ tile_ctr, float4* __restrict__ film,
                     const float* __restrict__ srgb, uchar4* __restrict__ out, uint32_t* __restrict__ tot,
                     int32_t* __restrict__ spill, unsigned long long* __restrict__ tc, lds_int* stack,
                     const TileSlices sl, unsigned long long rt_entry, lds_uint* cont_ctr,
                     const TileRect rt = TileRect{0, 0, 0, 0}) {
    const int stride = gridDim.x * kBlock;
    // counting instantiation only: the wave's shader-clock and real-time
    // counters at start and end give the clock the kernel ran at (read-only
    // counters; the timed instantiation executes none of this)
    unsigned long long clk0 = 0, rt0 = 0;
    if (kCount) {
        clk0 = __builtin_amdgcn_s_memtime();
        rt0 = __builtin_amdgcn_s_memrealtime();
    }
    const TileTrav tt{stack, spill, stride, tot + drops_slot(fc.max_bounces), cont_ctr + kWctr * (threadIdx.x >> 6), tc};
    TravCount cp;
    uint32_t n_c0 = 0, n_s0 = 0, n_c1 = 0, n_s1 = 0, n_t0 = 0;
    // The screen rectangle and the tile order come from the root node in LDS,
    // so the compiler cannot tell they are wave-uniform and would keep (and
    // spill) them in VGPRs for the whole kernel: every lane holds the same
    // values, lane 0's copy goes to SGPRs.
    const ScreenCull cull = uniform_cull(screen_cull(fc, v.nodes));
    const TileOrder fto = uniform_order(tile_order(fc, cull));
    // kRegion: the units are the region's tiles alone; the costs stay indexed by the frame's screen tiles
    const TileOrder to = kRegion ? region_order(fto, rt) : fto;
    const int lane = threadIdx.x & 63;
    // Work units: each tile of the screen-rectangle box is cut into sl.n slices,
    // one per sample group; every other tile is one unit whose samples are all
    // culled (the world term). Those are dealt statically (wave w takes the
    // tiles nb + w, nb + w + waves, ...: no atomics for the cheap units); the
    // box slices come from n_shards = min(grid, kTileShards) counters, one per
    // group of blocks with equal blockIdx % n_shards (blocks are dealt
    // round-robin over the 8 XCDs, so a shard's atomics stay in one XCD's L2),
    // shard g handing out slices g, g + n_shards, ... One counter for every
    // unit serialised ~35k device-scope atomics on one address per 04vs frame.
    const int ng = (fc.spp_total + kFilmGroup - 1) / kFilmGroup;
    const int nb = to.bw * to.bh;
    const int n_slices = kWhole ? 1 : sl.n;
    const int n_sliced = nb * n_slices;
    const int n_units = n_sliced + (to.n - nb);  // box slices, then one unit per background tile
    const int n_shards = min((int)gridDim.x, kTileShards);  // small frames launch fewer blocks than shards
    const int shard = (int)blockIdx.x % n_shards;
    // Film value and 8-bit pixel of a background tile: every sample is the
    // world term, summed in the grouped order, the same bits for every pixel,
    // so the wave computes them once (wave-uniform, SGPRs) instead of per tile
    // (128 x 3 adds and a tonemap with its sRGB table reads per background tile).
    float4 bg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int g = 0; g < ng; ++g) {
        float3 P = mk3(0.0f, 0.0f, 0.0f);
        const int s_end = min(fc.spp_total, (g + 1) * kFilmGroup);
        for (int s = g * kFilmGroup; s < s_end; ++s) add_to(P, fc.world);
        bg.x = bg.x + P.x;
        bg.y = bg.y + P.y;
        bg.z = bg.z + P.z;
    }
    bg = make_float4(uniform_f(bg.x), uniform_f(bg.y), uniform_f(bg.z), 0.0f);
    const uchar4 bg_px = __builtin_bit_cast(uchar4, uniform_i(__builtin_bit_cast(int, tonemap(fc, bg, srgb))));
    for (;;) {
        int t, k = 0, nk = 1;  // tile, slice, slices of this tile
        int u = 0;
        if (lane == 0) u = (int)atomicAdd(tile_ctr + shard * kTileCtrStride, 1u);
        u = __builtin_amdgcn_readlane(u, 0) * n_shards + shard;
        if (u >= n_units) break;
        if (u < n_sliced) {  // box tiles in the order of k_tile_order (the heaviest first)
            const int j = kWhole ? u : u / n_slices;
            k = kWhole ? 0 : u - j * n_slices;
            nk = n_slices;
            t = uniform_i(sl.order[j]);
        } else {  // background tiles (the world term) fill the end of the launch
            t = nb + (u - n_sliced);
        }
        const unsigned long long u_start = __builtin_amdgcn_s_memrealtime();
        int tx, ty;
        to.at(t, tx, ty);
        if (kRegion) {
            tx += rt.x0;
            ty += rt.y0;
        }
        const int px = tx * kTile + (lane & (kTile - 1)), py = ty * kTile + (lane >> 3);
        const bool valid = px < fc.W && py < fc.H;
        const int pix = py * fc.W + px;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tile_culled(fc, cull, tx, ty)) {  // background tile: film = the world term, grouped sum (bg)
            if (k != 0) continue;             // (slice 0 does the whole tile)
            if (valid) {
                film[pix] = bg;
                out[pix] = bg_px;
            }
            continue;
        }
        // samples of this unit: group k of a sliced tile, else all of them
        const int s_lo = nk > 1 ? k * kFilmGroup : 0;
        const int s_hi = nk > 1 ? min(fc.spp_total, s_lo + kFilmGroup) : fc.spp_total;
        uint64_t cm0, cm1;
        int cov;
        tile_mask(fc, v, fc.n_tris, (float)(tx * kTile), (float)(tx * kTile + kTile - 1), (float)(ty * kTile),
                  (float)(ty * kTile + kTile - 1), cm0, cm1, cov);
        const uint32_t pk = pixel_key(fc.seed, (uint32_t)pix);
        // no triangle can be hit from this tile (wave-uniform): every sample is
        // the world term, summed as the sample loop would (0 + world + ...)
        const int s_run = (cm0 | cm1) != 0 ? s_hi : s_lo;
        // film sum order: in order within groups of kFilmGroup samples, the
        // group sums in order (one group per unit when tiles are sliced)
        float3 P = mk3(0.0f, 0.0f, 0.0f);
        auto group_end = [&](int s) {
            if ((s + 1) % kFilmGroup == 0 || s + 1 == s_hi) {
                acc.x = acc.x + P.x;
                acc.y = acc.y + P.y;
                acc.z = acc.z + P.z;
                P = mk3(0.0f, 0.0f, 0.0f);
            }
        };
        for (int s = s_run; s < s_hi; ++s) {
            add_to(P, fc.world);
            group_end(s);
        }
        // Covered tiles: triangle `cov` alone is in the mask and
        // covers every sample position of the tile, all 64 pixels lie inside
        // the image, no sample position lies outside the screen rectangle
        // (the expanded tile is inside it) and the scene has at most one
        // light. Then every lane is valid, no ray is culled and every ray
        // meets `cov`: the body below is the general one further down without
        // the predicates, the mask loop and the per-lane triangle index — the
        // same float operations per sample in the same order. A ray that
        // fails the test or the clip range all the same is a miss, as there.
        bool covered = cov >= 0 && tx * kTile + kTile <= fc.W && ty * kTile + kTile <= fc.H && fc.n_lights <= 1;
        if (covered && cull.on) {
            const float r = fc.filter_reach, cx = (float)(tx * kTile) + 0.5f, cy = (float)(ty * kTile) + 0.5f;
            covered = cx - r >= cull.r[0] && cx + (float)(kTile - 1) + r <= cull.r[1] && cy - r >= cull.r[2] &&
                      cy + (float)(kTile - 1) + r <= cull.r[3];
        }
        int s_gen = s_run;  // the samples left to the general body: none of a covered tile
        if (RR_TILES_COVERED && covered) {
            // the side every ray sees: dot(N, d) has the sign of dot(N, v0 - cam_pos) wherever the ray meets
            // the plane in front of the camera (w > 0 over the tile), and tri_inv_depth_plane admitted the
            // triangle only with |dot(N, v0 - cam_pos)| >= 2^-4 |v0 - cam_pos|
            const float4 nm = lds_ld4(v.nrm + cov), a0 = lds_ld4(v.cam + kCamF4 * cov);  // a0 = rot3(v0 - cam_pos, 0)
            const bool flip = uniform_i(dot3(xyz(nm), mk3(a0.z, a0.x, a0.y)) > 0.0f ? 1 : 0) != 0;
#if RR_TILES_COVERED == 2
            // step (b), measured and not kept: the unit's values read once, held wave-uniform across the loop
            CoveredHeld held;
            {
                const auto uf3 = [](float3 a) { return mk3(uniform_f(a.x), uniform_f(a.y), uniform_f(a.z)); };
                const int word = uniform_i(f2i(nm.w));
                held.mid = word & ((1 << kHullShift) - 1);
                held.esc = ((((uint32_t)word >> kHullShift) >> (flip ? 1 : 0)) & 1u) != 0u;
                held.N = uf3(flip ? mk3(-nm.x, -nm.y, -nm.z) : xyz(nm));
                const Mat m = view_mat(v, held.mid);
                held.m.base = uf3(m.base);
                held.m.roughness = uniform_f(m.roughness);
                held.m.emission = uf3(m.emission);
                held.m.model = uniform_i(m.model);
                held.m.alpha = uniform_f(m.alpha);
                held.m.a2 = uniform_f(m.a2);
                held.m.kd0 = uniform_f(m.kd0);
                held.m.spec_on = uniform_i(m.spec_on);
                held.m.cspec0 = uf3(m.cspec0);
                held.m.metallic = held.m.specular = held.m.ior = 0.0f;
                const lds_f4w* fr = v.onb + kOnbF4 * cov + (flip ? 2 : 0);
                const float4 tb = lds_ld4(fr), bb = lds_ld4(fr + 1);
                held.tb = uf3(xyz(tb));
                held.bb = uf3(mk3(tb.w, bb.x, bb.y));
                for (int k = 0; k < 11; ++k) held.lt[k] = fc.n_lights > 0 ? uniform_f(v.lights[k]) : 0.0f;
            }
#else
            const CoveredInLoop held;
#endif
            for (int s = s_lo; s < s_hi; ++s) {
                const uint32_t key = sample_key(pk, (uint32_t)s);
                float3 o, d, L = mk3(0.0f, 0.0f, 0.0f);
                float tmin, tmax;
                camera_ray_xy(fc, v.filter, px, py, key, o, d, tmin, tmax);
                n_t0 += 64u;
                const Shear sh = make_shear_unit(d);
                if (kCount) ++cp.tris;
                const lds_f4w* q = v.cam + kCamF4 * cov + 3 * sh.kz;  // this ray's permutation
                const float4 ca = lds_ld4(q), cb = lds_ld4(q + 1), cc = lds_ld4(q + 2);
                Hit h;
                set_miss(h, tmax);
                float t = tmax, u, vv;
                bool hit = woop_core(sh, xyz(ca), xyz(cb), xyz(cc), t, u, vv);
                hit = hit && closer(t, f2i(ca.w), tmin, h);
                h.t = hit ? t : tmax;
                ShadeOut so;
                const ShadeConsts sc{fc.world, fc.clamp_indirect, fc.max_bounces, fc.max_diffuse, fc.max_glossy,
                                     fc.n_lights, fc.n_tris};
                if constexpr ((RR_TILES_CONT_INPLACE & (kWhole ? 1 : 2)) != 0) {
                    shade_covered(fc, 0, v, cov, flip, hit, o, d, mk3(1.0f, 1.0f, 1.0f), 0u, h, key, L, so,
                                  InlineShadow<kCount>{v, fc.n_tris, tt}, TileCont<kCount>{sc, v, tt, key}, held);
                } else {
                    shade_covered(fc, 0, v, cov, flip, hit, o, d, mk3(1.0f, 1.0f, 1.0f), 0u, h, key, L, so,
                                  InlineShadow<kCount>{v, fc.n_tris, tt}, EmitCont{}, held);
                    if (so.cont) TileCont<kCount>{sc, v, tt, key}(so.o, so.d, so.T, so.lob, so.esc, L);
                }
                n_c0 += wave_count(so.cont);
                n_s0 += wave_count(so.shadow);
                add_to(P, L);
                group_end(s);
            }
            s_gen = s_lo;
            // counting launches: the samples this body ran, per tile, in the second half of the cost buffer
            // (rr_debug_tile_costs hands out the whole buffer; tests/test_gpu_tile_covered.py reads it)
            if (kCount && lane == 0) atomicAdd(&sl.cost[fto.n + ty * fto.tx + tx], (uint32_t)(s_hi - s_lo));
        }
        for (int s = s_lo; s < s_gen; ++s) {
            const uint32_t key = sample_key(pk, (uint32_t)s);
            float3 o = mk3(0.0f, 0.0f, 0.0f), d = o, L = o;
            float tmin = 0.0f, tmax = -1.0f;
            bool culled = true;
            if (valid) camera_ray_xy(fc, v.filter, px, py, key, o, d, tmin, tmax, &cull, &culled);
            n_t0 += wave_count(!culled);
            bool cont = false, shadow = false;
            if (valid) {  // bounce 0: the camera ray against the tile's triangles (wave-uniform masks)
                Hit h;
                set_miss(h, tmax);
                if (!culled) camera_hit<kCount>(v, cm0, cm1, d, tmin, tmax, h, cp);
                ShadeOut so;
                const ShadeConsts sc{fc.world, fc.clamp_indirect, fc.max_bounces, fc.max_diffuse, fc.max_glossy,
                                     fc.n_lights, fc.n_tris};
                if constexpr ((RR_TILES_CONT_INPLACE & (kWhole ? 1 : 2)) != 0) {
                    // the continuation (escape to the world, or bounces 1.. out of line) is taken inside
                    shade(fc, 0, v, o, d, mk3(1.0f, 1.0f, 1.0f), 0u, h, key, L, so,
                          InlineShadow<kCount>{v, fc.n_tris, tt}, TileCont<kCount>{sc, v, tt, key});
                } else {
                    shade(fc, 0, v, o, d, mk3(1.0f, 1.0f, 1.0f), 0u, h, key, L, so,
                          InlineShadow<kCount>{v, fc.n_tris, tt});
                    if (so.cont) TileCont<kCount>{sc, v, tt, key}(so.o, so.d, so.T, so.lob, so.esc, L);
                }
                cont = so.cont;
                shadow = so.shadow;
            }
            // counted with the whole wave active: a ballot inside `if (valid)`
            // would land in the counters of valid lanes only, and lane 0 (the
            // one flush_rays reads) may lie outside the image
            n_c0 += wave_count(cont);
            n_s0 += wave_count(shadow);
            add_to(P, L);
            group_end(s);
        }
        if (!kWhole && nk > 1) {  // one group of a sliced tile: its sum goes to the slab, k_tiles_fold adds them up
            float* const slab = sl.slab + (size_t)t * sl.floats + (size_t)k * 192;
            slab[lane] = acc.x;
            slab[64 + lane] = acc.y;
            slab[128 + lane] = acc.z;
        } else if (valid) {
            film[pix] = acc;
            out[pix] = tonemap(fc, acc, srgb);
        }
        if (lane == 0) {  // this unit's time, for the next launch's hand-out order (k_tile_order)
            const unsigned long long u_end = __builtin_amdgcn_s_memrealtime();
            atomicAdd(&sl.cost[ty * fto.tx + tx], (uint32_t)(u_end - u_start));
            if ((kCount || RR_TILES_LOG_ALWAYS) && u < kUnitLog) {  // the counting launch's unit log (device.hpp kUnitLog)
                tc[kTravWords + 2 * u] = u_start;
                tc[kTravWords + 2 * u + 1] = u_end;
            }
        }
    }
    uint32_t* const tail = tot + camera_traced_slot(fc.max_bounces);
    n_c1 = tt.wctr[0];  // the later bounces (tiles_continue)
    n_s1 = tt.wctr[1];
    flush_rays(tot, n_c0, n_s0, n_c1, n_s1, tail, n_t0, tt.wctr[2], tt.wctr[3]);
    if (kCount && lane == 0) {  // the secondary walks' node / triangle counts of this wave
        atomicAdd(&tc[2], (unsigned long long)tt.wctr[4]);
        atomicAdd(&tc[3], (unsigned long long)tt.wctr[5]);
        atomicAdd(&tc[4], (unsigned long long)tt.wctr[6]);
        atomicAdd(&tc[5], (unsigned long long)tt.wctr[7]);
    }
    if (kCount) {
        flush_counts(tc, 0, cp.nodes, cp.tris);
        const unsigned long long clk1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0) {  // device.hpp kTravWords
            atomicAdd(&tc[6], clk1 - clk0);
            atomicAdd(&tc[7], rt1 - rt0);
            atomicAdd(&tc[8], 1ull);
            atomicAdd(&tc[9], rt1 - rt_entry);
            atomicMax(&tc[10], ~rt_entry);  // the first entry, complemented (the words start at 0)
            atomicMax(&tc[11], rt1);
            atomicMax(&tc[12], rt_entry);  // the last entry
            atomicMax(&tc[13], ~rt1);      // the first end, complemented
        }
    }
}

// Waves per SIMD the register budget must admit: 4 (<= 128 VGPRs) for the
// sample-group slices of a frame rendered alone, 5 (<= 96 VGPRs, 42 spill
// slots) for the whole-tile units of frames that overlap a pending one — the
// bench's pipelined frames: 04vs / 01 992 / 1,026 against 953 / 970 frames/s
// at 4 (3 interleaved rounds of 40 frames), while a lone frame's slices ran
// 1.181 / 1.151 against 1.144 / 1.140 ms; 6 waves (80 VGPRs) 710 frames/s,
// 3 (137 VGPRs, no spill) 860.
#ifndef RR_TILES_WAVES
#define RR_TILES_WAVES 4
#endif
#ifndef RR_TILES_WAVES_WHOLE
#define RR_TILES_WAVES_WHOLE 5
#endif
// kWhole: one work unit per box tile (the frame overlaps a pending k_tiles
// frame, TileSlices.n == 1), a variant of its own so that the slab code is
// compiled out and a counter pass tells its launches from the sliced ones by
// name.
template <bool kCount, bool kWhole>
__global__ __launch_bounds__(kBlock, kWhole ? RR_TILES_WAVES_WHOLE : RR_TILES_WAVES) void k_tiles(FrameConsts fc,
                                                                                                 SceneArgs sa,
                                                                  uint32_t* __restrict__ tile_ctr,
                                                                  float4* __restrict__ film,
                                                                  const float* __restrict__ srgb,
                                                                  uchar4* __restrict__ out, uint32_t* __restrict__ tot,
                                                                  int32_t* __restrict__ spill,
                                                                  unsigned long long* __restrict__ tc,
                                                                  TileSlices sl) {
    const unsigned long long rt_entry = kCount ? __builtin_amdgcn_s_memrealtime() : 0ull;
    __shared__ int lds_stack[kLdsStack * kBlock];
    __shared__ uint32_t cont_ctr[kWctr * kWavesPerBlock];  // per wave: TileTrav::wctr
    extern __shared__ float4 dyn4[];
    lds_int* stack = lds_slot(lds_stack);
    if (threadIdx.x < kWctr * kWavesPerBlock) cont_ctr[threadIdx.x] = 0u;  // stage_scene ends with a barrier
    int used;
    const LdsView v = stage_scene<true>((lds_f4w*)dyn4, sa, true, used, &fc);
    tiles_body<kCount, kWhole>(fc, v, tile_ctr, film, srgb, out, tot, spill, tc, stack, sl, rt_entry,
                               (lds_uint*)cont_ctr);
}

// Hand-out order of k_tiles' box tiles (longest processing time first): the
// tiles of this frame's box sorted by the time their units took in the
// previous launch at the same screen tile (descending, over 128 log-spaced
// buckets; the order inside a bucket is arbitrary), so the heaviest units start
// first and the light rim and background units fill the end of the launch. On
// 04vs the heaviest tiles lie on the box's rim rows (the lit faces), which the
// box's row order handed out last, and the launch ended with those units
// running on a nearly empty chip. Scheduling only: every unit computes the
// same bits in any order. The same single-workgroup launch zeroes the costs
// for the coming launch, the unit counters and the ray counters.
constexpr int kOrderBuckets = 128;
constexpr int kOrderThreads = 1024;
RR_D int cost_bucket(uint32_t c) {
    if (c < 4u) return (int)c;
    const int e = 31 - __builtin_clz(c);
    return min(kOrderBuckets - 1, 4 * e + (int)((c >> (e - 2)) & 3u));
}
template <bool kRegion>
RR_D void tile_order_body(const FrameConsts& fc, const BvhNode* __restrict__ nodes, uint32_t* __restrict__ cost,
                          int32_t* __restrict__ order, uint32_t* __restrict__ tile_ctr,
                          uint32_t* __restrict__ ray_ctr, int n_ray_ctr, const TileRect rt) {
    __shared__ uint32_t cnt[kOrderBuckets];
    const int tid = threadIdx.x;
    const ScreenCull cull = screen_cull(fc, nodes);
    const TileOrder fto = tile_order(fc, cull);
    const TileOrder to = kRegion ? region_order(fto, rt) : fto;
    const int nb = to.bw * to.bh;
    for (int i = tid; i < kOrderBuckets; i += kOrderThreads) cnt[i] = 0u;
    for (int i = tid; i < kTileShards * kTileCtrStride; i += kOrderThreads) tile_ctr[i] = 0u;
    for (int i = tid; i < n_ray_ctr; i += kOrderThreads) ray_ctr[i] = 0u;
    __syncthreads();
    for (int t = tid; t < nb; t += kOrderThreads) {
        int x, y;
        to.at(t, x, y);
        if (kRegion) {
            x += rt.x0;
            y += rt.y0;
        }
        atomicAdd(&cnt[cost_bucket(cost[y * fto.tx + x])], 1u);
    }
    __syncthreads();
    if (tid == 0) {  // bucket starts, the heaviest bucket first
        uint32_t run = 0;
        for (int b = kOrderBuckets - 1; b >= 0; --b) {
            const uint32_t c = cnt[b];
            cnt[b] = run;
            run += c;
        }
    }
    __syncthreads();
    for (int t = tid; t < nb; t += kOrderThreads) {
        int x, y;
        to.at(t, x, y);
        if (kRegion) {
            x += rt.x0;
            y += rt.y0;
        }
        order[atomicAdd(&cnt[cost_bucket(cost[y * fto.tx + x])], 1u)] = t;
    }
    __syncthreads();
    for (int i = tid; i < fto.n; i += kOrderThreads) cost[i] = 0u;
}
__global__ __launch_bounds__(kOrderThreads) void k_tile_order(FrameConsts fc, const BvhNode* __restrict__ nodes,
                                                              uint32_t* __restrict__ cost, int32_t* __restrict__ order,
                                                              uint32_t* __restrict__ tile_ctr,
                                                              uint32_t* __restrict__ ray_ctr, int n_ray_ctr) {
    tile_order_body<false>(fc, nodes, cost, order, tile_ctr, ray_ctr, n_ray_ctr, TileRect{0, 0, 0, 0});
}

// Film of the sliced tiles: the group sums of each box tile that is not
// culled, added in group order (the same box and culling test as k_tiles,
// from the same root node), then tonemapped. One wave per tile.
template <bool kRegion>
RR_D void tiles_fold_body(const FrameConsts& fc, const BvhNode* __restrict__ nodes, const TileSlices& sl,
                          float4* __restrict__ film, const float* __restrict__ srgb, uchar4* __restrict__ out,
                          const TileRect rt) {
    const ScreenCull cull = screen_cull(fc, nodes);
    const TileOrder to = kRegion ? region_order(tile_order(fc, cull), rt) : tile_order(fc, cull);
    const int nb = to.bw * to.bh;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    for (int t = wave; t < nb; t += gridDim.x * kWavesPerBlock) {
        int tx, ty;
        to.at(t, tx, ty);
        if (kRegion) {
            tx += rt.x0;
            ty += rt.y0;
        }
        if (tile_culled(fc, cull, tx, ty)) continue;
        const int px = tx * kTile + (lane & (kTile - 1)), py = ty * kTile + (lane >> 3);
        if (px >= fc.W || py >= fc.H) continue;
        const float* slab = sl.slab + (size_t)t * sl.floats;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int g = 0; g < sl.n; ++g, slab += 192) {
            acc.x = acc.x + slab[lane];
            acc.y = acc.y + slab[64 + lane];
            acc.z = acc.z + slab[128 + lane];
        }
        const int pix = py * fc.W + px;
        film[pix] = acc;
        out[pix] = tonemap(fc, acc, srgb);
    }
}
__global__ __launch_bounds__(kBlock) void k_tiles_fold(FrameConsts fc, const BvhNode* __restrict__ nodes,
                                                       TileSlices sl, float4* __restrict__ film,
                                                       const float* __restrict__ srgb, uchar4* __restrict__ out) {
    tiles_fold_body<false>(fc, nodes, sl, film, srgb, out, TileRect{0, 0, 0, 0});
}

// The three kernels of a region frame: the same bodies over the region's tiles (TileRect). Kernels of their
// own, so that a frame without a region launches what it always did.
template <bool kCount, bool kWhole>
__global__ __launch_bounds__(kBlock, kWhole ? RR_TILES_WAVES_WHOLE : RR_TILES_WAVES) void k_tiles_region(
    FrameConsts fc, SceneArgs sa, uint32_t* __restrict__ tile_ctr, float4* __restrict__ film,
    const float* __restrict__ srgb, uchar4* __restrict__ out, uint32_t* __restrict__ tot, int32_t* __restrict__ spill,
    unsigned long long* __restrict__ tc, TileSlices sl, TileRect rt) {
    const unsigned long long rt_entry = kCount ? __builtin_amdgcn_s_memrealtime() : 0ull;
    __shared__ int lds_stack[kLdsStack * kBlock];
    __shared__ uint32_t cont_ctr[kWctr * kWavesPerBlock];
    extern __shared__ float4 dyn4[];
    lds_int* stack = lds_slot(lds_stack);
    if (threadIdx.x < kWctr * kWavesPerBlock) cont_ctr[threadIdx.x] = 0u;
    int used;
    const LdsView v = stage_scene<true>((lds_f4w*)dyn4, sa, true, used, &fc);
    tiles_body<kCount, kWhole, true>(fc, v, tile_ctr, film, srgb, out, tot, spill, tc, stack, sl, rt_entry,
                                     (lds_uint*)cont_ctr, rt);
}
__global__ __launch_bounds__(kOrderThreads) void k_tile_order_region(FrameConsts fc, const BvhNode* __restrict__ nodes,
                                                                     uint32_t* __restrict__ cost,
                                                                     int32_t* __restrict__ order,
                                                                     uint32_t* __restrict__ tile_ctr,
                                                                     uint32_t* __restrict__ ray_ctr, int n_ray_ctr,
                                                                     TileRect rt) {
    tile_order_body<true>(fc, nodes, cost, order, tile_ctr, ray_ctr, n_ray_ctr, rt);
}
__global__ __launch_bounds__(kBlock) void k_tiles_fold_region(FrameConsts fc, const BvhNode* __restrict__ nodes,
                                                              TileSlices sl, float4* __restrict__ film,
                                                              const float* __restrict__ srgb, uchar4* __restrict__ out,
                                                              TileRect rt) {
    tiles_fold_body<true>(fc, nodes, sl, film, srgb, out, rt);
}

// LDS-resident scenes render through k_tiles (RR_FLAG_WAVEFRONT: through the
// split trace / shade kernels of large scenes, the parity tests' second path).
// k_tiles slices a box tile into its sample groups: one unit per group, the
// group sums handed to the slice finishing last through a slab of one plane
// (3 x 64 floats) per group.
int film_groups(int spp) { return (spp + kFilmGroup - 1) / kFilmGroup; }
size_t tile_slab_bytes(int spp, long tiles) {
    const int ng = film_groups(spp);
    return ng > 1 ? (size_t)192 * sizeof(float) * ng * (size_t)tiles : 0;
}
constexpr size_t kTileSlabMax = (size_t)16 << 30;
// What stage_scene stages (without the camera data): the hierarchy and the
// triangle records, + the normals / shading frames (1 + kOnbF4 float4 per
// triangle) and the derived material records when shading.
size_t scene_lds_bytes(const FrameConsts& fc, bool shading) {
    const int n_nodes = std::max(fc.n_tris - 1, 1);
    size_t f4 = 4 * (size_t)n_nodes + kTriF4 * (size_t)fc.n_tris;
    if (shading)
        f4 += (3 + kMatDF4 + kMatLutStride / 4) * (size_t)fc.n_mats + 3 * (size_t)fc.n_lights + kFilterN / 4 +
              (size_t)(1 + kOnbF4) * fc.n_tris;
    return 16 * f4;
}
}  // namespace

// k_tiles' LDS per block: its static arrays (the traversal stack of kLdsStack
// entries per lane, kWctr counter words per wave: 12,416 B, as hipcc reports
// for every k_tiles instantiation) + the dynamic part TileGrid allocates — the
// staged scene (stage_scene) and the camera-relative vertices (stage_camera,
// kCamF4 float4 per triangle). ONE function for both the residency decision
// and the launch (VERDICT r5 Weak 7: the decision used to count only the
// hierarchy, triangles, materials, lights and filter table, about half of
// what the launch then allocated).
constexpr size_t kTilesStaticLds = sizeof(int) * (size_t)(kLdsStack * kBlock + kWctr * kWavesPerBlock);
size_t tiles_dyn_lds_bytes(const FrameConsts& fc) {
    return scene_lds_bytes(fc, true) + 16 * (size_t)kCamF4 * (size_t)fc.n_tris;
}
// A scene is LDS-resident (k_tiles) when one block's LDS leaves at least
// kTilesMinBlocks blocks per CU (160 KB; 3 x 4 waves = 3 waves per SIMD).
// Measured on dense soups in the 04vs stand-in (tools/lds_residency_study.py,
// profiles/r5_lds_residency.txt): k_tiles ahead of the split path down to 3
// blocks per CU (70 triangles: 19.2 against 20.0 ms), level at 2 (90: 20.3
// against 20.4 ms); below 3 the split path takes the scene. And at most 128
// triangles (camera_hit's per-tile triangle mask).
constexpr int kTilesMinBlocks = 3;
constexpr size_t kCuLds = 160 * 1024;
bool scene_in_lds(int n_tris, int n_mats, int n_lights) {
    FrameConsts fc{};
    fc.n_tris = n_tris;
    fc.n_mats = n_mats;
    fc.n_lights = n_lights;
    return n_tris > 0 && n_tris <= 128 &&
           kTilesMinBlocks * (kTilesStaticLds + tiles_dyn_lds_bytes(fc)) <= kCuLds;
}

bool frame_uses_tiles(const FrameConsts& base, bool force_wavefront) {
    const long n_tiles = (long)((base.W + 7) / 8) * ((base.H + 7) / 8);
    return scene_in_lds(base.n_tris, base.n_mats, base.n_lights) && !force_wavefront &&
           tile_slab_bytes(base.spp_total, n_tiles) <= kTileSlabMax;
}

long long tiles_pixels_run(int W, int H, bool region_on, const RegionRect& r) {
    if (!region_on) return (long long)W * H;
    const int x0 = r.x0 / kTile * kTile, y0 = r.y0 / kTile * kTile;
    const int x1 = std::min(W, (r.x1 + kTile - 1) / kTile * kTile), y1 = std::min(H, (r.y1 + kTile - 1) / kTile * kTile);
    return (long long)(x1 - x0) * (y1 - y0);
}

namespace {
// The tiles that meet a region of pixels (inside the frame, not empty; an unset one gives an empty rectangle).
TileRect region_tiles(const RegionRect& r) {
    if (r.empty()) return TileRect{0, 0, 0, 0};
    const int x0 = r.x0 / kTile, y0 = r.y0 / kTile;
    return TileRect{x0, y0, (r.x1 + kTile - 1) / kTile - x0, (r.y1 + kTile - 1) / kTile - y0};
}
// Launch geometry of k_tiles: the scene and the camera data staged in dynamic
// LDS (stage_scene, stage_camera), the resident grid for it.
struct TileGrid {
    decltype(&k_tiles<false, false>) kx;
    decltype(&k_tiles_region<false, false>) kxr = nullptr;  // a region frame's
    size_t dyn;
    int grid;
    TileGrid(const FrameConsts& fc, bool count, bool whole, bool region) {
        dyn = tiles_dyn_lds_bytes(fc);  // what scene_in_lds counted
        kx = count ? (whole ? k_tiles<true, true> : k_tiles<true, false>)
                   : (whole ? k_tiles<false, true> : k_tiles<false, false>);
        if (region) {
            kxr = count ? (whole ? k_tiles_region<true, true> : k_tiles_region<true, false>)
                        : (whole ? k_tiles_region<false, true> : k_tiles_region<false, false>);
            grid = grid_for(kxr, dyn);
        } else {
            grid = grid_for(kx, dyn);
        }
    }
};
}  // namespace

void render_tiles_device(const DevMesh& m, DevBuild& s, DevPaths& p, DevFrame& f, const FrameConsts& base, int n_chunks,
                         FrameOpts o, hipStream_t st) {
    const int npix = base.npix;
    const TileGrid G(base, o.count_traversal, o.tile_whole, o.region_on);
    if (p.grid_blocks == 0) p.grid_blocks = device_cu_count() * kMaxBlocksPerCu;
    f.ensure_spill(p.grid_blocks);  // k_tiles: only the traversal stack spill area
    f.film.ensure((size_t)npix);
    f.rgba8.ensure((size_t)npix * 4);
    const int cpc = counters_per_chunk(base.max_bounces);
    const long tiles = (long)((base.W + 7) / 8) * ((base.H + 7) / 8);
    const size_t n_ctr = (size_t)cpc * n_chunks;
    f.counters.ensure(n_ctr);  // zeroed by k_tile_order
    unsigned long long* tc = nullptr;
    if (o.count_traversal || RR_TILES_LOG_ALWAYS) {  // (RR_TILES_LOG_ALWAYS: diagnostic builds log every launch's units)
        f.trav_counts.ensure(kTravWords + 2 * kUnitLog);
        RR_HIP(hipMemsetAsync(f.trav_counts.ptr, 0, (kTravWords + 2 * kUnitLog) * sizeof(unsigned long long), st));
        tc = f.trav_counts.ptr;
        f.unit_logged = true;
    }
    const SceneArgs sa{s.nodes.ptr, s.qnodes.ptr, s.tris.ptr, f.materials.ptr, f.lights.ptr, p.filter_table.ptr,
                       f.mat_lut.ptr, std::max(m.n_tris - 1, 1), m.n_tris, base.n_mats, base.n_lights, s.nq};
    FrameConsts fc = base;
    fc.first_sample = 0;
    fc.spp_chunk = base.spp_total;
    uint32_t* tot = reinterpret_cast<uint32_t*>(f.counters.ptr);
    if (f.tile_cost.cap < 2 * (size_t)tiles) {  // costs of a new size start at 0 (the first order is the box's)
        f.tile_cost.ensure(2 * (size_t)tiles);
        RR_HIP(hipMemsetAsync(f.tile_cost.ptr, 0, sizeof(uint32_t) * tiles, st));
    }
    if (o.count_traversal)  // the covered body's sample counts of this launch (tiles_body)
        RR_HIP(hipMemsetAsync(f.tile_cost.ptr + tiles, 0, sizeof(uint32_t) * tiles, st));
    f.tile_order.ensure((size_t)tiles);
    // units: one per (box tile, sample group) when the frame runs alone, so
    // the heaviest tiles do not finish the launch on a nearly empty chip;
    // one per tile (every group of it, summed in order in the unit) when
    // the frame overlaps a pending one (o.tile_whole): the other frame's
    // waves fill the tail, and the slab writes and the fold launch go
    TileSlices sl{o.tile_whole ? 1 : film_groups(base.spp_total), (size_t)192 * film_groups(base.spp_total), nullptr,
                  f.tile_order.ptr, f.tile_cost.ptr};
    f.tile_slices = sl.n;
    // a region frame: only the tiles that meet the region are units, and the slab holds those alone
    const TileRect rt = region_tiles(o.region);
    const long tiles_run = o.region_on ? (long)rt.w * rt.h : tiles;
    if (sl.n > 1) {
        f.tile_slab.ensure(sl.floats * (size_t)tiles_run);
        sl.slab = f.tile_slab.ptr;
    }
    const int g = clamp_grid(tiles_run * 64, G.grid);
    f.prof.begin(st, RR_K_TILES);
    f.tile_ctrs.ensure((size_t)kTileShards * kTileCtrStride);
    const int g_fold = (int)std::min<long>((tiles_run + kWavesPerBlock - 1) / kWavesPerBlock, 2048);
    if (o.region_on) {
        k_tile_order_region<<<1, kOrderThreads, 0, st>>>(fc, s.nodes.ptr, f.tile_cost.ptr, f.tile_order.ptr,
                                                         f.tile_ctrs.ptr, reinterpret_cast<uint32_t*>(f.counters.ptr),
                                                         (int)n_ctr, rt);
        G.kxr<<<g, kBlock, G.dyn, st>>>(fc, sa, f.tile_ctrs.ptr, f.film.ptr, p.srgb_lut.ptr,
                                        reinterpret_cast<uchar4*>(f.rgba8.ptr), tot, f.spill.ptr, tc, sl, rt);
        if (sl.n > 1)
            k_tiles_fold_region<<<g_fold, kBlock, 0, st>>>(fc, s.nodes.ptr, sl, f.film.ptr, p.srgb_lut.ptr,
                                                           reinterpret_cast<uchar4*>(f.rgba8.ptr), rt);
        f.prof.end(st);
        RR_HIP(hipGetLastError());
        return;
    }
    k_tile_order<<<1, kOrderThreads, 0, st>>>(fc, s.nodes.ptr, f.tile_cost.ptr, f.tile_order.ptr, f.tile_ctrs.ptr,
                                              reinterpret_cast<uint32_t*>(f.counters.ptr), (int)n_ctr);
    G.kx<<<g, kBlock, G.dyn, st>>>(fc, sa, f.tile_ctrs.ptr, f.film.ptr, p.srgb_lut.ptr,
                                           reinterpret_cast<uchar4*>(f.rgba8.ptr), tot, f.spill.ptr, tc, sl);
    if (sl.n > 1)
        k_tiles_fold<<<g_fold, kBlock, 0, st>>>(
            fc, s.nodes.ptr, sl, f.film.ptr, p.srgb_lut.ptr, reinterpret_cast<uchar4*>(f.rgba8.ptr));
    f.prof.end(st);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
