// What the two path renderers share: the split trace / shade path of large
// scenes (wavefront.hip) and the LDS-resident tile path (tiles.hip, built
// without SLP vectorisation). Scene views, the camera ray, shade(), the
// tonemap and the host's launch-grid helpers: device and host-inline code
// only, in the anonymous namespace of each of the two translation units.
// Both set `#pragma clang fp contract(off)` before they include this file (and
// the Makefile passes -ffp-contract=off): the arithmetic here relies on it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <type_traits>
#include <utility>

#include "device.hpp"

namespace rr {

struct SceneArgs {
    const BvhNode* nodes;
    const QNode6* qnodes;    // quantised 6-wide hierarchy (split path)
    const TriPack* tris;
    const float* mats;
    const float* lights;
    const float* filter;
    const float* mat_lut;    // kMatLutStride floats per material
    int n_nodes, n_tris, n_mats, n_lights;
    int n_qnodes;            // its node count
};

namespace {

constexpr int kFilterN = 1024;
// Film sum order (every path, and oracle/rr_oracle.c): samples are summed in
// order within groups of kFilmGroup, and the group sums in order into the
// film (sum = 0; per group: sum += group). Frames of <= kFilmGroup samples
// are the plain in-order sum. Groups let k_tiles split a tile's samples
// across waves without changing a bit.
#ifndef RR_FILM_GROUP
#define RR_FILM_GROUP 32
#endif
constexpr int kFilmGroup = RR_FILM_GROUP;
constexpr int kSrgbN = 4096;
constexpr int kLightF = 12;
constexpr int kMatF = 12;
constexpr float kFltMax = 3.402823466e+38f;

// Read-only scene data of the path kernels: in HBM (GlobalView) or, for
// scenes small enough, staged once per block into LDS (LdsView), which turns
// every node / triangle / material / filter fetch of the traversal and shading
// chains into a ds_read (~64-cycle latency instead of an L1/L2 round trip).
template <typename NodeP, typename TriP, typename FloatP>
struct SceneView {
    NodeP nodes;
    TriP tris;
    FloatP mats, lights, filter;
    FloatP lut;  // material tables (kMatLutStride floats per material, build_material_lut)
    lds_f4w* cam = nullptr;  // LDS scenes, camera kernels: 3 float4 per triangle (stage_camera)
    // unit geometric normal + material per triangle: LDS scenes' staged copy
    // (shading kernels), HBM scenes' DevBuild::tnrm (null: none built) — one
    // member for both, so the LDS view passed to k_tiles' out-of-line calls
    // stays the size it was
    typename std::conditional<std::is_same<FloatP, lds_float*>::value, lds_f4w*, const float4*>::type nrm = nullptr;
    lds_f4w* matd = nullptr;  // LDS scenes, shading kernels: each material with its derived terms (kMatDF4)
    lds_f4w* onb = nullptr;   // LDS scenes, shading kernels: make_onb of both sides' normals (kOnbF4 per triangle)
};
// The split path's shading reads each hit triangle's normal and material from
// DevBuild::tnrm (16 B, GlobalView::nrm) instead of its 48 B record and a
// cross product: shading per 02 / 03 / C5 frame slice 11.34 / 11.49 / 9.18 ->
// 10.77 / 10.85 / 8.61 ms (profiles/r5_ab_spec.txt). shade() still takes the
// record where a caller has no such table and passes null.
using GlobalView = SceneView<const BvhNode*, const TriPack*, const float*>;
using LdsView = SceneView<lds_node*, lds_tri*, lds_float*>;

template <typename FloatP>
__device__ __forceinline__ Mat load_mat(FloatP mats, int id) {
    const FloatP m = mats + kMatF * id;
    Mat r;
    r.base = mk3(m[0], m[1], m[2]);
    r.metallic = m[3];
    r.specular = m[4];
    r.roughness = m[5];
    r.ior = m[6];
    r.emission = mk3(m[7], m[8], m[9]);
    r.model = (int)m[10];
    return r;
}

// Material `id` with its derived BSDF terms: LDS-resident scenes stage them
// per material (stage_scene: load_mat + mat_derive once per block, the same
// operations, so the same bits), 4 float4 a shading point reads instead of
// deriving them per sample; scenes in HBM derive at load.
constexpr int kMatDF4 = 4;
//   [0] base.xyz, roughness  [1] emission.xyz, model  [2] alpha, a2, kd0, spec_on  [3] cspec0.xyz, 0
template <typename View>
RR_D Mat view_mat(const View& v, int id) {
    Mat m;
    if constexpr (std::is_same<View, LdsView>::value) {
        const lds_f4w* q = v.matd + kMatDF4 * id;
        const float4 a = lds_ld4(q), b = lds_ld4(q + 1), c = lds_ld4(q + 2), d = lds_ld4(q + 3);
        m.base = xyz(a);
        m.roughness = a.w;
        m.emission = xyz(b);
        m.model = f2i(b.w);
        m.alpha = c.x;
        m.a2 = c.y;
        m.kd0 = c.z;
        m.spec_on = f2i(c.w);
        m.cspec0 = xyz(d);
        m.metallic = m.specular = m.ior = 0.0f;  // used by mat_derive only
    } else {
        m = load_mat(v.mats, id);
        mat_derive(m);
    }
    return m;
}

// Screen rectangle of the scene box (screen_rect), or disabled.
struct ScreenCull {
    bool on = false;
    float r[4];
    RR_D bool outside(float fx, float fy) const {
        return on && (fx < r[0] || fx > r[1] || fy < r[2] || fy > r[3]);
    }
};
// From the root node's two child boxes (global or LDS nodes).
template <typename NodeP>
RR_D ScreenCull screen_cull(const FrameConsts& fc, NodeP nodes) {
    ScreenCull sc;
    if (fc.n_tris <= 0) return sc;
    const BvhNode nd = load_node(nodes, 0);
    const float lo[3] = {fminf(nd.a.x, nd.b.z), fminf(nd.a.y, nd.b.w), fminf(nd.a.z, nd.c.x)};
    const float hi[3] = {fmaxf(nd.a.w, nd.c.y), fmaxf(nd.b.x, nd.c.z), fmaxf(nd.b.y, nd.c.w)};
    sc.on = screen_rect(fc.cam_pos, fc.cam_right, fc.cam_up, fc.cam_back, fc.half_w, fc.half_h, (float)fc.W,
                        (float)fc.H, lo, hi, sc.r);
    return sc;
}

// Camera ray for (pixel, sample): filter-importance-sampled subpixel position,
// pinhole through the sensor plane at unit distance, z-depth clipping.
// culled (optional): set when the ray's subpixel position is outside the
// scene's screen rectangle (the ray misses everything).
template <typename FloatP>
__device__ __forceinline__ void camera_ray_xy(const FrameConsts& fc, FloatP filt, int px, int py,
                                              uint32_t key, float3& o, float3& d, float& tmin, float& tmax,
                                              const ScreenCull* cull = nullptr, bool* culled = nullptr) {
    // the subpixel pair: the 16-bit halves of the path key itself (a hash
    // output, so no hash of its own; the other dimensions hash key + offset);
    // both < 1: the filter table is read without its range branches
    const float ux = (float)(key >> 16) * 1.52587890625e-05f, uy = (float)(key & 0xffffu) * 1.52587890625e-05f;
    const float fx = (float)px + 0.5f + table_lerp_padded(filt, kFilterN, ux);
    const float fy = (float)py + 0.5f + table_lerp_padded(filt, kFilterN, uy);
    if (cull) {
        *culled = cull->outside(fx, fy);
        if (*culled) {  // a miss: no direction needed (shade() of a miss reads only T and the world)
            o = fc.cam_pos;
            d = mk3(0.0f, 0.0f, 1.0f);
            tmin = 0.0f;
            tmax = -1.0f;
            return;
        }
    }
    const float sx = fmaf(fx, fc.inv_w2, -1.0f) * fc.half_w;
    const float sy = fmaf(-fy, fc.inv_h2, 1.0f) * fc.half_h;
    const float len = sqrt_rn(fmaf(sy, sy, fmaf(sx, sx, 1.0f)));  // >= 1
    const float3 dw = mk3(fmaf(fc.cam_up.x, sy, fmaf(fc.cam_right.x, sx, -fc.cam_back.x)),
                          fmaf(fc.cam_up.y, sy, fmaf(fc.cam_right.y, sx, -fc.cam_back.y)),
                          fmaf(fc.cam_up.z, sy, fmaf(fc.cam_right.z, sx, -fc.cam_back.z)));
    const float il = rcp_rn(len);  // len in [1, 2^60]: the camera's half extents are finite
    d = scl3(dw, il);
    o = fc.cam_pos;
    tmin = fc.clip_start * len;
    tmax = fc.clip_end * len;
}

// Staged material word of LDS-resident scenes: material id | hull_flags << kHullShift.
constexpr int kHullShift = 30;
constexpr int kOnbF4 = 4;  // staged shading frames per triangle (stage_scene)

struct ShadeOut {
    bool cont, shadow;
    bool esc;                // the rays leave a hull side of the hit triangle (hull_flags): they meet nothing
    float3 o, d, T;          // continuation ray + throughput
    uint32_t lob;            // continuation's lobe bounce counters (lobe_counts)
    float3 so, sd, sc;       // shadow ray + pending contribution
    float sdist;
};

// Per-lobe bounce counters of a path (Cycles path state diffuse_bounce /
// glossy_bounce, intern/cycles/kernel/integrator/path_state.h path_state_next),
// packed: diffuse scatters in bits 0..15, glossy scatters in bits 16..31.
constexpr uint32_t kGlossyOne = 0x10000u;
// Whether the path ends at this hit (emission only, no NEE, no scatter): the
// scatter that brought it here advanced a counter to its cap. Cycles marks the
// path PATH_RAY_TERMINATE_AFTER_TRANSPARENT when bounce >= max_bounce,
// diffuse_bounce >= max_diffuse_bounce or glossy_bounce >= max_glossy_bounce
// after the increment; the caps here are >= 1 (setup_frame), so a cap of 0
// ("direct light only") behaves as Cycles': the camera hit still scatters once.
template <typename FC>
RR_D bool path_capped(const FC& fc, int bounce, uint32_t lob) {
    return bounce >= fc.max_bounces || (int)(lob & 0xffffu) >= fc.max_diffuse || (int)(lob >> 16) >= fc.max_glossy;
}

RR_D void add_to(float3& L, float3 c) {
    L.x = L.x + c.x;
    L.y = L.y + c.y;
    L.z = L.z + c.z;
}

// Shadow rays of shade(): handed back in ShadeOut (queue kernels) ...
struct EmitShadow {
    static constexpr bool kInline = false;
    RR_D bool operator()(float3, float3, float) const { return false; }
};

// K9: shade one path at `bounce` given its closest hit; L updated in place.
// With an inline shadow tracer (Shadow::kInline: a functor returning whether
// the ray (origin, direction, distance) is occluded) the NEE ray is traced as
// soon as it exists and its contribution added, before the continuation is
// sampled: the same radiance additions in the same order as emitting it
// (emission, then NEE, then the next bounce), with the shadow-ray state dead
// before the continuation's registers are needed. out.shadow still reports
// that a shadow ray was traced.
// ... and the continuation: handed back in ShadeOut (out.o / d / T / lob), or,
// with an in-place handler (Cont::kInline: called as on_cont(origin,
// direction, throughput, lobe counters, leaves a hull side, L)), taken over at
// the point it is sampled, so that its ray is never held past shade() (k_tiles:
// held to the sample loop's join, the compiler spilled it to scratch in every
// sample, most of that kernel's HBM write traffic).
struct EmitCont {
    static constexpr bool kInline = false;
    RR_D void operator()(float3, float3, float3, uint32_t, bool, float3&) const {}
};

// Lights behind the hit's surface: shade_covered(), the
// shading of k_tiles' tiles that one triangle covers, asks light_behind
// (rr_device.h) before it draws a point on a point / disk light, and where
// that holds skips the draw and the cosN test it could only fail: nothing
// added, out.shadow false, as without the rule. shade() does not ask: with
// the rule in its LdsView instantiation as well (k_tiles' general body and
// tiles_continue) the whole-tile kernel ran slower than without any rule
// (measured, code removed: profiles/light_facing.md).
#ifndef RR_LIGHT_FACING
#define RR_LIGHT_FACING 1  // 0: the rule compiled out (tiles.hip as before it: the reference of tests and A/B runs)
#endif

// FC: FrameConsts or ShadeConsts (the fields shade() reads: world,
// clamp_indirect, the bounce caps, n_lights).
template <typename View, typename Shadow = EmitShadow, typename FC = FrameConsts, typename Cont = EmitCont>
__device__ __forceinline__ void shade(const FC& fc, int bounce, const View& v, float3 o, float3 d,
                                      float3 T, uint32_t lob, const Hit& h, uint32_t key, float3& L, ShadeOut& out,
                                      const Shadow& trace_shadow = Shadow{}, const Cont& on_cont = Cont{}) {
    out.cont = false;
    out.shadow = false;
    out.esc = false;
    if (h.idx < 0) {
        float3 c = mul3(T, fc.world);
        if (bounce > 0) c = clamp_contrib(c, fc.clamp_indirect);
        add_to(L, c);
        return;
    }
    int mid;
    float3 N;
    uint32_t hull = 0;  // hull_flags of the hit triangle (LDS-resident scenes)
    if constexpr (std::is_same<View, LdsView>::value) {
        const float4 nm = lds_ld4(v.nrm + h.idx);  // staged: norm3(cross3(e1, e2)), material id | hull flags
        N = xyz(nm);
        mid = f2i(nm.w) & ((1 << kHullShift) - 1);
        hull = (uint32_t)f2i(nm.w) >> kHullShift;
        // an LDS-resident scene holds a handful of materials (scene_lds_f4): the
        // table offsets become 24-bit multiplies (full rate) instead of
        // v_mul_lo_u32 / v_mad_u64_u32
        __builtin_assume(mid >= 0 && mid < 4096);
    } else if (v.nrm) {
        const float4 nm = v.nrm[h.idx];  // k_tri_nrm: the same normal, precomputed
        N = xyz(nm);
        mid = f2i(nm.w);
    } else {
        const TriPack tp = load_tri(v.tris, h.idx);
        mid = f2i(tp.p1.w);
        N = norm3(cross3(sub3(xyz(tp.p1), xyz(tp.p0)), sub3(xyz(tp.p2), xyz(tp.p0))));
    }
    const Mat m = view_mat(v, mid);
    const auto lut = v.lut + kMatLutStride * mid;
    const float t = h.t;
    const float3 P = madd3(o, d, t);
    const bool flip = dot3(N, d) > 0.0f;
    if (flip) N = mk3(-N.x, -N.y, -N.z);
    // shadow and continuation rays leave on N's side: the front side unless flipped
    const bool esc = ((hull >> (flip ? 1 : 0)) & 1u) != 0u;
    out.esc = esc;
    const float3 wo = mk3(-d.x, -d.y, -d.z);
    if (m.emission.x != 0.0f || m.emission.y != 0.0f || m.emission.z != 0.0f) {
        float3 c = mul3(T, m.emission);
        if (bounce > 0) c = clamp_contrib(c, fc.clamp_indirect);
        add_to(L, c);
    }
    if (path_capped(fc, bounce, lob)) return;
    const BsdfView vw = bsdf_view(m, lut, N, wo);
    const uint32_t dim0 = 2u + (uint32_t)(kDimsPerBounce * bounce);
    // dimension pairs of this bounce (rng2): (light pick, lobe choice) at
    // dim0, the disk point at dim0 + 1, the BSDF direction at dim0 + 4;
    // Russian roulette keeps dim0 + 6 (oracle/rr_oracle.c radiance)
    float u_light, u_lobe;
    rng2(key, dim0, u_light, u_lobe);
    const float3 Po = offset_ray(P, N);
    // next-event estimation toward one uniformly chosen light
    if (fc.n_lights > 0) {
        int li = (int)(u_light * (float)fc.n_lights);
        if (li > fc.n_lights - 1) li = fc.n_lights - 1;
        __builtin_assume(li >= 0 && li < kMaxLights);  // rng >= 0, n_lights <= kMaxLights (setup_frame)
        const auto lt = v.lights + kLightF * li;
        float3 wi, Li;  // Li: radiance x cos_light / pdf (solid angle), i.e. I*cos/d^2
        float dist;
        if (lt[0] == 0.0f) {  // point / disk light
            const float3 lp = mk3(lt[1], lt[2], lt[3]);
            const float radius = lt[7];
            const float3 I = mk3(lt[8], lt[9], lt[10]);
            const float3 tl = sub3(lp, P);
            const float dl2 = dot3(tl, tl);
            if (radius > 0.0f) {
                float sl, rl;
                sqrt_rcp_any(dl2, sl, rl);
                const float3 wl = scl3(tl, rl);
                float3 b1, b2;
                make_onb(wl, b1, b2);
                float dx, dy;
                float u1, u2;
                rng2(key, dim0 + 1u, u1, u2);
                concentric_disk(u1, u2, dx, dy);
                dx = dx * radius;
                dy = dy * radius;
                const float3 sp = madd3(madd3(lp, b1, dx), b2, dy);
                const float3 ts = sub3(sp, P);
                const float ds2 = dot3(ts, ts);
                float id;
                sqrt_rcp_any(ds2, dist, id);
                wi = scl3(ts, id);
                const float cl = fabsf(dot3(wl, wi));
                Li = scl3(I, cl * id * id);
            } else {
                float id;
                sqrt_rcp_any(dl2, dist, id);
                wi = scl3(tl, id);
                Li = scl3(I, 1.0f / dl2);
            }
        } else {  // sun: delta direction, irradiance
            wi = mk3(-lt[4], -lt[5], -lt[6]);
            dist = kFltMax;
            Li = mk3(lt[8], lt[9], lt[10]);
        }
        const float cosN = dot3(N, wi);
        if (cosN > 0.0f) {
            float pdf;
            const float3 f = bsdf_eval_v(m, lut, vw, N, wo, wi, pdf);  // f * cosN
            const float k = (float)fc.n_lights;
            float3 c = mk3(T.x * f.x * k * Li.x, T.y * f.y * k * Li.y, T.z * f.z * k * Li.z);
            if (bounce > 0) c = clamp_contrib(c, fc.clamp_indirect);
            if (max3f(c) > 0.0f) {
                out.shadow = true;
                if constexpr (Shadow::kInline) {
                    if (esc || !trace_shadow(Po, wi, dist)) add_to(L, c);
                } else {
                    out.so = Po;
                    out.sd = wi;
                    out.sdist = dist;
                    out.sc = c;
                }
            }
        }
    }
    // continue the path
    float3 wi, f;
    float pdf;
    bool glossy;
    float u_b1, u_b2;
    rng2(key, dim0 + 4u, u_b1, u_b2);
    bool sampled;
    if constexpr (std::is_same<View, LdsView>::value) {  // the staged frame of the hit side
        const lds_f4w* fr = v.onb + kOnbF4 * h.idx + (flip ? 2 : 0);
        const float4 tb = lds_ld4(fr), bb = lds_ld4(fr + 1);
        sampled = bsdf_sample_onb(m, lut, vw, N, xyz(tb), mk3(tb.w, bb.x, bb.y), wo, u_lobe, u_b1, u_b2, wi, f, pdf,
                                  glossy);
    } else {
        sampled = bsdf_sample(m, lut, vw, N, wo, u_lobe, u_b1, u_b2, wi, f, pdf, glossy);
    }
    if (!sampled) return;
    const float k = 1.0f / pdf;  // f = f * cosL already
    T = mk3(T.x * f.x * k, T.y * f.y * k, T.z * f.z * k);
    if (!(max3f(T) > 0.0f)) return;
    if (bounce >= kRrStartBounce) {
        const float q = fminf(max3f(T), 1.0f);
        if (rng(key, dim0 + 6u) >= q) return;
        const float iq = 1.0f / q;
        T = mk3(T.x * iq, T.y * iq, T.z * iq);
    }
    out.cont = true;
    if constexpr (Cont::kInline) {
        on_cont(Po, wi, T, lob + (glossy ? kGlossyOne : 1u), esc, L);
        return;
    }
    out.o = Po;
    out.d = wi;
    out.T = T;
    out.lob = lob + (glossy ? kGlossyOne : 1u);
}

// shade() for k_tiles' tiles that one triangle covers (tiles.hip tile_mask,
// DESIGN.md §4): every lane of the wave shades the same triangle `tri` of an
// LDS-resident scene, seen from the same side (`flip`: from behind, what
// shade() takes from the sign of dot(N, d)), and the scene has at most one
// light (the caller checks fc.n_lights <= 1). What shade() fetches by the
// lane's own h.idx and light pick — the staged normal and material word, the
// derived material, the table base, the shading frame, the light's record —
// is read here at wave-uniform addresses, the side, the emission test and the
// light's kind become wave-uniform branches, and the pick, the flip's selects
// and the per-lane hull bit are gone. `hit`: this lane's ray met the triangle
// inside its clip range; else the miss term, as shade() for h.idx < 0. Of h
// only h.t is read. Every float operation on what varies per lane is
// shade()'s, in shade()'s order, so the radiance has the same bits; shade()
// itself is left as it is so that the kernels that call it compile to the
// same instructions. A change of shade() is to be made here as well
// (tests/test_gpu_tile_covered.py compares the two bit for bit).
//
// Held: where the unit's values live. CoveredInLoop: read from LDS at the
// uniform addresses in every sample (kept, RR_TILES_COVERED=1). CoveredHeld:
// read once per work unit by the caller into wave-uniform registers
// (RR_TILES_COVERED=2; measured, not kept: profiles/tile_covered.md).
struct CoveredInLoop {
    static constexpr bool kHeld = false;
};
struct CoveredHeld {
    static constexpr bool kHeld = true;
    float3 N;        // the side seen (flipped already)
    int mid;
    bool esc;        // that side is a hull side
    Mat m;
    float3 tb, bb;   // the staged frame of that side
    float lt[11];    // the light's record (n_lights == 1)
};
template <typename Shadow, typename FC, typename Cont, typename Held = CoveredInLoop>
__device__ __forceinline__ void shade_covered(const FC& fc, int bounce, const LdsView& v, int tri, bool flip, bool hit,
                                              float3 o, float3 d, float3 T, uint32_t lob, const Hit& h, uint32_t key,
                                              float3& L, ShadeOut& out, const Shadow& trace_shadow,
                                              const Cont& on_cont, const Held& held = Held{}) {
    static_assert(Shadow::kInline, "the shadow ray is traced in place");
    out.cont = false;
    out.shadow = false;
    out.esc = false;
    if (!hit) {
        float3 c = mul3(T, fc.world);
        if (bounce > 0) c = clamp_contrib(c, fc.clamp_indirect);
        add_to(L, c);
        return;
    }
    float3 N;
    int mid;
    bool esc;
    Mat m;
    if constexpr (Held::kHeld) {
        N = held.N;
        mid = held.mid;
        esc = held.esc;
        m = held.m;
    } else {
        const float4 nm = lds_ld4(v.nrm + tri);  // staged: norm3(cross3(e1, e2)), material id | hull flags
        N = xyz(nm);
        mid = f2i(nm.w) & ((1 << kHullShift) - 1);
        const uint32_t hull = (uint32_t)f2i(nm.w) >> kHullShift;
        m = view_mat(v, mid);
        if (flip) N = mk3(-N.x, -N.y, -N.z);
        esc = ((hull >> (flip ? 1 : 0)) & 1u) != 0u;
    }
    __builtin_assume(mid >= 0 && mid < 4096);
    const auto lut = v.lut + kMatLutStride * mid;
    const float t = h.t;
    const float3 P = madd3(o, d, t);
    out.esc = esc;
    const float3 wo = mk3(-d.x, -d.y, -d.z);
    if (m.emission.x != 0.0f || m.emission.y != 0.0f || m.emission.z != 0.0f) {
        float3 c = mul3(T, m.emission);
        if (bounce > 0) c = clamp_contrib(c, fc.clamp_indirect);
        add_to(L, c);
    }
    if (path_capped(fc, bounce, lob)) return;
    const BsdfView vw = bsdf_view(m, lut, N, wo);
    const uint32_t dim0 = 2u + (uint32_t)(kDimsPerBounce * bounce);
    float u_light, u_lobe;
    rng2(key, dim0, u_light, u_lobe);
    const float3 Po = offset_ray(P, N);
    if (fc.n_lights > 0) {  // the one light: every u_light picks it
        const auto lt = [&](int k) {
            if constexpr (Held::kHeld) return held.lt[k];
            else return v.lights[k];
        };
        float3 wi, Li;
        float dist;
        bool away = false;  // the light lies behind the side seen: nothing to draw
        if (lt(0) == 0.0f) {  // point / disk light
            const float3 lp = mk3(lt(1), lt(2), lt(3));
            const float radius = lt(7);
            if constexpr (RR_LIGHT_FACING != 0) away = light_behind(N, P, lp, radius);
            if (!away) {
                const float3 I = mk3(lt(8), lt(9), lt(10));
                const float3 tl = sub3(lp, P);
                const float dl2 = dot3(tl, tl);
                if (radius > 0.0f) {
                    float sl, rl;
                    sqrt_rcp_any(dl2, sl, rl);
                    const float3 wl = scl3(tl, rl);
                    float3 b1, b2;
                    make_onb(wl, b1, b2);
                    float dx, dy;
                    float u1, u2;
                    rng2(key, dim0 + 1u, u1, u2);
                    concentric_disk(u1, u2, dx, dy);
                    dx = dx * radius;
                    dy = dy * radius;
                    const float3 sp = madd3(madd3(lp, b1, dx), b2, dy);
                    const float3 ts = sub3(sp, P);
                    const float ds2 = dot3(ts, ts);
                    float id;
                    sqrt_rcp_any(ds2, dist, id);
                    wi = scl3(ts, id);
                    const float cl = fabsf(dot3(wl, wi));
                    Li = scl3(I, cl * id * id);
                } else {
                    float id;
                    sqrt_rcp_any(dl2, dist, id);
                    wi = scl3(tl, id);
                    Li = scl3(I, 1.0f / dl2);
                }
            }
        } else {  // sun: delta direction, irradiance
            wi = mk3(-lt(4), -lt(5), -lt(6));
            dist = kFltMax;
            Li = mk3(lt(8), lt(9), lt(10));
        }
        if (!away) {  // else every cosN the branch could compute is <= 0 (light_behind)
            const float cosN = dot3(N, wi);
            if (cosN > 0.0f) {
                float pdf;
                const float3 f = bsdf_eval_v(m, lut, vw, N, wo, wi, pdf);  // f * cosN
                const float k = (float)fc.n_lights;
                float3 c = mk3(T.x * f.x * k * Li.x, T.y * f.y * k * Li.y, T.z * f.z * k * Li.z);
                if (bounce > 0) c = clamp_contrib(c, fc.clamp_indirect);
                if (max3f(c) > 0.0f) {
                    out.shadow = true;
                    if (esc || !trace_shadow(Po, wi, dist)) add_to(L, c);
                }
            }
        }
    }
    // continue the path
    float3 wi, f;
    float pdf;
    bool glossy;
    float u_b1, u_b2;
    rng2(key, dim0 + 4u, u_b1, u_b2);
    float3 ft, fb;  // the staged frame of the side seen
    if constexpr (Held::kHeld) {
        ft = held.tb;
        fb = held.bb;
    } else {
        const lds_f4w* fr = v.onb + kOnbF4 * tri + (flip ? 2 : 0);
        const float4 tb = lds_ld4(fr), bb = lds_ld4(fr + 1);
        ft = xyz(tb);
        fb = mk3(tb.w, bb.x, bb.y);
    }
    if (!bsdf_sample_onb(m, lut, vw, N, ft, fb, wo, u_lobe, u_b1, u_b2, wi, f, pdf, glossy))
        return;
    const float k = 1.0f / pdf;  // f = f * cosL already
    T = mk3(T.x * f.x * k, T.y * f.y * k, T.z * f.z * k);
    if (!(max3f(T) > 0.0f)) return;
    if (bounce >= kRrStartBounce) {
        const float q = fminf(max3f(T), 1.0f);
        if (rng(key, dim0 + 6u) >= q) return;
        const float iq = 1.0f / q;
        T = mk3(T.x * iq, T.y * iq, T.z * iq);
    }
    out.cont = true;
    if constexpr (Cont::kInline) {
        on_cont(Po, wi, T, lob + (glossy ? kGlossyOne : 1u), esc, L);
        return;
    }
    out.o = Po;
    out.d = wi;
    out.T = T;
    out.lob = lob + (glossy ? kGlossyOne : 1u);
}

constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kMaxBlocksPerCu = 8;  // grid cap per CU

// Traversal-count reduction (RR_FLAG_COUNT_TRAVERSAL only).
__device__ __forceinline__ void flush_counts(unsigned long long* __restrict__ tc, int slot, uint32_t nv,
                                             uint32_t nt) {
    unsigned long long a = nv, b = nt;
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tc[slot], a);
        atomicAdd(&tc[slot + 1], b);
    }
}

RR_D void set_miss(Hit& h, float tmax) {
    h.t = tmax;
    h.u = h.v = 0.0f;
    h.idx = -1;
    h.orig = -1;
}

// K12: mean -> exposure -> view transform -> 8-bit.
RR_D uchar4 tonemap(const FrameConsts& fc, float4 acc, const float* __restrict__ srgb) {
    float c[3] = {acc.x * fc.inv_spp * fc.exposure_scale, acc.y * fc.inv_spp * fc.exposure_scale,
                  acc.z * fc.inv_spp * fc.exposure_scale};
    uint8_t q[3];
    for (int k = 0; k < 3; ++k) {
        float v = fminf(fmaxf(c[k], 0.0f), 1.0f);
        if (fc.view_transform == 0) v = srgb_oetf(v, srgb, kSrgbN);
        q[k] = quantize8(v);
    }
    return make_uchar4(q[0], q[1], q[2], 255);
}

// Persistent grid = resident blocks: CUs x blocks per CU the kernel's register
// and LDS budget admits (a grid-stride loop over more blocks than fit would
// only queue the surplus behind the first wave of blocks).
template <typename K>
int resident_grid(K kernel, size_t dyn_lds = 0, int block = kBlock) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, dyn_lds) != hipSuccess || per_cu <= 0)
        per_cu = std::max(1, 1024 / block);
    return device_cu_count() * std::min(per_cu, kMaxBlocksPerCu * kBlock / block);
}
// Resident grid per (kernel, dynamic LDS bytes), cached.
template <typename K>
int grid_for(K kernel, size_t dyn_lds, int block = kBlock) {
    static std::map<std::pair<const void*, size_t>, int> cache;
    const auto key = std::make_pair(reinterpret_cast<const void*>(kernel), dyn_lds);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    return cache[key] = resident_grid(kernel, dyn_lds, block);
}
inline int clamp_grid(long work, int resident, int block = kBlock) {
    const long g = (work + block - 1) / block;
    return (int)std::max<long>(1, std::min<long>(g, resident));
}

}  // namespace
}  // namespace rr
