// Reservoir resampling as ReSTIR DI (restir_di.hip) and ReSTIR GI (restir_gi.hip) share it: the code of restir_di.h's rule sections
// `reprojection`, `reuse`, `temporal`, `neighbours`, `spatial` and `jacobian` (the rule text stays there; restir_gi.h says what GI changes),
// written once over a sample kind, and the host skeleton of the two stage files.
//
// A kind (RestirDiKind, restir_di.h; RestirGiKind, restir_gi.h) is a struct of static TR_DEV functions that carries what differs:
//   Sample, State = RestirState<Sample>, Reservoir   the sample, the reservoir in registers and its record in memory
//   Eval                                  what a contribution returns besides its value: dir, dist2 (the shadow ray) and what the Jacobian needs
//   create(), load(src), store(dst, r)    the null reservoir; a record read (weight_sum = 0) and written
//   confidence(src)                       the confidence of a stored reservoir alone (one word)
//   is_null(sample)
//   contribution(sv, sample, dom, eval)   the unshadowed contribution of a sample at a surface
//   jacobian(sample, eval, from, at)      reconnection_jacobian of a sample evaluated at `at` (eval) that was found at `from`
//   SURFACE_LATE                          where the spatial merge reads a neighbour's whole surface record: behind the first traversal or ahead of it
// The device half keeps the order of fp operations and of random draws of restir_di.h; a stage's kernels keep their own parts (DI: the
// candidate loop, the miss colour, the emission; GI: the secondary ray, the initial sample's update, `in` plus the indirect light).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "shading.h"
#include "trace.h"
#include "first_hit.h"
#include "stage_host.h"
#include "pt.h"

namespace tr {

constexpr int RESTIR_MAX_SPATIAL = 4;

struct alignas(16) RestirSurface {       // trhip_restir_di_surface
    f3 pos; int instance_id;
    f3 mapped_normal; float metallic;
    f3 flat_normal; float roughness;
    f3 view; float transmittance;
    f4 albedo;
    f3 emission; float f0;
    float ior_in, ior_out, pad0, pad1;
};
struct RestirTemporalRecord {            // trhip_restir_di_temporal
    int px, py; uint reuse; float prev_confidence;
    float target, weight, draw; uint selected;
};
struct RestirSpatialRecord {             // trhip_restir_di_spatial
    int px, py; uint good, selected;     // px = -1: an empty slot
    float target_n, visibility_n, jacobian_n, m;
    float wi, draw, target_c, visibility_c;
    float jacobian_c, mis_canonical, pad0, pad1;
};
struct RestirFinalRecord {               // trhip_restir_di_final
    f3 contribution; float visibility;   // the unshadowed contribution of the chosen sample
    float canonical_m, wi, draw; uint selected;
};
static_assert(sizeof(RestirSurface) == 112 && sizeof(RestirTemporalRecord) == 32 && sizeof(RestirSpatialRecord) == 64 && sizeof(RestirFinalRecord) == 32, "layout");

// Word i of a record: the buffers are device allocations and every record is 16-byte aligned - one global (not flat) 16-byte load or store
TR_HD u4 restir_word(const void* p, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint v4u __attribute__((ext_vector_type(4)));
    const v4u v = ((const v4u __attribute__((address_space(1)))*)p)[i];
    return u4{v.x, v.y, v.z, v.w};
#else
    return ((const u4*)p)[i];
#endif
}
TR_HD void restir_set_word(void* p, int i, u4 w) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint v4u __attribute__((ext_vector_type(4)));
    ((v4u __attribute__((address_space(1)))*)p)[i] = v4u{w.x, w.y, w.z, w.w};
#else
    ((u4*)p)[i] = w;
#endif
}
#define TR_U(x) __float_as_uint(x)       // for the record writers here and in the stage files

template <class Sample>
struct RestirState {                     // `reservoir` (restir_di.glsl:29-37) without its contribution
    Sample s;
    float target_function, weight_sum, uc_weight, confidence;
};
template <class Sample>
TR_DEV bool restir_update(RestirState<Sample>& r, const Sample& s, float weight, float u) {    // update_reservoir (restir_di.glsl:118-131)
    r.weight_sum = r.weight_sum + weight;
    if (u * r.weight_sum < weight) { r.s = s; return true; }
    return false;
}
template <class Sample>
TR_DEV float restir_uc_weight(const RestirState<Sample>& r) { return r.weight_sum > 0.0f ? r.weight_sum / r.target_function : 0.0f; }

// The part of a surface record light_contribution reads (the shader's `domain`)
struct RestirDomain {
    f3 pos, mapped_normal, flat_normal, view;
    SampledMaterial mat;
};
TR_DEV void restir_store_surface(RestirSurface* dst, const RestirDomain& d, int instance_id) {
    restir_set_word(dst, 0, u4{TR_U(d.pos.x), TR_U(d.pos.y), TR_U(d.pos.z), (uint)instance_id});
    restir_set_word(dst, 1, u4{TR_U(d.mapped_normal.x), TR_U(d.mapped_normal.y), TR_U(d.mapped_normal.z), TR_U(d.mat.metallic)});
    restir_set_word(dst, 2, u4{TR_U(d.flat_normal.x), TR_U(d.flat_normal.y), TR_U(d.flat_normal.z), TR_U(d.mat.roughness)});
    restir_set_word(dst, 3, u4{TR_U(d.view.x), TR_U(d.view.y), TR_U(d.view.z), TR_U(d.mat.transmittance)});
    restir_set_word(dst, 4, u4{TR_U(d.mat.albedo.x), TR_U(d.mat.albedo.y), TR_U(d.mat.albedo.z), TR_U(d.mat.albedo.w)});
    restir_set_word(dst, 5, u4{TR_U(d.mat.emission.x), TR_U(d.mat.emission.y), TR_U(d.mat.emission.z), TR_U(d.mat.f0)});
    restir_set_word(dst, 6, u4{TR_U(d.mat.ior_in), TR_U(d.mat.ior_out), 0u, 0u});
}
// Position, instance id and flat normal alone: what the neighbour search reads (two words)
TR_DEV void restir_load_surface_head(const RestirSurface* src, f3& pos, int& instance_id, f3& flat_normal) {
    const u4 a = restir_word(src, 0), c = restir_word(src, 2);
    pos = F3(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)); instance_id = (int)a.w;
    flat_normal = F3(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z));
}
TR_DEV int restir_load_surface(const RestirSurface* src, RestirDomain& d) {
    const u4 a = restir_word(src, 0), b = restir_word(src, 1), c = restir_word(src, 2), e = restir_word(src, 3), f = restir_word(src, 4), g = restir_word(src, 5),
             h = restir_word(src, 6);
#define TR_F(x) __uint_as_float(x)
    d.pos = F3(TR_F(a.x), TR_F(a.y), TR_F(a.z));
    d.mapped_normal = F3(TR_F(b.x), TR_F(b.y), TR_F(b.z)); d.mat.metallic = TR_F(b.w);
    d.flat_normal = F3(TR_F(c.x), TR_F(c.y), TR_F(c.z)); d.mat.roughness = TR_F(c.w);
    d.view = F3(TR_F(e.x), TR_F(e.y), TR_F(e.z)); d.mat.transmittance = TR_F(e.w);
    d.mat.albedo = F4(TR_F(f.x), TR_F(f.y), TR_F(f.z), TR_F(f.w));
    d.mat.emission = F3(TR_F(g.x), TR_F(g.y), TR_F(g.z)); d.mat.f0 = TR_F(g.w);
    d.mat.ior_in = TR_F(h.x); d.mat.ior_out = TR_F(h.y);
#undef TR_F
    return (int)a.w;
}

TR_DEV bool restir_casts(f3 c) { return c.x > 0.0f || c.y > 0.0f || c.z > 0.0f; }

// The shadow ray of a contribution (`visibility` of restir_di.h)
template <bool TWO_LEVEL>
TR_DEV float restir_shadow(const SceneView& sv, float min_ray_dist, f3 pos, f3 contribution, f3 dir, float dist2, int* stack, int& overflow) {
    float visibility = 0.0f;
    if (restir_casts(contribution)) {
        TraceStats st = {};
        visibility = trace_shadow4<false, TWO_LEVEL>(sv, pos, dir, min_ray_dist, sqrtf(dist2) - min_ray_dist, stack, st, overflow);
    }
    return visibility;
}

// The visibility of a target function that traces nothing (`visibility modes` of restir_di.h): 1 where restir_shadow would cast a ray
TR_DEV float restir_untraced(f3 contribution) { return restir_casts(contribution) ? 1.0f : 0.0f; }

// reconnection_jacobian, mis_canonical, mis_noncanonical (restir_di.glsl:477-533)
TR_DEV float restir_jacobian(f3 prev_src, f3 cur_src, f3 dst, f3 n) {
    const f3 qdelta = prev_src - dst, rdelta = cur_src - dst;
    const float lq = length(qdelta), lr = length(rdelta);
    const float theta_q = fabsf(dot(n, qdelta)), theta_r = fabsf(dot(n, rdelta));
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return 1.0f;
    float v = (theta_r * (lq * lq * lq)) / (theta_q * (lr * lr * lr));
    if (isinf(v) || isnan(v)) v = 0.0f;
    return v;
}
TR_DEV float restir_mis_canonical(float c_conf, float o_conf, float total, float c_target, float c_in_other, float jacobian) {
    if (c_target == 0.0f) return 0.0f;
    const float w = c_conf * c_target;
    return ((o_conf / total) * w) / (w + ((total - c_conf) * c_in_other) * jacobian);
}
TR_DEV float restir_mis_noncanonical(float c_conf, float o_conf, float total, float o_target, float o_in_canonical, float jacobian) {
    if (o_target == 0.0f) return 0.0f;
    const float w = (total - c_conf) * o_target;
    return ((o_conf / total) * w) / (w + (c_conf * o_in_canonical) * jacobian);
}

// `reprojection` and `reuse`: get_reprojected_pixel's stochastic rounding (one draw) and temporal_edge_detection (restir_di.glsl:138-153,
// 375-388).  motion: the reprojected position before the rounding; origin_dist: length(ray origin - pos).  prev_surfaces, histories: the
// pixel's layer.
struct RestirReprojection { int rx = -1, ry = -1; bool reuse = false; float prev_confidence = 0.0f; };      // as it is without temporal reuse
template <class Kind>
TR_DEV RestirReprojection restir_reproject(const LaunchCtx& L, int has_history, const RestirSurface* prev_surfaces, const typename Kind::Reservoir* histories,
                                           const RestirDomain& dom, f2 motion, float origin_dist, LocalSampler& ls) {
    RestirReprojection rp;
    const int ix = (int)motion.x, iy = (int)motion.y;
    const f2 off = F2(motion.x - (float)ix, motion.y - (float)iy);
    const f4 rs = u4_to_unit(pcg4d(ls.rs));
    rp.rx = ix + (off.x < rs.x ? 0 : 1); rp.ry = iy + (off.y < rs.y ? 0 : 1);
    if (has_history && (uint)rp.rx < L.launch_w && (uint)rp.ry < L.launch_h) {
        f3 ppos, pflat;
        int pid;
        const RestirSurface* prev = prev_surfaces + (size_t)rp.ry * L.launch_w + (uint)rp.rx;
        restir_load_surface_head(prev, ppos, pid, pflat);
        const u4 w1 = restir_word(prev, 1);
        const f3 prev_normal = F3(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z));
        const float delta_pos = length(dom.pos - ppos);
        const float max_range = 0.01f * origin_dist / (fabsf(dot(dom.view, dom.mapped_normal)) + 0.001f);
        rp.reuse = !(dot(prev_normal, dom.mapped_normal) < 0.95f || delta_pos > max_range);
    }
    if (rp.reuse) rp.prev_confidence = Kind::confidence(histories + (size_t)rp.ry * L.launch_w + (uint)rp.rx);
    return rp;
}

// `temporal`: the merge of the history reservoir restir_reproject chose (one draw with reuse) and the clamp of the confidence
template <class Kind>
TR_DEV void restir_temporal_merge(const SceneView& sv, const LaunchCtx& L, const RestirReprojection& rp, const typename Kind::Reservoir* histories,
                                  const RestirDomain& dom, float max_confidence, LocalSampler& ls, typename Kind::State& r, RestirTemporalRecord& trec) {
    trec.px = rp.rx; trec.py = rp.ry; trec.reuse = rp.reuse ? 1u : 0u; trec.prev_confidence = rp.prev_confidence;
    if (rp.reuse) {
        const typename Kind::State prev_r = Kind::load(histories + (size_t)rp.ry * L.launch_w + (uint)rp.rx);
        typename Kind::Eval e;
        const float target = rgb_to_luminance(Kind::contribution(sv, prev_r.s, dom, e));
        float weight = ((prev_r.confidence / (r.confidence + prev_r.confidence)) * target) * prev_r.uc_weight;
        if (isnan(weight)) weight = 0.0f;
        const float u = u4_to_unit(pcg4d(ls.rs)).x;
        const bool selected = restir_update(r, prev_r.s, weight, u);
        if (selected) r.target_function = target;
        r.confidence = r.confidence + prev_r.confidence;
        r.uc_weight = restir_uc_weight(r);
        trec.target = target; trec.weight = weight; trec.draw = u; trec.selected = selected ? 1u : 0u;
    }
    r.confidence = fmin2(r.confidence, max_confidence);
}
TR_DEV RestirTemporalRecord restir_no_temporal() { return {-1, -1, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0u}; }
TR_DEV void restir_write_temporal(RestirTemporalRecord* dst, const RestirTemporalRecord& trec) {
    restir_set_word(dst, 0, u4{(uint)trec.px, (uint)trec.py, trec.reuse, TR_U(trec.prev_confidence)});
    restir_set_word(dst, 1, u4{TR_U(trec.target), TR_U(trec.weight), TR_U(trec.draw), trec.selected});
}

// spatial_samples[k] = value for a k the compiler cannot see: selects over constants, the array stays in registers
template <int N>
TR_DEV void set_slot(int (&sx)[N], int (&sy)[N], uint& good_bits, int k, int x, int y, bool good) {
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i == k) { sx[i] = x; sy[i] = y; good_bits = good ? (good_bits | (1u << i)) : (good_bits & ~(1u << i)); }
}
template <int N>
TR_DEV void get_slot(const int (&sx)[N], const int (&sy)[N], int k, int& x, int& y) {
    x = -1; y = -1;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i == k) { x = sx[i]; y = sy[i]; }
}

TR_DEV void restir_write_spatial(RestirSpatialRecord* dst, const RestirSpatialRecord& srec) {
    restir_set_word(dst, 0, u4{(uint)srec.px, (uint)srec.py, srec.good, srec.selected});
    restir_set_word(dst, 1, u4{TR_U(srec.target_n), TR_U(srec.visibility_n), TR_U(srec.jacobian_n), TR_U(srec.m)});
    restir_set_word(dst, 2, u4{TR_U(srec.wi), TR_U(srec.draw), TR_U(srec.target_c), TR_U(srec.visibility_c)});
    restir_set_word(dst, 3, u4{TR_U(srec.jacobian_c), TR_U(srec.mis_canonical), 0u, 0u});
}
TR_DEV void restir_write_final(RestirFinalRecord* dst, const RestirFinalRecord& frec) {
    restir_set_word(dst, 0, u4{TR_U(frec.contribution.x), TR_U(frec.contribution.y), TR_U(frec.contribution.z), TR_U(frec.visibility)});
    restir_set_word(dst, 1, u4{TR_U(frec.canonical_m), TR_U(frec.wi), TR_U(frec.draw), frec.selected});
}
// The records of a pixel without a surface (either pointer null without options.record)
template <int SPATIAL>
TR_DEV void restir_clear_records(RestirFinalRecord* rec_final, RestirSpatialRecord* rec_spatial, size_t pix) {
    const u4 zero = {0u, 0u, 0u, 0u};
    if (rec_final) { restir_set_word(rec_final + pix, 0, zero); restir_set_word(rec_final + pix, 1, zero); }
    if (rec_spatial)
        for (int i = 0; i < SPATIAL; ++i) {
            RestirSpatialRecord* rec = rec_spatial + (pix * SPATIAL + i);
            restir_set_word(rec, 0, u4{~0u, ~0u, 0u, 0u}); restir_set_word(rec, 1, zero); restir_set_word(rec, 2, zero); restir_set_word(rec, 3, zero);
        }
}

// `spatial` for SPATIAL > 0: the neighbour search and the pairwise-MIS merge of the neighbours' canonical reservoirs, the canonical one
// last.  surfaces, canonicals: the pixel's layer; rec_spatial: null or the chunk's records; ls: the spatial pass's sampler, untouched so
// far.  The scene view, the launch and what the pixel holds come in by value, and the merged reservoir, the canonical merge's record and
// the traversals' overflow go out by value: through references the loop is compiled against memory it cannot tell from the records it
// writes, and that schedule stays when it is inlined.  `cam` stays a reference into the scene's camera array.
// SHARED_VISIBILITY (restir_di.h's `visibility modes`, the shader's define of that name): neither re-evaluation
// traces - its visibility is restir_untraced - and a bad neighbour takes no slot.  The default, false, is the code as it was: ReSTIR GI
// and ReSTIR DI's per-target mode instantiate that.
template <class Kind>
struct RestirMerged { typename Kind::State r; RestirFinalRecord frec; int overflow; };
template <class Kind, bool TWO_LEVEL, int SPATIAL, bool SHARED_VISIBILITY = false>
TR_DEV RestirMerged<Kind> restir_spatial_merge(const SceneView sv, const LaunchCtx L, const CameraData& cam, float search_radius, float min_ray_dist,
                                               const RestirSurface* surfaces, const typename Kind::Reservoir* canonicals, RestirSpatialRecord* rec_spatial,
                                               int px, int py, size_t pix, const RestirDomain dom, const typename Kind::State canonical, LocalSampler ls,
                                               int* stack, int overflow) {
    typename Kind::State r = Kind::create();
    RestirFinalRecord frec = {F3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    constexpr int S = SPATIAL > 0 ? SPATIAL : 1;
    int sx[S], sy[S];
    uint good_bits = 0u;
#pragma unroll
    for (int i = 0; i < S; ++i) { sx[i] = -1; sy[i] = -1; }
    // `neighbours`: 2 * SPATIAL draws; good ones fill the slots from the front, bad ones from the back (restir_di_spatial.rgen:104-130)
    int good_neighbors = 0, bad_neighbors = 0;
    float inv_max_plane_dist;
    {   // get_inv_max_plane_dist (restir_di.glsl:398-403)
        float frustum_size = fmin2(fabsf(cam.proj_inverse.c[0].x * 2.0f), fabsf(cam.proj_inverse.c[1].y * 2.0f));
        frustum_size = frustum_size * fabsf(dot(F3(cam.view_inverse.c[2]), F3(cam.view_inverse.c[3]) - dom.pos));
        inv_max_plane_dist = 1.0f / frustum_size;
    }
    for (int i = 0; i < SPATIAL * 2; ++i) {
        const f4 rnd = u4_to_unit(pcg4d(ls.rs));
        const f2 d = search_radius * sample_blackman_harris_concentric_disk<RoundedMath>(F2(rnd.x, rnd.y));
        const int nx = px + (int)floorf(d.x + 0.5f), ny = py + (int)floorf(d.y + 0.5f);
        if ((uint)nx >= L.launch_w || (uint)ny >= L.launch_h) continue;
        f3 npos, nflat;
        int nid;
        restir_load_surface_head(surfaces + (size_t)ny * L.launch_w + (uint)nx, npos, nid, nflat);
        if (nid < 0) continue;
        const float edge = clampf(1.0f - fabsf(dot(dom.flat_normal, npos - dom.pos)) * inv_max_plane_dist, 0.0f, 1.0f);
        const bool bad = edge < 0.99f || dot(nflat, dom.flat_normal) < 0.75f;
        if (!bad && good_neighbors < SPATIAL) {
            set_slot(sx, sy, good_bits, good_neighbors, nx, ny, true);
            ++good_neighbors;
        } else if (!SHARED_VISIBILITY && bad && good_neighbors + bad_neighbors < SPATIAL) {     // restir_di_spatial.rgen:123-129
            ++bad_neighbors;
            set_slot(sx, sy, good_bits, SPATIAL - bad_neighbors, nx, ny, false);
        }
    }
    float total_confidence = canonical.confidence;
#pragma unroll
    for (int i = 0; i < S; ++i)
        if (sx[i] >= 0) total_confidence = total_confidence + Kind::confidence(canonicals + (size_t)sy[i] * L.launch_w + (uint)sx[i]);
    float canonical_m = canonical.confidence / total_confidence;
    const bool canonical_null = Kind::is_null(canonical.s);
    // one copy of the two re-evaluations and their traversals: the loop stays a loop, the slot is read by selects over constants
#pragma unroll 1
    for (int i = 0; i < SPATIAL; ++i) {
        int nx, ny;
        get_slot(sx, sy, i, nx, ny);
        RestirSpatialRecord srec = {nx, ny, (good_bits >> i) & 1u, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (nx >= 0) {
            const size_t npix = (size_t)ny * L.launch_w + (uint)nx;
            RestirDomain sample_domain;      // the whole surface ahead of the first traversal, or only its position and the rest behind it
            if (Kind::SURFACE_LATE) {
                f3 nflat;
                int nid;
                restir_load_surface_head(surfaces + npix, sample_domain.pos, nid, nflat);
            } else {
                restir_load_surface(surfaces + npix, sample_domain);
            }
            const typename Kind::State n = Kind::load(canonicals + npix);
            if (!Kind::is_null(n.s)) {
                typename Kind::Eval e;
                const f3 contrib = Kind::contribution(sv, n.s, dom, e);
                const float visibility = SHARED_VISIBILITY ? restir_untraced(contrib)
                                                           : restir_shadow<TWO_LEVEL>(sv, min_ray_dist, dom.pos, contrib, e.dir, e.dist2, stack, overflow);
                const float target = rgb_to_luminance(contrib * visibility);
                const float jacob = Kind::jacobian(n.s, e, sample_domain.pos, dom.pos);
                const float m = restir_mis_noncanonical(canonical.confidence, n.confidence, total_confidence, n.target_function, target, jacob);
                float wi = ((target * m) * n.uc_weight) * jacob;
                if (isnan(wi)) wi = 0.0f;
                const float u = u4_to_unit(pcg4d(ls.rs)).x;
                const bool selected = restir_update(r, n.s, wi, u);
                if (selected) r.target_function = target;
                srec.selected = selected ? 1u : 0u; srec.target_n = target; srec.visibility_n = visibility; srec.jacobian_n = jacob; srec.m = m; srec.wi = wi; srec.draw = u;
            }
            r.confidence = r.confidence + n.confidence;
            if (!canonical_null) {
                if (Kind::SURFACE_LATE) restir_load_surface(surfaces + npix, sample_domain);
                typename Kind::Eval e;
                const f3 contrib = Kind::contribution(sv, canonical.s, sample_domain, e);
                const float visibility = SHARED_VISIBILITY ? restir_untraced(contrib)
                                                           : restir_shadow<TWO_LEVEL>(sv, min_ray_dist, sample_domain.pos, contrib, e.dir, e.dist2, stack, overflow);
                const float alt_target = rgb_to_luminance(contrib * visibility);
                const float jacob = Kind::jacobian(canonical.s, e, dom.pos, sample_domain.pos);
                const float mc = restir_mis_canonical(canonical.confidence, n.confidence, total_confidence, canonical.target_function, alt_target, jacob);
                canonical_m = canonical_m + mc;
                srec.target_c = alt_target; srec.visibility_c = visibility; srec.jacobian_c = jacob; srec.mis_canonical = mc;
            }
        }
        if (rec_spatial) restir_write_spatial(rec_spatial + (pix * SPATIAL + i), srec);
    }
    float wi = (canonical_m * canonical.target_function) * canonical.uc_weight;
    if (isnan(wi)) wi = 0.0f;
    const float u = u4_to_unit(pcg4d(ls.rs)).x;
    const bool selected = restir_update(r, canonical.s, wi, u);
    if (selected) r.target_function = canonical.target_function;
    r.confidence = r.confidence + canonical.confidence;
    r.uc_weight = restir_uc_weight(r);
    frec.canonical_m = canonical_m; frec.wi = wi; frec.draw = u; frec.selected = selected ? 1u : 0u;
    return {r, frec, overflow};
}

// ---------------------------------------------------------------------------------------------------
// The host skeleton of restir_di.hip and restir_gi.hip.  `api` is "trhip_restir_di" or "trhip_restir_gi": the messages name the entry
// point.  A stage struct derives from RestirStageHost and adds `opt` (its trhip_restir_*_options) and its own buffers.

template <int EVENTS>
struct RestirStageHost : StageHost<EVENTS> {
    trhip_device* dev = nullptr;
    uint32_t w = 0, h = 0, layers = 0;
    uint32_t frame = 0;                      // frames since create or reset: the sampler's frame, the surface pair's parity
    std::vector<uint32_t> viewports;         // the last frame's list: layer i's history belongs to viewports[i]
    RestirSurface* surface[2] = {nullptr, nullptr};
    RestirTemporalRecord* rec_temporal = nullptr;      // null unless options.record, as the two below
    RestirSpatialRecord* rec_spatial = nullptr;
    RestirFinalRecord* rec_final = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
};

// trhip_restir_*_create: own_checks() refuses the options only this stage has (behind the null checks, ahead of the shared options),
// own_buffers(s, n) allocates its buffers for n pixels behind the shared ones.
template <class Stage, class Options, class OwnChecks, class OwnBuffers>
int restir_create(const std::string& api, trhip_device* dev, const Options* opt, uint32_t width, uint32_t height, uint32_t layers, Stage** out,
                  OwnChecks own_checks, OwnBuffers own_buffers) {
    const std::string fn = api + "_create";
    if (!out) return set_error(fn + ": null out");
    *out = nullptr;
    if (!opt) return set_error(fn + ": null options");
    if (int r = own_checks(fn)) return r;
    if (opt->spatial_samples > (uint32_t)RESTIR_MAX_SPATIAL) return set_error(fn + ": spatial_samples " + std::to_string(opt->spatial_samples) + " is outside 0..4");
    if (!(opt->search_radius > 0.0f) || !(opt->search_radius <= 1024.0f)) return set_error(fn + ": search_radius must be in (0, 1024]");
    if (!(opt->max_confidence >= 1.0f) || !std::isfinite(opt->max_confidence)) return set_error(fn + ": max_confidence must be finite and at least 1");
    if (opt->temporal_reuse != 0 && opt->temporal_reuse != 1) return set_error(fn + ": temporal_reuse must be 0 or 1");
    if (!(opt->min_ray_dist > 0.0f) || !std::isfinite(opt->min_ray_dist)) return set_error(fn + ": min_ray_dist must be finite and positive");
    if (opt->record != 0 && opt->record != 1) return set_error(fn + ": record must be 0 or 1");
    if (width == 0 || height == 0 || layers == 0) return set_error(fn + ": zero width, height or layer count");
    if (width > 16384 || height > 16384 || layers > 4096) return set_error(fn + ": image too large");
    if (!dev) return set_error(fn + ": null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    Stage* s = new Stage;
    s->dev = dev; s->hip_device = device_index(dev);
    s->opt = *opt;
    s->w = width; s->h = height; s->layers = layers;
    const size_t n = s->pixels();
    s->alloc_zeroed(s->surface[0], n * sizeof(RestirSurface));
    s->alloc_zeroed(s->surface[1], n * sizeof(RestirSurface));
    if (opt->record) {
        s->alloc_zeroed(s->rec_temporal, n * sizeof(RestirTemporalRecord));
        if (opt->spatial_samples) s->alloc_zeroed(s->rec_spatial, n * opt->spatial_samples * sizeof(RestirSpatialRecord));
        s->alloc_zeroed(s->rec_final, n * sizeof(RestirFinalRecord));
    }
    own_buffers(s, n);
    return stage_finish_create(fn.c_str(), s, out);
}

template <class Stage>
int restir_reset(const std::string& api, Stage* s) {
    if (!s) return set_error(api + "_reset: null stage");
    s->frame = 0;
    return 0;
}

// The head of trhip_restir_*_render: the arguments, the device, the scene and the viewport list
template <class Stage>
int restir_begin_render(const std::string& api, Stage* s, const uint32_t* viewports, uint32_t count, const void* out_color_dev, DeviceScene*& scene) {
    const std::string fn = api + "_render";
    if (!s) return set_error(fn + ": null stage");
    if (!viewports || !out_color_dev) return set_error(fn + ": null argument");
    DEVCHK(s->hip_device);
    scene = device_scene(s->dev);
    if (int r = check_scene_ready(fn.c_str(), scene->instance_count, scene->accel_built)) return r;
    if (int r = check_viewport_list(fn.c_str(), viewports, count, s->layers, scene->camera_count)) return r;
    // History and the previous surface records are kept per layer, the position in the list: another list would merge another viewport's
    if (s->opt.temporal_reuse && s->frame > 0 && !std::equal(viewports, viewports + count, s->viewports.begin(), s->viewports.end()))
        return set_error(fn + ": the viewport list differs from the last frame's, whose history it would reuse: call " + api + "_reset first");
    return 0;
}

// The parameter fields both stages' kernels take
template <class Params, class Stage>
void restir_fill_params(Params& base, const Stage& s, const DeviceScene& scene) {
    base.search_radius = s.opt.search_radius; base.max_confidence = s.opt.max_confidence; base.min_ray_dist = s.opt.min_ray_dist;
    nee_probabilities(scene, 1.0f, 1.0f, 1.0f, 1.0f, base.prob_point, base.prob_tri, base.prob_dir, base.prob_env);
    { uint seed = s.opt.rng_seed; base.rng_seed = seed != 0 ? pcg(seed) : 0; }                  // src/rt_stage.cc:82
    base.frame = s.frame;
    base.has_history = s.frame > 0;
}

// The frame: every chunk's kernel of one pass, then the next pass (a chunk's launch reads only its own layers); ev[pass + 1] behind pass.
// fill(P, off) sets the stage's own pointers of a chunk that starts `off` pixels into the images; the shared ones are set here.
// The three steps are functions of their own for a frame whose passes take different parameter blocks (ReSTIR DI's power-proportional
// light selection: restir_di_power.h); restir_run_passes is the frame of one block.
template <class Stage>
int restir_begin_frame(Stage* s, hipStream_t st) {
    HIPCHK(hipEventRecord(s->ev[0], st));
    return 0;
}
template <class Stage, class Params, class Fill>
int restir_run_pass(Stage* s, DeviceScene* scene, int projection, const uint32_t* viewports, uint32_t count, hipStream_t st, const Params& base,
                    void (*kernel)(SceneView, LaunchCtx, int, ViewportList, Params, uint*), int pass, Fill fill) {
    const LaunchCtx L = whole_image_launch(s->w, s->h);
    const size_t layer_px = (size_t)s->w * s->h;
    const int cur = (int)(s->frame & 1u);
    for_each_viewport_chunk<ViewportList>(viewports, count, [&](uint32_t first, uint32_t n, const ViewportList& list) {
        Params P = base;
        const size_t off = first * layer_px;
        P.surface = s->surface[cur] + off; P.prev_surface = s->surface[cur ^ 1] + off;
        P.rec_temporal = s->rec_temporal ? s->rec_temporal + off : nullptr;
        P.rec_spatial = s->rec_spatial ? s->rec_spatial + off * s->opt.spatial_samples : nullptr;
        P.rec_final = s->rec_final ? s->rec_final + off : nullptr;
        fill(P, off);
        hipLaunchKernelGGL(kernel, tile_grid(s->w, s->h, n), dim3(TR_BLOCK), 0, st, scene->view(), L, projection, list, P, device_overflow_flag(s->dev));
    });
    HIPCHK(hipEventRecord(s->ev[pass + 1], st));
    return 0;
}
template <class Stage>
int restir_end_frame(Stage* s, const uint32_t* viewports, uint32_t count) {
    HIPCHK(hipGetLastError());
    s->frames += 1;
    s->frame += 1;
    s->viewports.assign(viewports, viewports + count);
    return 0;
}
template <class Stage, class Params, class Fill>
int restir_run_passes(Stage* s, DeviceScene* scene, int projection, const uint32_t* viewports, uint32_t count, hipStream_t st, const Params& base,
                      void (*const* kernels)(SceneView, LaunchCtx, int, ViewportList, Params, uint*), int passes, Fill fill) {
    if (int r = restir_begin_frame(s, st)) return r;
    for (int pass = 0; pass < passes; ++pass)
        if (int r = restir_run_pass(s, scene, projection, viewports, count, st, base, kernels[pass], pass, fill)) return r;
    return restir_end_frame(s, viewports, count);
}

// trhip_restir_*_download: shared[] = the stage's codes of the surface, temporal, spatial and final records; decision: `which` is a
// decision record; own(n, src, size) names the stage's other buffers and is false for a code it does not know.
template <class Stage, class Own>
int restir_download(const std::string& api, Stage* s, int which, void* host, size_t bytes, bool decision, const int (&shared)[4], Own own) {
    const std::string fn = api + "_download";
    return stage_download(fn.c_str(), s, host, bytes, [&](const void*& src, size_t& size) {
        const size_t n = s->pixels();
        if (decision && !s->opt.record) return set_error(fn + ": the decision records are only kept with record");
        if (which == shared[0]) { src = s->surface[(s->frame + 1u) & 1u]; size = n * sizeof(RestirSurface); }      // the half the last frame wrote
        else if (which == shared[1]) { src = s->rec_temporal; size = n * sizeof(RestirTemporalRecord); }
        else if (which == shared[2]) {
            if (!s->rec_spatial) return set_error(fn + ": the stage has no spatial samples");
            src = s->rec_spatial; size = n * s->opt.spatial_samples * sizeof(RestirSpatialRecord);
        }
        else if (which == shared[3]) { src = s->rec_final; size = n * sizeof(RestirFinalRecord); }
        else if (!own(n, src, size)) return set_error(fn + ": unknown buffer");
        return 0;
    });
}

}  // namespace tr
