// ReSTIR GI - reservoir resampling of indirect light (after Ouyang, Liu, Kettunen, Pharr and Pantaleoni, "ReSTIR GI: Path
// Resampling for Real-Time Path Tracing", 2021, and restir_di.h, whose resampling rule it keeps): constants, layouts, the order of
// operations and the order of random draws of k_restir_gi_initial, k_restir_gi_temporal and k_restir_gi_spatial (restir_gi.hip) behind the
// entry points trhip_restir_gi_* (include/trhip.h).  The reference has no such renderer; the rule is this project's own.
// tests/restir_gi_model.py repeats this file in float32 and float64.  What is not restated here is restir_di.h's, word for word: the
// surface record, update_reservoir, reprojection, reuse, neighbours, the Jacobian, mis_canonical and mis_noncanonical.
//
// A sample is a point x_s on a surface, its geometric normal n_s on the side the pixel's ray arrived from, and the radiance L_o it sent
// towards the pixel that found it: DI's triangle-light sample with the light replaced by a traced secondary hit.  The null sample has
// n_s = 0 and L_o = 0.
//
// Layouts (all fp32 / u32 / i32, [layers][h][w] records):
//   surface record    RestirSurface (restir_di.h) through first_hit / first_hit_surface, as DI writes it; frame f writes half f & 1
//   reservoir         RestirGiReservoir, 48 bytes = three aligned 16-byte words: x_s + uc_weight, n_s + target_function, L_o + confidence.
//                     `canonical` is written by the initial kernel (the initial sample, its pdf in uc_weight's place, its target, confidence
//                     0), rewritten in place by the temporal kernel (each pixel reads and writes its own record) and read by the spatial
//                     one; `history` is written by the spatial kernel and read by the next frame's temporal kernel.
//   reprojection      RestirGiReproject, 16 bytes, written by the initial kernel (which has the hit), read by the temporal one: the
//                     reprojected pixel position before the stochastic rounding, and length(ray origin - pos)
//   decision records  (options.record) RestirGiInitialRecord [pixel], x_s's RestirSurface [pixel], its light sample as a
//                     RestirCandidateRecord [pixel] (weight, draw, selected stay 0), RestirTemporalRecord [pixel], RestirSpatialRecord
//                     [pixel][spatial_samples], RestirFinalRecord [pixel]  (the last three: restir_di.h's); with bounces > 1 a
//                     RestirGiPathRecord and the vertex's RestirSurface [pixel][bounces - 1], one per extra vertex x_2 ... x_bounces
//
// Random draws.  sampler = init_local_sampler((px, py, viewport, 0x80000000), 3 * frame + pass, pcg(rng_seed) or 0, uniform) (rng.h),
// pass = 0, 1, 2 in the initial, temporal and spatial kernel, frame = the stage's frame counter: three streams disjoint from each other
// and, for less than 2^30 frames, from both of DI's at every frame (DI's fourth coordinate is 2 * frame + pass, below 2^31; a fourth
// coordinate of 1 would not do: 1 + 3 * frame + pass meets DI's 2 * frame' + pass').  A draw is pcg4d(sampler.rs); "unit" =
// float(word) * 2^-32 per component.  Order:
//   initial    one draw (unit .xy: the direction); if the secondary ray hits: one draw (the four words: sample_canonical at x_s);
//              [bounces > 1, behind those two, per extra vertex while the lane is alive: one draw (unit .xy: the direction), and
//              if the throughput survives: one draw (the four words: sample_canonical at the new vertex)]
//   temporal   [TEMPORAL: one draw, unit .xy: the reprojection]  one draw (unit .x: the selection of the initial sample)
//              [reuse: one draw, unit .x: the temporal merge]
//   spatial    2 * SPATIAL draws (unit .xy: the offsets), per slot that holds a neighbour whose sample is not null one draw (unit .x),
//              one draw (unit .x: the canonical merge)
//
// Order of operations (plain fp32, no contraction, correctly rounded divide and square root, dot left to right, RoundedMath (common.h)
// wherever a sin, cos, pow or atan2 is reached - as restir_di.h):
//   initial      at a pixel with a surface: local = sample_cosine_hemisphere<RoundedMath>(u.xy);
//                dir = create_tangent_space(mapped_normal) * local;  pdf = pdf_cosine_hemisphere(local);
//                dot(dir, flat_normal) < 1e-6f or pdf <= 0: the null sample, no ray.  Otherwise trace_closest4 from pos along dir from
//                min_ray_dist to infinity; a miss: the null sample (what that ray sees is direct light).  A hit is shaded with
//                first_hit_surface(sv, hit, dir, pos) into a surface record of its own (view = normalize(x_s - pos), flat_normal = the
//                hard normal, which shade_surface turns towards the ray); one sample_canonical draw at x_s with the scene's NEE
//                probabilities, its light_contribution at x_s's record and its shadow ray, as DI's candidate;
//                L_o = (contribution * visibility) / light_pdf per component, 0 if any component is NaN or inf; x_s's own emission is
//                not part of it (it is direct light at the pixel).  An L_o without a positive component: the null sample.
//                The sample is (x_s.pos, x_s.flat_normal, L_o).  This is bounces = 1.
//   path         bounces = B > 1 (trhip_restir_gi_set_bounces): L_o is the radiance of a path continued from x_1 := x_s, a vertex
//                treating the next one exactly as the pixel treats x_s.  dom_1 = x_s's surface record, T_1 = (1, 1, 1), L_o = NEE_1 =
//                the L_o above.  For k = 1 .. B - 1 while the lane is alive: one draw u; local = sample_cosine_hemisphere<RoundedMath>(u.xy);
//                dir_k = create_tangent_space(dom_k.mapped_normal) * local; pdf_k = pdf_cosine_hemisphere(local);
//                dot(dir_k, dom_k.flat_normal) < 1e-6f or pdf_k <= 0 ends the lane; else trace_closest4 from dom_k.pos along dir_k from
//                min_ray_dist to infinity; a miss ends the lane (what that ray sees is direct light at x_k, which NEE_k estimates); a
//                hit is dom_{k+1} = first_hit_surface(sv, hit, dir_k, dom_k.pos) with view = normalize(x_{k+1} - x_k);
//                f_k = contribution of the sample (x_{k+1}, dom_{k+1}.flat_normal, (1, 1, 1)) at dom_k, / pdf_k per component;
//                T_{k+1} = T_k * f_k per component; a T_{k+1} with a NaN or inf component or without a positive one ends the lane;
//                else one draw, the four words of sample_canonical at x_{k+1}, its light_contribution at dom_{k+1} and its shadow ray
//                as at x_1: NEE_{k+1} = (contribution * visibility) / light_pdf, non-finite -> 0; L_o = L_o + T_{k+1} * NEE_{k+1}.
//                The emission of a vertex is never added (it is direct light at the vertex before it, which that vertex's light
//                sample covers); no Russian roulette; cosine sampling only; limits 2 and 3 hold at every vertex.  The test for the
//                null sample, the target and the recorded L_o take the final sum: a path whose first light sample is black can
//                still carry light.
//   contribution of a sample at a surface: to = x_s - pos; dist2 = dot(to, to); dir = normalize(to); normal = n_s.  0 (with dir = 0,
//                dist2 = 0) for the null sample;  0 when not dist2 > 0, when dot(dir, flat_normal) < 1e-6f or when
//                dot(n_s, -dir) < 1e-6f;  else tbn, shading_view, shading_light, ggx_bsdf_pdf<RoundedMath>, correct_lobes_for_normal_map
//                and modulate_bsdf as DI's light_contribution has them behind its direction, times L_o
//   visibility   as DI: a contribution with a component > 0 casts trace_shadow4(pos, dir, min_ray_dist, sqrtf(dist2) - min_ray_dist);
//                target = rgb_to_luminance(contribution * visibility).  The initial sample's visibility is 1 by construction: no ray.
//   resampling   DI's with candidates = 1: weight = (1.0f / (1.0f + prev_confidence)) * target / pdf, NaN -> 0; update_reservoir;
//                confidence += 1; uc_weight = weight_sum > 0 ? weight_sum / target : 0
//   temporal     DI's reprojection, reuse and merge: target' = luminance(contribution of the history sample here), no shadow ray, no
//                Jacobian; weight = ((prev.confidence / (confidence + prev.confidence)) * target') * prev.uc_weight, NaN -> 0;
//                with TEMPORAL always confidence = min(confidence, max_confidence)
//   spatial      DI's neighbour search, slot filling and pairwise-MIS merge; j = reconnection_jacobian(npos, x_s, n_s, pos, x_s, n_s) =
//                restir_jacobian(npos, pos, x_s, n_s) for every sample that is not null (and the other way round for the canonical
//                sample at the neighbour); one shadow ray per re-evaluation; NaN weights are 0; the canonical merge comes last
//   colour       out.rgb = in.rgb + ((contribution of the chosen sample here * its shadow ray's visibility) * uc_weight); out.a = in.a;
//                a pixel without a surface copies `in` and keeps null reservoirs; a null `in` is (0, 0, 0, 1)
//
// Limits (trhip.h and DESIGN.md section 25 repeat them):
//   1. L_o is the radiance x_s sent towards the pixel that found it and is not evaluated again for a pixel that reuses the sample: the
//      paper's Lambertian assumption, a bias on glossy secondary surfaces.
//   2. No transmission: the contribution is 0 below the flat normal.
//   3. A surface with roughness below 0.001 gets no specular indirect light (ggx_bsdf_pdf's distribution is 0 there; no delta lobes).
//   4. History samples are not validated again when geometry or lights move; max_confidence bounds their age.
//   5. Sphere lights are points, as in DI.  Cosine-hemisphere sampling only, at most 8 bounces without Russian roulette, one device.
//
// Where the code is.  temporal, spatial and what they take from restir_di.h: restir_resample.h, the same code as ReSTIR DI's.  Here: the
// reservoir, the reprojection, initial and path records and RestirGiKind with `contribution`.  initial, resampling and colour:
// restir_gi.hip; `path`: restir_gi_path.hip (restir_gi_path.h: the kernels' parameters, shared by the two).
#pragma once
#include "restir_di.h"

namespace tr {

constexpr uint RESTIR_GI_SAMPLER_W = 0x80000000u;    // the fourth sampler coordinate of the stage's three streams

struct alignas(16) RestirGiReservoir {   // trhip_restir_gi_reservoir
    f3 x_s; float uc_weight;
    f3 n_s; float target_function;
    f3 L_o; float confidence;
};
struct alignas(16) RestirGiReproject {
    f2 motion; float origin_dist, pad;
};
struct RestirGiInitialRecord {           // trhip_restir_gi_initial
    f2 draw; float pdf; uint traced;     // unit .xy of the direction's draw; traced: the secondary ray was cast
    f3 dir; float t;                     // the secondary hit (instance_id -1: none), as trace_closest4 returns it
    int instance_id, primitive_id; float u, v;
    u4 light_draw;                       // the four words sample_canonical took at x_s (0 without a hit)
    f3 L_o; float target;                // target: of the initial sample at the pixel
    float weight, sel_draw; uint selected, pad;   // the temporal kernel's update_reservoir of the initial sample
};
struct alignas(16) RestirGiPathRecord {  // trhip_restir_gi_path: extra vertex k + 1 of `path`, nine aligned 16-byte words
    f2 draw; float pdf; uint traced;     // unit .xy of dir_k's draw, pdf_k; traced: the ray was cast
    f3 dir; float t;                     // dir_k and its hit (instance_id -1: none), as trace_closest4 returns it
    int instance_id, primitive_id; float u, v;
    u4 light_draw;                       // the four words sample_canonical took at x_{k+1} (0 where the lane ended before)
    uint light; f2 light_data; float light_pdf;      // the light sample as RestirCandidateRecord has it (RESTIR_NULL_INDEX: none)
    f3 contribution; float visibility;
    f3 factor; float pad0;               // f_k
    f3 throughput; float pad1;           // T_{k+1} (0 where no hit formed it)
    f3 L_o; float pad2;                  // the running sum behind this vertex
};
static_assert(sizeof(RestirGiReservoir) == 48 && sizeof(RestirGiReproject) == 16 && sizeof(RestirGiInitialRecord) == 96 && sizeof(RestirGiPathRecord) == 144, "layout");
constexpr uint RESTIR_GI_MAX_BOUNCES = 8u;

struct RestirGiSample { f3 x, n, L; };

// What restir_resample.h asks of a sample: a point, its normal and the radiance it sent
struct RestirGiKind {
    using Sample = RestirGiSample;
    using State = RestirState<Sample>;
    using Reservoir = RestirGiReservoir;
    struct Eval { f3 dir; float dist2; };
    // The spatial merge reads a neighbour's surface ahead of the first traversal: read behind it, the wait showed
    static constexpr bool SURFACE_LATE = false;
    static TR_DEV State create() { return {{F3(0.0f), F3(0.0f), F3(0.0f)}, 0.0f, 0.0f, 0.0f, 0.0f}; }
    static TR_DEV State load(const Reservoir* src) {
        const u4 a = restir_word(src, 0), b = restir_word(src, 1), c = restir_word(src, 2);
#define TR_F(x) __uint_as_float(x)
        State r;
        r.s.x = F3(TR_F(a.x), TR_F(a.y), TR_F(a.z)); r.uc_weight = TR_F(a.w);
        r.s.n = F3(TR_F(b.x), TR_F(b.y), TR_F(b.z)); r.target_function = TR_F(b.w);
        r.s.L = F3(TR_F(c.x), TR_F(c.y), TR_F(c.z)); r.confidence = TR_F(c.w);
#undef TR_F
        r.weight_sum = 0.0f;
        return r;
    }
    static TR_DEV void store(Reservoir* dst, const State& r) {
        restir_set_word(dst, 0, u4{TR_U(r.s.x.x), TR_U(r.s.x.y), TR_U(r.s.x.z), TR_U(r.uc_weight)});
        restir_set_word(dst, 1, u4{TR_U(r.s.n.x), TR_U(r.s.n.y), TR_U(r.s.n.z), TR_U(r.target_function)});
        restir_set_word(dst, 2, u4{TR_U(r.s.L.x), TR_U(r.s.L.y), TR_U(r.s.L.z), TR_U(r.confidence)});
    }
    static TR_DEV float confidence(const Reservoir* src) { return __uint_as_float(restir_word(src, 2).w); }
    static TR_DEV bool is_null(const Sample& s) {
        return s.n.x == 0.0f && s.n.y == 0.0f && s.n.z == 0.0f && s.L.x == 0.0f && s.L.y == 0.0f && s.L.z == 0.0f;
    }
    // `contribution` above: restir_contribution's tail behind the direction, times L_o
    static TR_DEV f3 contribution(const SceneView&, const Sample& s, const RestirDomain& dom, Eval& e) {
        e.dir = F3(0.0f); e.dist2 = 0.0f;
        if (is_null(s)) return F3(0.0f);
        const f3 to = s.x - dom.pos;
        e.dist2 = dot(to, to);
        e.dir = normalize(to);
        if (!(e.dist2 > 0.0f)) return F3(0.0f);
        if (dot(e.dir, dom.flat_normal) < 1e-6f) return F3(0.0f);
        if (dot(s.n, -e.dir) < 1e-6f) return F3(0.0f);
        const m3 tbn = create_tangent_space(dom.mapped_normal);
        const f3 shading_view = view_to_tangent_space(dom.view, tbn);
        const f3 shading_light = mulT(e.dir, tbn);
        Lobes lobes = {0, 0, 0, 0};
        ggx_bsdf_pdf<RoundedMath>(shading_light, shading_view, dom.mat, lobes);
        if (dot(dom.flat_normal, e.dir) < 0) { lobes.diffuse = 0; lobes.dielectric_reflection = 0; lobes.metallic_reflection = 0; }     // correct_lobes_for_normal_map
        else lobes.transmission = 0;
        return modulate_bsdf(dom.mat, lobes) * s.L;
    }
    // the reconnection point and its normal are the sample's own
    static TR_DEV float jacobian(const Sample& s, const Eval&, f3 from, f3 at) { return restir_jacobian(from, at, s.x, s.n); }
};

}  // namespace tr
