// ReSTIR DI for gfx950, sphere lights as area lights (trhip_restir_di_set_sphere_lights; restir_di.h `sphere lights`, DESIGN.md
// section 35): a translation unit of its own, so that the kernels of restir_di.hip, restir_di_power.hip and restir_di_bsdf.hip stay the
// code they were (restir_di_sphere.h).
//   k_restir_di_canonical_sphere  k_restir_di_canonical (restir_di.hip), k_restir_di_canonical_power (POWER) or
//                                 k_restir_di_canonical_bsdf (BSDF) with restir_sphere_draw behind the sampler of the light candidates'
//                                 loop and the area mode's contribution: a candidate on a light with a radius is a point on its sphere
//   k_restir_di_spatial_sphere    k_restir_di_spatial (restir_di.hip) over the area mode's sample kind: the normal of a sphere sample
//                                 is not 0, so the unchanged merge gives it the solid-angle Jacobian of a triangle sample
// IEEE fp32 without contraction in a fixed order, vector stores only, no atomics: two runs of the same inputs give the same bits.
#include "restir_di_sphere.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;
using Kind = RestirDiSphereKind;

// BSDF = false: the candidate loop and the weights of k_restir_di_canonical; BSDF = true: those of k_restir_di_canonical_bsdf
template <bool TWO_LEVEL, bool TEMPORAL, int VISIBILITY, bool POWER, bool BSDF>
__global__ __launch_bounds__(KB, 2) void k_restir_di_canonical_sphere(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirBsdfParams P, uint* overflow_flag) {
    __shared__ int s_stack_rows[TR_STACK_WORDS];
    int* const s_stack = s_stack_rows + TR_STACK_ROW0;
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const uint layer = blockIdx.z, viewport = list.v[layer];
    const CameraData cam = sv.cameras[viewport];
    f3 ray_origin, dir;
    HitRecord hit;
    int overflow;
    first_hit<TWO_LEVEL>(sv, L, cam, projection, px, py, P.min_ray_dist, s_stack + threadIdx.x, ray_origin, dir, hit, overflow);
    const size_t layer_px = (size_t)L.launch_w * L.launch_h;
    const size_t pix = layer * layer_px + (size_t)py * L.launch_w + (uint)px;
    RestirDomain dom = {};
    Kind::State r = Kind::create();
    RestirTemporalRecord trec = restir_no_temporal();
    if (hit.instance_id >= 0) {
        SurfacePoint v;
        first_hit_surface(sv, hit, dir, ray_origin, v, dom.mat);
        dom.pos = v.pos; dom.mapped_normal = v.mapped_normal; dom.flat_normal = v.hard_normal;
        dom.view = normalize(v.pos - ray_origin);
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, 0u}, 2u * P.frame, P.rng_seed, SAMPLER_UNIFORM);

        RestirReprojection rp;
        if (TEMPORAL) {
            const f3 prev_pos = surface_prev_pos(sv, hit.instance_id, hit.primitive_id, hit.u, hit.v);
            const f3 m = get_camera_projection(sv.prev_cameras[viewport], projection, prev_pos);
            const f2 motion = F2(m.x, 1.0f - m.y) * F2((float)L.launch_w, (float)L.launch_h) - 0.5f;
            rp = restir_reproject<Kind>(L, P.has_history, P.prev_surface + layer * layer_px, P.history + layer * layer_px, dom, motion, length(ray_origin - dom.pos), ls);
        }

        const int total = BSDF ? P.candidates + P.bsdf_candidates : P.candidates;
        const float n_light = (float)P.candidates, n_bsdf = (float)P.bsdf_candidates;
        const float mis_weight = BSDF ? (float)total / ((float)total + rp.prev_confidence) : 1.0f / ((float)P.candidates + rp.prev_confidence);
        const m3 tbn = create_tangent_space(dom.mapped_normal);
        const f3 shading_view = view_to_tangent_space(dom.view, tbn);
        const HitRecord no_hit = {-1, -1, 0.0f, 0.0f, -1.0f};
        for (int i = 0; i < P.candidates; ++i) {
            const u4 rnd = pcg4d(ls.rs);
            RestirLightRecord Lr;
            float light_pdf;
            RestirSample s;
            if constexpr (POWER) s = restir_sample_canonical_power(sv, P, rnd, dom.pos, Lr, light_pdf);
            else s = restir_sample_canonical(sv, P, rnd, dom.pos, Lr, light_pdf);
            restir_sphere_draw(P, rnd, dom.pos, Lr, s, light_pdf);      // `sphere lights` 2
            f3 light_dir, light_norm;
            float light_dist2;
            const f3 contrib = restir_contribution<true>(sv, s, Lr, dom, light_dir, light_dist2, light_norm);
            const float visibility = VISIBILITY != 0 ? restir_untraced(contrib)
                                                     : restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
            const float target = rgb_to_luminance(contrib * visibility);
            float weight, p_b = 0.0f, denom = 0.0f;
            if constexpr (BSDF) {
                // `bsdf candidates` 8, `sphere lights` 6: the BSDF technique produces triangle and environment samples only
                if (s.type == 1u || s.type == 3u) p_b = restir_bsdf_pdf(dom, tbn, shading_view, light_dir);
                denom = n_light * light_pdf + n_bsdf * p_b;
                weight = restir_balance_weight(mis_weight, target, denom);
            } else {
                weight = mis_weight * target / light_pdf;
                if (isnan(weight)) weight = 0.0f;
            }
            const float u = u4_to_unit(pcg4d(ls.rs)).x;
            const bool selected = restir_update(r, s, weight, u);
            if (selected) r.target_function = target;
            r.confidence = r.confidence + 1.0f;
            if (P.rec_candidates) {
                const size_t slot = pix * (size_t)total + (uint)i;
                if constexpr (BSDF) {
                    restir_write_candidate(P, slot, s, light_pdf, contrib, visibility, weight, u, selected, 0u, light_dir, p_b, no_hit, false, denom);
                } else {
                    RestirCandidateRecord* rec = P.rec_candidates + slot;
                    restir_set_word(rec, 0, u4{s.type << 30 | s.index, TR_U(s.data.x), TR_U(s.data.y), TR_U(light_pdf)});
                    restir_set_word(rec, 1, u4{TR_U(contrib.x), TR_U(contrib.y), TR_U(contrib.z), TR_U(visibility)});
                    restir_set_word(rec, 2, u4{TR_U(weight), TR_U(u), selected ? 1u : 0u, 0u});
                }
            }
        }
        if constexpr (BSDF) {
            for (int i = 0; i < P.bsdf_candidates; ++i) {
                const f4 ur = u4_to_unit(pcg4d(ls.rs));
                const float u = u4_to_unit(pcg4d(ls.rs)).x;
                f3 out_dir;
                Lobes sampled_lobes = {0, 0, 0, 0};
                float sampler_pdf;      // not used: `bsdf candidates` 3
                ggx_bsdf_sample<RoundedMath>(ur, shading_view, dom.mat, out_dir, sampled_lobes, sampler_pdf);
                const bool no_dir = any_nan(out_dir) || (out_dir.x == 0.0f && out_dir.y == 0.0f && out_dir.z == 0.0f);
                const f3 bdir = no_dir ? F3(0.0f) : normalize(mul(tbn, out_dir));
                const float p_b = no_dir ? 0.0f : restir_bsdf_pdf(dom, tbn, shading_view, bdir);
                const bool cast = !no_dir && p_b > 0.0f && !(dot(bdir, dom.flat_normal) < 1e-6f);
                HitRecord bhit = no_hit;
                if (cast) {
                    TraceStats st = {};
                    trace_closest4<1, false, TWO_LEVEL>(sv, dom.pos, bdir, P.min_ray_dist, __builtin_huge_valf(), 0u, s_stack + threadIdx.x, bhit, st, overflow);
                }
                // a triangle or an environment sample, or null: never a sphere light (`sphere lights` 6)
                const RestirSample s = restir_sample_of_hit(sv, cast, bhit, bdir);
                const RestirLightRecord Lr = restir_fetch_light(sv, s);
                f3 light_dir, light_norm;
                float light_dist2;
                const f3 contrib = restir_contribution<true>(sv, s, Lr, dom, light_dir, light_dist2, light_norm);
                const float visibility = restir_untraced(contrib);
                const float target = rgb_to_luminance(contrib * visibility);
                const float p_l = restir_identity_light_pdf<POWER>(sv, P, s, Lr, dom.pos, light_dir);
                const float denom = n_light * p_l + n_bsdf * p_b;
                const float weight = restir_balance_weight(mis_weight, target, denom);
                const bool selected = restir_update(r, s, weight, u);
                if (selected) r.target_function = target;
                r.confidence = r.confidence + 1.0f;
                if (P.rec_candidates)
                    restir_write_candidate(P, pix * (size_t)total + (uint)(P.candidates + i), s, p_l, contrib, visibility, weight, u, selected, 1u, bdir, p_b, bhit, cast, denom);
            }
        }
        r.uc_weight = restir_uc_weight(r);
        float sampled_visibility = 1.0f;
        if (VISIBILITY == 2) {
            Kind::Eval e;
            const f3 contrib = Kind::contribution(sv, r.s, dom, e);
            sampled_visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, e.dir, e.dist2, s_stack + threadIdx.x, overflow);
        }
        if constexpr (VISIBILITY != 0)
            if (P.rec_sampled) restir_set_word(P.rec_sampled + pix, 0, u4{TR_U(sampled_visibility), TR_U(r.uc_weight), 0u, 0u});
        if (VISIBILITY == 2) r.uc_weight = r.uc_weight * sampled_visibility;

        if (TEMPORAL) restir_temporal_merge<Kind>(sv, L, rp, P.history + layer * layer_px, dom, P.max_confidence, ls, r, trec);
    } else if constexpr (VISIBILITY != 0) {
        if (P.rec_sampled) restir_set_word(P.rec_sampled + pix, 0, u4{TR_U(VISIBILITY == 2 ? 0.0f : 1.0f), 0u, 0u, 0u});
    }
    if (overflow) *overflow_flag = 1;
    restir_store_surface(P.surface + pix, dom, hit.instance_id >= 0 ? hit.instance_id : -1);
    Kind::store(P.canonical + pix, r);
    if (P.rec_temporal) restir_write_temporal(P.rec_temporal + pix, trec);
}

// k_restir_di_spatial of restir_di.hip, line for line, over the area mode's kind and the parameter block of this unit
template <bool TWO_LEVEL, int SPATIAL, int VISIBILITY>
__global__ __launch_bounds__(KB, 2) void k_restir_di_spatial_sphere(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirBsdfParams P, uint* overflow_flag) {
    __shared__ int s_stack_rows[TR_STACK_WORDS];
    int* const s_stack = s_stack_rows + TR_STACK_ROW0;
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const uint layer = blockIdx.z, viewport = list.v[layer];
    const size_t layer_px = (size_t)L.launch_w * L.launch_h;
    const size_t pix = layer * layer_px + (size_t)py * L.launch_w + (uint)px;
    RestirDomain dom;
    const int instance_id = restir_load_surface(P.surface + pix, dom);
    int overflow = 0;
    if (instance_id < 0) {      // the direct stage's miss colour, as k_restir_di_spatial
        const CameraData cam = sv.cameras[viewport];
        f3 origin, view;
        get_screen_camera_ray(L, px, py, cam, projection, false, F2(0), F2(0.5f), origin, view);
        f4 c = sv.environment_factor;
        if (sv.environment_proj >= 0) {
            f2 uv;
            uv.y = asinf(-view.y) / TR_PI + 0.5f;
            uv.x = atan2f(view.z, view.x) / (2 * TR_PI) + 0.5f;
            const f4 t = sample_envmap(sv, uv);
            c.x *= t.x; c.y *= t.y; c.z *= t.z;
        }
        f3 light = F3(0);
        for (uint i = 0; i < sv.directional_light_count; ++i) {
            const DirectionalLight dl = sv.directional_lights[i];
            if (dl.dir_cutoff >= 1.0f) continue;
            const float visible = stepf(dl.dir_cutoff, dot(view, -dl.dir));
            light += visible * dl.color / (2.0f * TR_PI * (1.0f - dl.dir_cutoff));
        }
        light += F3(c);
        Kind::store(P.history + pix, Kind::create());
        P.out[pix] = F4(light, 1.0f);
        restir_clear_records<SPATIAL>(P.rec_final, P.rec_spatial, pix);
        return;
    }
    const Kind::State canonical = Kind::load(P.canonical + pix);
    Kind::State r = canonical;
    RestirFinalRecord frec = {F3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    if (SPATIAL > 0) {
        const LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, 0u}, 2u * P.frame + 1u, P.rng_seed, SAMPLER_UNIFORM);
        const RestirMerged<Kind> m = restir_spatial_merge<Kind, TWO_LEVEL, SPATIAL, VISIBILITY != 0>(sv, L, sv.cameras[viewport], P.search_radius, P.min_ray_dist,
            P.surface + layer * layer_px, P.canonical + layer * layer_px, P.rec_spatial, px, py, pix, dom, canonical, ls, s_stack + threadIdx.x, overflow);
        r = m.r; frec = m.frec; overflow = m.overflow;
    }
    Kind::Eval e;
    const f3 contrib = Kind::contribution(sv, r.s, dom, e);
    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, e.dir, e.dist2, s_stack + threadIdx.x, overflow);
    if (overflow) *overflow_flag = 1;
    const f3 shaded = contrib * visibility;
    if (VISIBILITY == 2) r.uc_weight = r.uc_weight * visibility;
    Kind::store(P.history + pix, r);
    P.out[pix] = F4(shaded * r.uc_weight + dom.mat.emission, 1.0f);
    frec.contribution = contrib; frec.visibility = visibility;
    if (P.rec_final) restir_write_final(P.rec_final + pix, frec);
}

template <bool TWO_LEVEL, bool TEMPORAL, bool POWER, bool BSDF>
RestirSphereKernel canonical_of(int visibility) {
    switch (visibility) {
        case 0: return k_restir_di_canonical_sphere<TWO_LEVEL, TEMPORAL, 0, POWER, BSDF>;
        case 1: return k_restir_di_canonical_sphere<TWO_LEVEL, TEMPORAL, 1, POWER, BSDF>;
        default: return k_restir_di_canonical_sphere<TWO_LEVEL, TEMPORAL, 2, POWER, BSDF>;
    }
}
template <bool TWO_LEVEL, bool TEMPORAL>
RestirSphereKernel canonical_of(int visibility, bool power, bool bsdf) {
    if (bsdf) return power ? canonical_of<TWO_LEVEL, TEMPORAL, true, true>(visibility) : canonical_of<TWO_LEVEL, TEMPORAL, false, true>(visibility);
    return power ? canonical_of<TWO_LEVEL, TEMPORAL, true, false>(visibility) : canonical_of<TWO_LEVEL, TEMPORAL, false, false>(visibility);
}

template <bool TWO_LEVEL, int VISIBILITY>
RestirSphereKernel spatial_of(uint32_t spatial) {
    switch (spatial) {
        case 0: return k_restir_di_spatial_sphere<TWO_LEVEL, 0, VISIBILITY>;
        case 1: return k_restir_di_spatial_sphere<TWO_LEVEL, 1, VISIBILITY>;
        case 2: return k_restir_di_spatial_sphere<TWO_LEVEL, 2, VISIBILITY>;
        case 3: return k_restir_di_spatial_sphere<TWO_LEVEL, 3, VISIBILITY>;
        default: return k_restir_di_spatial_sphere<TWO_LEVEL, 4, VISIBILITY>;
    }
}
template <bool TWO_LEVEL>
RestirSphereKernel spatial_of(uint32_t spatial, int visibility) {
    switch (visibility) {
        case 0: return spatial_of<TWO_LEVEL, 0>(spatial);
        case 1: return spatial_of<TWO_LEVEL, 1>(spatial);
        default: return spatial_of<TWO_LEVEL, 2>(spatial);
    }
}

}  // namespace

RestirSphereKernel restir_di_sphere_canonical_kernel(bool two_level, bool temporal, int visibility, bool power, bool bsdf) {
    if (two_level) return temporal ? canonical_of<true, true>(visibility, power, bsdf) : canonical_of<true, false>(visibility, power, bsdf);
    return temporal ? canonical_of<false, true>(visibility, power, bsdf) : canonical_of<false, false>(visibility, power, bsdf);
}

RestirSphereKernel restir_di_sphere_spatial_kernel(bool two_level, uint32_t spatial, int visibility) {
    return two_level ? spatial_of<true>(spatial, visibility) : spatial_of<false>(spatial, visibility);
}

}  // namespace tr
