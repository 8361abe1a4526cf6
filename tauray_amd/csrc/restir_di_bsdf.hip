// ReSTIR DI for gfx950, the BSDF-sampled candidates (trhip_restir_di_set_bsdf_candidates; restir_di.h `bsdf candidates`, DESIGN.md
// section 34): a translation unit of its own, so that the kernels of restir_di.hip and restir_di_power.hip stay the code they were
// (restir_di_bsdf.h).
//   k_restir_di_canonical_bsdf   k_restir_di_canonical (restir_di.hip) with two candidate loops: the light candidates, drawn as ever
//                                (POWER: through the table, restir_di_power.h), then the BSDF candidates - a direction from
//                                ggx_bsdf_sample<RoundedMath>, one closest-hit ray, the emissive triangle or the environment it finds
//                                as an ordinary light sample - all weighted by the balance heuristic over the two techniques
// IEEE fp32 without contraction in a fixed order, vector stores only, no atomics: two runs of the same inputs give the same bits.
#include "restir_di_bsdf.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;
using Kind = RestirDiKind;

// k_restir_di_canonical of restir_di.hip, line for line, but for the weights of the light candidates' loop, the second loop behind it
// and the parameter block
template <bool TWO_LEVEL, bool TEMPORAL, int VISIBILITY, bool POWER>
__global__ __launch_bounds__(KB, 2) void k_restir_di_canonical_bsdf(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirBsdfParams P, uint* overflow_flag) {
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

        // `bsdf candidates` 9: the balance heuristic over L light and B BSDF candidates
        const int total = P.candidates + P.bsdf_candidates;
        const float n_light = (float)P.candidates, n_bsdf = (float)P.bsdf_candidates;
        const float mis_weight = (float)total / ((float)total + rp.prev_confidence);
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
            f3 light_dir, light_norm;
            float light_dist2;
            const f3 contrib = restir_contribution(sv, s, Lr, dom, light_dir, light_dist2, light_norm);
            const float visibility = VISIBILITY != 0 ? restir_untraced(contrib)
                                                     : restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
            const float target = rgb_to_luminance(contrib * visibility);
            // `bsdf candidates` 8: the BSDF technique produces triangle and environment samples only
            float p_b = 0.0f;
            if (s.type == 1u || s.type == 3u) p_b = restir_bsdf_pdf(dom, tbn, shading_view, light_dir);
            const float denom = n_light * light_pdf + n_bsdf * p_b;
            const float weight = restir_balance_weight(mis_weight, target, denom);
            const float u = u4_to_unit(pcg4d(ls.rs)).x;
            const bool selected = restir_update(r, s, weight, u);
            if (selected) r.target_function = target;
            r.confidence = r.confidence + 1.0f;
            if (P.rec_candidates)
                restir_write_candidate(P, pix * (size_t)total + (uint)i, s, light_pdf, contrib, visibility, weight, u, selected, 0u, light_dir, p_b, no_hit, false, denom);
        }
        for (int i = 0; i < P.bsdf_candidates; ++i) {
            // `bsdf candidates` 1 to 4: two draws whatever becomes of the candidate
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
            // 5: the one traversal of the loop; a null candidate skips it by predicate
            HitRecord bhit = no_hit;
            if (cast) {
                TraceStats st = {};
                trace_closest4<1, false, TWO_LEVEL>(sv, dom.pos, bdir, P.min_ray_dist, __builtin_huge_valf(), 0u, s_stack + threadIdx.x, bhit, st, overflow);
            }
            const RestirSample s = restir_sample_of_hit(sv, cast, bhit, bdir);
            // 6: the light's record only now, and the sample evaluated like any other; the closest-hit ray was its visibility
            const RestirLightRecord Lr = restir_fetch_light(sv, s);
            f3 light_dir, light_norm;
            float light_dist2;
            const f3 contrib = restir_contribution(sv, s, Lr, dom, light_dir, light_dist2, light_norm);
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

template <bool TWO_LEVEL, bool TEMPORAL, bool POWER>
RestirBsdfKernel canonical_of(int visibility) {
    switch (visibility) {
        case 0: return k_restir_di_canonical_bsdf<TWO_LEVEL, TEMPORAL, 0, POWER>;
        case 1: return k_restir_di_canonical_bsdf<TWO_LEVEL, TEMPORAL, 1, POWER>;
        default: return k_restir_di_canonical_bsdf<TWO_LEVEL, TEMPORAL, 2, POWER>;
    }
}
template <bool TWO_LEVEL, bool TEMPORAL>
RestirBsdfKernel canonical_of(int visibility, bool power) {
    return power ? canonical_of<TWO_LEVEL, TEMPORAL, true>(visibility) : canonical_of<TWO_LEVEL, TEMPORAL, false>(visibility);
}

}  // namespace

RestirBsdfKernel restir_di_bsdf_canonical_kernel(bool two_level, bool temporal, int visibility, bool power) {
    if (two_level) return temporal ? canonical_of<true, true>(visibility, power) : canonical_of<true, false>(visibility, power);
    return temporal ? canonical_of<false, true>(visibility, power) : canonical_of<false, false>(visibility, power);
}

}  // namespace tr
