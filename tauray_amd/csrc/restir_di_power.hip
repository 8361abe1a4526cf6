// ReSTIR DI for gfx950, the power-proportional light selection (trhip_restir_di_set_light_selection; restir_di.h `light selection`,
// DESIGN.md section 33): a translation unit of its own, so that restir_di.hip's kernels stay the code they were (restir_di_power.h).
//   k_restir_light_weights        one thread per point and triangle light: the light's weight, float [n_point + n_tri]
//   k_restir_di_canonical_power   k_restir_di_canonical (restir_di.hip) with restir_sample_canonical_power in its candidate loop: each
//                                 candidate costs one dependent 16-byte load, the table entry, ahead of the light record's
// Both are IEEE fp32 without contraction in a fixed order, vector stores only, no atomics.
#include "restir_di_power.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;
using Kind = RestirDiKind;

// restir_di.h `light selection`, `weights`.  The spot cone and the radius of a point light and the emission texture of a triangle are not
// part of the weight: the uniform share of the pdf covers what the weight leaves out.
__global__ __launch_bounds__(KB) void k_restir_light_weights(SceneView sv, float* weights) {
    const uint i = blockIdx.x * (uint)KB + threadIdx.x;
    const uint n_point = sv.point_light_count, n_tri = sv.tri_light_count;
    if (i >= n_point + n_tri) return;
    float w;
    if (i < n_point) {
        const u4 r0 = *reinterpret_cast<const u4*>(sv.point_lights + i);
        w = rgb_to_luminance(F3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)));
    } else {
        const u4* rec = reinterpret_cast<const u4*>(sv.tri_lights + (i - n_point));
        const u4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
#define TR_F(x) __uint_as_float(x)
        const f3 P0 = F3(TR_F(r0.x), TR_F(r0.y), TR_F(r0.z)), P1 = F3(TR_F(r0.w), TR_F(r1.x), TR_F(r1.y)), P2 = F3(TR_F(r1.z), TR_F(r1.w), TR_F(r2.x));
#undef TR_F
        w = rgb_to_luminance(r9g9b9e5_to_rgb(r2.y)) * (0.5f * length(cross(P1 - P0, P2 - P0)));
    }
    if (!(w > 0.0f) || isinf(w)) w = 0.0f;      // negative, NaN or infinite
    weights[i] = w;
}

// k_restir_di_canonical of restir_di.hip, line for line, but for the sampler of the candidate loop and the parameter block
template <bool TWO_LEVEL, bool TEMPORAL, int VISIBILITY>
__global__ __launch_bounds__(KB, 2) void k_restir_di_canonical_power(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirPowerParams P, uint* overflow_flag) {
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

        const float mis_weight = 1.0f / ((float)P.candidates + rp.prev_confidence);
        for (int i = 0; i < P.candidates; ++i) {
            const u4 rnd = pcg4d(ls.rs);
            RestirLightRecord Lr;
            float light_pdf;
            const RestirSample s = restir_sample_canonical_power(sv, P, rnd, dom.pos, Lr, light_pdf);
            f3 light_dir, light_norm;
            float light_dist2;
            const f3 contrib = restir_contribution(sv, s, Lr, dom, light_dir, light_dist2, light_norm);
            const float visibility = VISIBILITY != 0 ? restir_untraced(contrib)
                                                     : restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
            const float target = rgb_to_luminance(contrib * visibility);
            float weight = mis_weight * target / light_pdf;
            if (isnan(weight)) weight = 0.0f;
            const float u = u4_to_unit(pcg4d(ls.rs)).x;
            const bool selected = restir_update(r, s, weight, u);
            if (selected) r.target_function = target;
            r.confidence = r.confidence + 1.0f;
            if (P.rec_candidates) {
                RestirCandidateRecord* rec = P.rec_candidates + (pix * (size_t)P.candidates + (uint)i);
                restir_set_word(rec, 0, u4{s.type << 30 | s.index, TR_U(s.data.x), TR_U(s.data.y), TR_U(light_pdf)});
                restir_set_word(rec, 1, u4{TR_U(contrib.x), TR_U(contrib.y), TR_U(contrib.z), TR_U(visibility)});
                restir_set_word(rec, 2, u4{TR_U(weight), TR_U(u), selected ? 1u : 0u, 0u});
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

template <bool TWO_LEVEL, bool TEMPORAL>
RestirPowerKernel canonical_of(int visibility) {
    switch (visibility) {
        case 0: return k_restir_di_canonical_power<TWO_LEVEL, TEMPORAL, 0>;
        case 1: return k_restir_di_canonical_power<TWO_LEVEL, TEMPORAL, 1>;
        default: return k_restir_di_canonical_power<TWO_LEVEL, TEMPORAL, 2>;
    }
}

}  // namespace

RestirPowerKernel restir_di_power_canonical_kernel(bool two_level, bool temporal, int visibility) {
    if (two_level) return temporal ? canonical_of<true, true>(visibility) : canonical_of<true, false>(visibility);
    return temporal ? canonical_of<false, true>(visibility) : canonical_of<false, false>(visibility);
}

hipError_t restir_launch_light_weights(const SceneView& sv, float* weights, hipStream_t stream) {
    const uint n = sv.point_light_count + sv.tri_light_count;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_restir_light_weights, dim3((n + (uint)KB - 1u) / (uint)KB), dim3(KB), 0, stream, sv, weights);
    return hipGetLastError();
}

}  // namespace tr
