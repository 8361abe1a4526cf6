// ReSTIR DI's power-proportional light selection (restir_di.h `light selection`; trhip_restir_di_set_light_selection): what restir_di.hip
// and restir_di_power.hip share.  The kernels of the power mode - k_restir_light_weights and the twelve instances of
// k_restir_di_canonical_power - are a translation unit of their own, and that canonical kernel repeats k_restir_di_canonical around
// another sampler instead of sharing a body with it, so that the uniform instances stay the code they were: the inliner weighs a
// function by its callers in the unit, and a body shared through a function changes register allocation.  For
// the same reason the power kernel has a parameter block of its own, and RestirParams (restir_di.hip) keeps its layout.  The spatial
// kernel never sees a candidate's pdf: the power mode's frame launches the spatial instances that the uniform mode launches.
#pragma once
#include "restir_di.h"

namespace tr {

// RestirParams' fields (restir_di.hip) and two more.  rec_spatial and rec_final are the frame skeleton's; the canonical pass reads neither.
struct RestirPowerParams {
    int candidates;
    float search_radius, max_confidence, min_ray_dist;
    float prob_point, prob_tri, prob_dir, prob_env;
    uint rng_seed, frame;
    int has_history;
    RestirSurface* surface;
    const RestirSurface* prev_surface;
    RestirReservoir* canonical;
    RestirReservoir* history;
    f4* out;
    RestirCandidateRecord* rec_candidates;      // null unless options.record, as the five below
    RestirTemporalRecord* rec_temporal;
    RestirSpatialRecord* rec_spatial;
    RestirFinalRecord* rec_final;
    RestirSampledRecord* rec_sampled;           // written in the visibility modes shared and sampled only
    const AliasEntry* light_table;              // [point_light_count + tri_light_count]: the point lights' table, then the triangle lights'
};

using RestirPowerKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, RestirPowerParams, uint*);
RestirPowerKernel restir_di_power_canonical_kernel(bool two_level, bool temporal, int visibility);      // restir_di_power.hip

// k_restir_light_weights over the scene's point and triangle lights into weights[point_light_count + tri_light_count], on `stream`
hipError_t restir_launch_light_weights(const SceneView& sv, float* weights, hipStream_t stream);

// sample_canonical with the point and the triangle class drawn through the table (restir_di.h `light selection`, `draw`).  It repeats
// restir_sample_canonical: select, one masked fetch of the table entry, one masked fetch of the light record, compute.  The directional
// and the environment class are drawn as there, and so is the point on a triangle.
template <class Params>
TR_DEV RestirSample restir_sample_canonical_power(const SceneView& sv, const Params& P, u4 rnd, f3 pos, RestirLightRecord& L, float& light_pdf) {
    f4 u = u4_to_unit(rnd);
    enum { NONE = 0, POINT, TRI, DIR, ENV };
    int kind = NONE;
    if ((u.w -= P.prob_point) < 0) kind = POINT;
    else if ((u.w -= P.prob_tri) < 0) kind = TRI;
    else if ((u.w -= P.prob_dir) < 0) kind = DIR;
    else if ((u.w -= P.prob_env) < 0) kind = ENV;
    const int n_point = (int)sv.point_light_count, n_tri = (int)sv.tri_light_count, n_dir = (int)sv.directional_light_count;
    if ((kind == POINT && n_point <= 0) || (kind == TRI && n_tri <= 0) || (kind == DIR && n_dir <= 0) || (kind == ENV && sv.environment_proj < 0)) kind = NONE;
    asm volatile("" : "+v"(kind));
    const int light_count = kind == POINT ? n_point : kind == TRI ? n_tri : n_dir;
    int light_index = clampi((int)(u.z * light_count), 0, light_count - 1);      // the directional class; the other two below
    // the slot is the high word of word * n, what is left of the word decides between the slot and its alias
    const bool tabled = kind == POINT || kind == TRI;
    const unsigned long long scaled = (unsigned long long)(kind == POINT ? rnd.x : rnd.z) * (unsigned long long)(uint)light_count;
    const uint slot = (uint)(scaled >> 32), low = (uint)scaled;
    u4 entry = {0u, 0u, 0u, 0u};
    if (tabled) entry = *reinterpret_cast<const u4*>(P.light_table + ((kind == TRI ? (uint)n_point : 0u) + slot));
    const bool take_alias = low > entry.y;
    const float table_pdf = __uint_as_float(take_alias ? entry.w : entry.z);
    // an alias is a slot of the same table (tauray_alias.hh); the clamp keeps the fetch inside the array whatever the table holds
    if (tabled) light_index = (int)clampu(take_alias ? entry.x : slot, 0u, (uint)light_count - 1u);
    L.r0 = u4{0u, 0u, 0u, 0u}; L.r1 = L.r0; L.r2 = L.r0; L.r3 = L.r0;
    int alias_i = 0;
    if (kind == POINT) { const u4* rec = reinterpret_cast<const u4*>(sv.point_lights + light_index); L.r0 = rec[0]; L.r1 = rec[1]; L.r2 = rec[2]; L.r3 = rec[3]; }
    if (kind == TRI) { const u4* rec = reinterpret_cast<const u4*>(sv.tri_lights + light_index); L.r0 = rec[0]; L.r1 = rec[1]; L.r2 = rec[2]; L.r3 = rec[3]; }
    if (kind == DIR) { const u4* rec = reinterpret_cast<const u4*>(sv.directional_lights + light_index); L.r0 = rec[0]; L.r1 = rec[1]; }
    u4 alias = {0u, 0u, 0u, 0u};
    if (kind == ENV) {
        const uint sx = sv.env_w, sy = sv.env_h;
        const uint ipx = clampu(rnd.x / (0xFFFFFFFFu / sx), 0u, sx - 1u), ipy = clampu(rnd.y / (0xFFFFFFFFu / sy), 0u, sy - 1u);
        alias_i = (int)(ipx + ipy * sx);
        alias = *reinterpret_cast<const u4*>(sv.alias_table + alias_i);
    }
    L.valid = kind != NONE;
#define TR_F(x) __uint_as_float(x)
    RestirSample s = restir_null_sample();
    light_pdf = 1.0f;
    if (kind == POINT) {
        s.type = 0u; s.index = (uint)light_index;
        light_pdf = table_pdf * P.prob_point;
    } else if (kind == TRI) {
        s.type = 1u; s.index = (uint)light_index;
        const f3 A = F3(TR_F(L.r0.x), TR_F(L.r0.y), TR_F(L.r0.z)) - pos, B = F3(TR_F(L.r0.w), TR_F(L.r1.x), TR_F(L.r1.y)) - pos, C = F3(TR_F(L.r1.z), TR_F(L.r1.w), TR_F(L.r2.x)) - pos;
        float tri_pdf = 0.0f;
        const f3 out_dir = sample_triangle_light<RoundedMath>(1, F2(u.x, u.y), A, B, C, tri_pdf);
        const float out_length = ray_plane_intersection_dist(out_dir, A, B, C);
        if (isinf(tri_pdf) || tri_pdf <= 0 || out_length <= P.min_ray_dist || any_nan(out_dir)) tri_pdf = 1e9f;
        const f3 bary = get_barycentric_coords(out_dir * out_length, A, B, C);
        s.data = F2(bary.x, bary.y);
        light_pdf = (tri_pdf * table_pdf) * P.prob_tri;
    } else if (kind == DIR) {
        s.type = 2u; s.index = (uint)light_index;
        const float dir_cutoff = TR_F(L.r1.w);
        light_pdf = dir_cutoff >= 1.0f ? 1.0f : 1.0f / (2.0f * TR_PI * (1.0f - dir_cutoff));
        light_pdf = (light_pdf / (float)light_count) * P.prob_dir;
        s.data = F2(u.x, u.y);
    } else if (kind == ENV) {
        s.type = 3u; s.index = 0u;
        const uint sx = sv.env_w, sy = sv.env_h, pixel_count = sx * sy;
        int i = alias_i;
        light_pdf = TR_F(alias.z);
        if (rnd.z > alias.y) { i = (int)alias.x; light_pdf = TR_F(alias.w); }
        const int ppx = (int)((uint)i % sx), ppy = (int)((uint)i / sx);
        const f2 off = F2((float)(uint)(rnd.x * pixel_count), (float)(uint)(rnd.y * pixel_count)) * TR_INV_UINT32_MAX;
        s.data = (F2((float)ppx, (float)ppy) + off) / F2((float)sx, (float)sy);
        light_pdf = light_pdf * P.prob_env;
    }
#undef TR_F
    return s;
}

}  // namespace tr
