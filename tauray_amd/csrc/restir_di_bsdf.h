// ReSTIR DI's BSDF-sampled candidates (restir_di.h `bsdf candidates`; trhip_restir_di_set_bsdf_candidates): what
// restir_di.hip and restir_di_bsdf.hip share.  k_restir_di_canonical_bsdf is a translation unit of its own and repeats
// k_restir_di_canonical around a second candidate loop instead of sharing a body with it, for the reason restir_di_power.h gives: the
// inliner weighs a function by its callers in the unit, and a body shared through a function changes register allocation (DESIGN.md
// section 30).  It has a parameter block of its own; RestirParams and RestirPowerParams keep their layouts.  The spatial kernel never
// sees a candidate's pdf: a frame with BSDF candidates launches the spatial instances every other frame launches.
#pragma once
#include "restir_di_power.h"

namespace tr {

struct alignas(16) RestirBsdfRecord {    // trhip_restir_di_bsdf_candidate, [pixel][L + B] next to the candidate records
    uint technique;                      // 0: a light candidate, 1: a BSDF candidate
    f3 dir;                              // light: the contribution's direction; BSDF: the traced one (0 when the sampler gave none)
    float p_b;
    int instance_id, primitive_id;       // the BSDF ray's hit; instance -1 and t -1: a miss, nothing traced, or a light candidate
    float u, v, t;
    float denom; uint traced;            // 1: the closest-hit ray was cast
};
static_assert(sizeof(RestirBsdfRecord) == 48, "layout");

// RestirPowerParams' fields and two more.  light_table is read by the POWER instances only.
struct RestirBsdfParams {
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
    RestirCandidateRecord* rec_candidates;      // [pixel][candidates + bsdf_candidates]; null unless options.record, as the six below
    RestirTemporalRecord* rec_temporal;
    RestirSpatialRecord* rec_spatial;
    RestirFinalRecord* rec_final;
    RestirSampledRecord* rec_sampled;
    const AliasEntry* light_table;
    int bsdf_candidates;
    RestirBsdfRecord* rec_bsdf;                 // [pixel][candidates + bsdf_candidates]
};

using RestirBsdfKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, RestirBsdfParams, uint*);
RestirBsdfKernel restir_di_bsdf_canonical_kernel(bool two_level, bool temporal, int visibility, bool power);      // restir_di_bsdf.hip

// What the canonical kernels with BSDF candidates share (restir_di_bsdf.hip, and restir_di_sphere.hip's BSDF instances)
// `bsdf candidates` 3: p_b of a world direction at a surface
TR_DEV float restir_bsdf_pdf(const RestirDomain& dom, const m3& tbn, f3 shading_view, f3 dir) {
    Lobes lobes = {0, 0, 0, 0};
    return ggx_bsdf_pdf<RoundedMath>(mulT(dir, tbn), shading_view, dom.mat, lobes);
}

// `bsdf candidates` 9
TR_DEV float restir_balance_weight(float mis_weight, float target, float denom) {
    float weight = (mis_weight * target) / denom;
    if (isnan(weight) || !(denom > 0.0f)) weight = 0.0f;
    return weight;
}

TR_DEV void restir_write_candidate(const RestirBsdfParams& P, size_t slot, const RestirSample& s, float p_l, f3 contrib, float visibility, float weight, float u, bool selected,
                                   uint technique, f3 dir, float p_b, const HitRecord& hit, bool traced, float denom) {
    RestirCandidateRecord* rec = P.rec_candidates + slot;
    restir_set_word(rec, 0, u4{s.type << 30 | s.index, TR_U(s.data.x), TR_U(s.data.y), TR_U(p_l)});
    restir_set_word(rec, 1, u4{TR_U(contrib.x), TR_U(contrib.y), TR_U(contrib.z), TR_U(visibility)});
    restir_set_word(rec, 2, u4{TR_U(weight), TR_U(u), selected ? 1u : 0u, 0u});
    RestirBsdfRecord* brec = P.rec_bsdf + slot;
    restir_set_word(brec, 0, u4{technique, TR_U(dir.x), TR_U(dir.y), TR_U(dir.z)});
    restir_set_word(brec, 1, u4{TR_U(p_b), (uint)hit.instance_id, (uint)hit.primitive_id, TR_U(hit.u)});
    restir_set_word(brec, 2, u4{TR_U(hit.v), TR_U(hit.t), TR_U(denom), traced ? 1u : 0u});
}

// `bsdf candidates` 5: the lat-long uv of a direction, the inverse of uv_to_latlong_direction, with atan2 alone
template <class M>
TR_DEV f2 restir_latlong_uv(f3 dir) {
    f2 uv;
    uv.x = M::atan2(dir.z, dir.x) / (2.0f * TR_PI) + 0.5f;
    uv.y = M::atan2(-dir.y, sqrtf(dir.x * dir.x + dir.z * dir.z)) / TR_PI + 0.5f;
    return uv;
}

// `bsdf candidates` 5: what a closest-hit ray along `dir` found, as a light sample.  traced: the ray was cast.
TR_DEV RestirSample restir_sample_of_hit(const SceneView& sv, bool traced, const HitRecord& hit, f3 dir) {
    RestirSample s = restir_null_sample();
    if (traced && hit.instance_id >= 0) {
        const int base = sv.instances[hit.instance_id].light_base_id;
        const uint index = (uint)base + (uint)hit.primitive_id;
        // light_data.x weighs pos[0] and .y pos[1] (restir_contribution); a hit's (u, v) weigh vertices 1 and 2 (shade_surface)
        if (base >= 0 && index < sv.tri_light_count) { s.type = 1u; s.index = index; s.data = F2(1.0f - hit.u - hit.v, hit.u); }
    } else if (traced && sv.environment_proj >= 0) {
        s.type = 3u; s.index = 0u; s.data = restir_latlong_uv<RoundedMath>(dir);
    }
    return s;
}

// `bsdf candidates` 7: the pdf with which the light technique produces the identity of a triangle or environment sample, from the
// identity, its fetched record and the contribution's direction alone.  POWER: the triangle's share is the table's, else 1 / n_tri.
template <bool POWER, class Params>
TR_DEV float restir_identity_light_pdf(const SceneView& sv, const Params& P, const RestirSample& s, const RestirLightRecord& L, f3 pos, f3 dir) {
#define TR_F(x) __uint_as_float(x)
    float p_l = 0.0f;
    if (!L.valid) return p_l;
    // a class whose probability is 0 gives 0, and its table is not read
    if (s.type == 1u && P.prob_tri > 0.0f) {
        const f3 A = F3(TR_F(L.r0.x), TR_F(L.r0.y), TR_F(L.r0.z)) - pos, B = F3(TR_F(L.r0.w), TR_F(L.r1.x), TR_F(L.r1.y)) - pos, C = F3(TR_F(L.r1.z), TR_F(L.r1.w), TR_F(L.r2.x)) - pos;
        // sample_spherical_triangle's solid angle, operation for operation
        const f3 nA = normalize(A), nB = normalize(B), nC = normalize(C);
        const float dAB = dot(nA, nB), dBC = dot(nB, nC), dAC = dot(nA, nC);
        const float div = 1.0f / sqrtf(2.0f * fabsf(nB.x) + 2.0f);
        const float e = nB.x > 0 ? div : -div;
        const f3 h = nB * div + F3(e, 0, 0);
        const f3 a = nA - 2.0f * h * (dAB * div + e * nA.x);
        const f3 c = nC - 2.0f * h * (dBC * div + e * nC.x);
        const float G0 = fabsf(a.y * c.z - c.y * a.z);
        const float G1 = dAC + dBC;
        const float G2 = 1.0f + dAB;
        const float solid_angle = 2.0f * RoundedMath::atan2(G0, G1 + G2);
        float tri_pdf = 1.0f / solid_angle;
        const float out_length = ray_plane_intersection_dist(dir, A, B, C);
        if (isinf(tri_pdf) || tri_pdf <= 0 || out_length <= P.min_ray_dist || any_nan(dir)) tri_pdf = 1e9f;
        float sel = 1.0f / (float)(int)sv.tri_light_count;
        if constexpr (POWER) sel = P.light_table[sv.point_light_count + s.index].pdf;
        p_l = (tri_pdf * sel) * P.prob_tri;
    } else if (s.type == 3u && P.prob_env > 0.0f) {
        const uint sx = sv.env_w, sy = sv.env_h;
        const int ipx = clampi((int)floorf(s.data.x * (float)sx), 0, (int)sx - 1), ipy = clampi((int)floorf(s.data.y * (float)sy), 0, (int)sy - 1);
        p_l = sv.alias_table[(uint)ipx + (uint)ipy * sx].pdf * P.prob_env;
    }
#undef TR_F
    return p_l;
}

}  // namespace tr
