// ReSTIR DI's sphere lights as area lights (restir_di.h `sphere lights`; trhip_restir_di_set_sphere_lights): what
// restir_di.hip and restir_di_sphere.hip share.  The area mode's kernels - k_restir_di_canonical_sphere and k_restir_di_spatial_sphere,
// written over RestirDiKindT<true> - are a translation unit of their own and repeat the point mode's kernels instead of sharing a body
// with them, for the reason restir_di_power.h gives, so that every point instance stays the code it was.  Both passes take
// RestirBsdfParams, the widest block: one canonical kernel serves the uniform and the power selection, with and without BSDF candidates.
#pragma once
#include "restir_di_bsdf.h"

namespace tr {

using RestirDiSphereKind = RestirDiKindT<true>;

using RestirSphereKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, RestirBsdfParams, uint*);
RestirSphereKernel restir_di_sphere_canonical_kernel(bool two_level, bool temporal, int visibility, bool power, bool bsdf);      // restir_di_sphere.hip
RestirSphereKernel restir_di_sphere_spatial_kernel(bool two_level, uint32_t spatial, int visibility);

// `sphere lights` 2: behind restir_sample_canonical or restir_sample_canonical_power.  A type-0 sample whose light has a radius becomes
// a point of the cone the sphere subtends at pos, as sample_point_light (shading.h) draws it; L is the record the sampler fetched, rnd
// its draw, light_pdf the pdf of the index on entry and of the point on return.  Any other sample is left as it is.
template <class Params>
TR_DEV void restir_sphere_draw(const Params& P, u4 rnd, f3 pos, const RestirLightRecord& L, RestirSample& s, float& light_pdf) {
#define TR_F(x) __uint_as_float(x)
    if (!L.valid || s.type != 0u) return;
    const float r = TR_F(L.r2.y);
    if (r != 0.0f) {
        const f4 u = u4_to_unit(rnd);
        const f3 light_pos = F3(TR_F(L.r1.z), TR_F(L.r1.w), TR_F(L.r2.x));
        const f3 d = pos - light_pos;
        const float dist2 = dot(d, d);
        const float k = 1.0f - r * r / dist2;
        const float cutoff = k > 0 ? sqrtf(k) : -1.0f;
        const f3 dir = sample_cone<RoundedMath>(F2(u.y, u.z), -normalize(d), cutoff);
        const float b = dot(d, dir);
        const float len = -b - sqrtf(fmax2(b * b - dist2 + r * r, 0.0f));
        const f3 x = pos + dir * len;
        const f3 n = normalize(x - light_pos);
        s.data = restir_oct_encode(n);
        float solid_pdf = 1.0f / (2.0f * TR_PI * (1.0f - cutoff));
        if (any_nan(n) || len <= P.min_ray_dist) solid_pdf = 1e9f;
        light_pdf = light_pdf * solid_pdf;
    }
#undef TR_F
}

}  // namespace tr
