// dshgi_renderer's indirect light (shader/forward.frag:100-159, shader/spherical_harmonics.glsl:80-312, src/scene_stage.cc:1119-1131,
// src/scene.cc:163-211, src/sh_grid.cc:116-144, shader/ggx.glsl:69-72 restated): the per-grid parameters, the pinned order of operations of
// k_dshgi_indirect and k_brdf_integration (dshgi.hip) behind the entry points trhip_dshgi_* and trhip_brdf_integration_generate
// (include/trhip.h).  tests/dshgi_model.py repeats this file in float32 and float64, as the SH model repeats sh_probes.h.
//
// Layouts: a grid is the RGBA16F volume of sh_probes.h, [rz][ry * C][rx] entries of four halfs (8 bytes), coefficient l of probe (x, y, z)
// at (x, y + l * ry, z).  The BRDF-integration table is RG32F [h][w], texel (i, j) at j * w + i: i along cos_v, j along sqrt(roughness).
//
// Order of operations (plain fp32; every product, sum, quotient and square root is rounded on its own: the build has contraction off and
// the correctly rounded divide and square root; cos and pow are the C library's double functions of the float argument, rounded to float
// once (sh_cos, sh_pow of sh_probes.h); dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; M * v = (M[0] * v.x + M[1] * v.y) + M[2] * v.z,
// for a point + M[3] * 1.0f; normalize(a) = a / sqrtf(dot(a, a)) per component; R = the resolution, C = (order + 1)^2;
// clamp(x, lo, hi) = fminf(fmaxf(x, lo), hi), the C functions: a NaN x gives lo - GLSL leaves it undefined, this file defines it):
//   host         per grid, in float as glm computes them: q = quat_cast of the transform's upper 3 x 3 with its columns normalized
//                (orientation_quat, sh_probes.h);  qi = conjugate(q) / ((q.w * q.w + q.x * q.x) + (q.y * q.y + q.z * q.z));
//                normal_from_world = mat3_cast(qi);  pos_from_world = affineInverse(transform): Inv = inverse(mat3(transform)) by cofactors
//                times 1 / determinant, fourth column -(Inv * transform[3].xyz);  grid_clamp = 0.5f / float(R);  inv_grid_size = 1.0f / float(R)
//   surface      v, mat = shade_surface of the first hit (k_gbuffer's front half);  view = normalize(v.pos - ray origin)
//   grid space   sample_pos = pos_from_world * (v.pos, 1);  sample_normal = normalize(normal_from_world * v.smooth_normal);
//                sh_normal = normalize(normal_from_world * v.mapped_normal);
//                ref = view - v.mapped_normal * (2.0f * dot(v.mapped_normal, view));  sh_ref = normalize(normal_from_world * ref)
//   lobes        b = sh_basis(dir) (sh_probes.h);  cosine lobe: b[l] * (1.0f, 2.0f / 3.0f, 1.0f / 4.0f, 0.0f, -1.0f / 24.0f) by band;
//                GGX lobe at r = sqrtf(mat.roughness): b[l] * (1, zh[0], zh[1], zh[2], zh[3]) by band with, per band k,
//                zh[k] = ((A0[k] + A1[k] * cos(r * B1[k] + C1[k])) + A2[k] * cos(r * B2[k] + C2[k])) + r * ((1.0f / sqrtf(D[k] + r * r)) * E[k] + F[k])
//   trilinear    p = clamp(sample_pos * 0.5f + 0.5f, grid_clamp, 1.0f - grid_clamp);  c = p * float(R) - 0.5f;
//                lo = clamp(int(floorf(c)), 0, R - 1);  hi = min(lo + 1, R - 1);  f = c - float(lo);  per axis
//                w[k] = (wx * wy) * wz for corner k = ix + 2 iy + 4 iz, wx = ix ? f.x : 1.0f - f.x (wy, wz alike);
//                per coefficient l: t = the sum over k ascending, from 0, of texel_k[l].rgb * w[k] (eight texels, one fixed chain);
//                diffuse_sum += t * cosine[l];  reflection_sum += t * ggx[l]   (both start at 0, l ascending)
//                Deviation: Vulkan's sampler filters with 8-bit fixed-point weights; these are the fp32 fractions.
//   visibility   gp = sample_pos * 0.5f + 0.5f;  interp = clamp(gp * float(R) - 0.5f, 0.0f, float(R) - 1.0f);  fl = int(interp) (truncation);
//                lo = clamp(fl, 0, R - 1);  hi = clamp(fl + 1, 0, R - 1);  p_off = interp - float(lo);  m_off = 1.0f - p_off;
//                weight[k] = (ax * ay) * az, a = ix ? p_off : m_off (as above);  corner k at s = (ix ? hi.x : lo.x, ...);  per corner:
//                sample_dir = float(s) - interp;  sample_dist = sqrtf(dot(sample_dir, sample_dir));  sample_dir = sample_dir / sample_dist;
//                normal_factor = clamp((dot(sample_normal, sample_dir) + 1.0f) * 0.5f, 0.0f, 1.0f);
//                vd = -normalize(sample_dir * inv_grid_size);  visibility = sum over l ascending, from 0, of texel[l].w * sh_basis(vd)[l];
//                visibility_factor = clamp((visibility - sample_dist) + 0.4f, 0.0f, 1.0f);  wk = (weight[k] * visibility_factor) * normal_factor;
//                sum_weight += wk (from 0, k ascending);  inv_weight = sum_weight > 0.0f ? 1.0f / sum_weight : 0.0f;
//                per coefficient l: t = (sum over k ascending, from 0, of texel_k[l].rgb * wk) * inv_weight;  the sums as in the trilinear branch.
//                A shading point exactly on a probe has sample_dist = 0 and sample_dir = 0 / 0 = NaN there: both factors clamp to 0 and
//                the corner's weight is 0 (every corner of an axis of resolution 1 is such a corner when the point lies in the probe's
//                plane).  All weights 0: the probe is 0, not NaN.  A corner's texels are read twice (once for .w, once weighted) rather
//                than held: the kernel stays at the trilinear branch's registers.
//   incoming     incoming_diffuse = max(diffuse_sum, 0);  incoming_reflection = max(reflection_sum, 0)
//   brdf         cos_v = max(dot(v.mapped_normal, -view), 0.0f);  fresnel = f0 + (max(1.0f - roughness, f0) - f0) * pow(1.0f - cos_v, 5.0f);
//                kd = ((1.0f - fresnel) * (1.0f - metallic)) * (1.0f - transmittance);
//                table: u = clamp(cos_v * float(w) - 0.5f, 0.0f, float(w) - 1.0f);  i0 = clamp(int(floorf(u)), 0, w - 1);  i1 = min(i0 + 1, w - 1);
//                fu = u - float(i0);  the same along j with r * float(h);  bi = (t00 * (1.0f - fu) + t10 * fu) * (1.0f - fv) + (t01 * (1.0f - fu) + t11 * fu) * fv;
//                diffuse = incoming_diffuse * kd;  reflection = incoming_reflection * mix(fresnel * bi.x + bi.y, 1.0f, metallic)
//   colour       indirect = diffuse * albedo * (1.0f - metallic) + reflection * mix(vec3(0.02f), albedo, metallic) / mix(0.02f, 1.0f, metallic)
//                (modulate_color as sample_color of resolve_kernel.h writes it, no emission term);  a miss or an instance without a grid: 0;
//                out.rgb = direct.rgb + indirect, one add per channel;  out.a = direct.a
//
// The BRDF-integration table (the reference loads data/brdf_integration.exr; the generator evaluates the split sum this project's GGX terms
// define).  Cell (i, j) of a size x size table, N samples:
//   cos_v = (float(i) + 0.5f) / float(size);  pr = (float(j) + 0.5f) / float(size);  a = pr * pr;  V = (sqrtf(1.0f - cos_v * cos_v), 0, cos_v)
//   sample s: u1 = (float(s) + 0.5f) / float(N);  u2 = float(bit-reversed s) * 2^-32 (Hammersley);  phi = (2.0f * pi_f) * u1;
//             ct = sqrtf((1.0f - u2) / (1.0f + (a * a - 1.0f) * u2));  st = sqrtf(1.0f - ct * ct);  H = (st * cos(phi), st * sin(phi), ct):
//             the half vector drawn with density ggx_distribution(H.z, a) * H.z (shading.h), which therefore cancels from the estimate;
//             vh = dot(V, H);  L = H * (2.0f * vh) - V;  a sample with L.z <= 0 or vh <= 0 adds nothing;  otherwise
//             g = ggx_masking_shadowing(V.z, vh, L.z, dot(L, H), a) (shading.h);  gv = (g * vh) / (H.z * V.z);  fc = pow(1.0f - vh, 5.0f);
//             scale += (1.0f - fc) * gv;  bias += fc * gv   (both from 0, s ascending, one thread per cell)
//   texel = (scale / float(N), bias / float(N))
#pragma once
#include "common.h"
#include "sh_probes.h"

namespace tr {

struct DshgiGrid {                       // sh_grid_buffer of src/scene_stage.cc:1119-1131 and the grid's texture
    const void* texels;                  // RGBA16F, 8 bytes an entry
    m4 pos_from_world;
    m3 normal_from_world;
    int res[3];
    f3 grid_clamp, inv_grid_size;
};

struct DshgiSurface {                    // trhip_dshgi_surface: the record k_dshgi_indirect shaded a pixel with
    f3 pos, smooth_normal, mapped_normal, view;
    f4 albedo;
    float metallic, roughness, f0, transmittance;
    int grid, instance_id;
};

// The lookup's loops are unrolled (the lobes are indexed by constants and stay in registers); left alone, the compiler issues every texel
// read of the lookup first and holds them all - 8 C reads of two registers each.  A fence ends a group: the reads behind it are not
// issued before the sums in front of it are done (the register table of DESIGN.md section 20).
#define DSH_FENCE(a, b) asm volatile("" : "+v"(a), "+v"(b) : : "memory")
constexpr int DSH_GROUP = 3;             // coefficients of a group: 24 texel reads in flight

typedef const unsigned long long __attribute__((address_space(1)))* DshTexels;      // an entry as one 8-byte word; the grids' images are device allocations: global, not flat, loads
typedef const unsigned short __attribute__((address_space(1)))* DshHalfs;

TR_DEV float dsh_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
TR_DEV f3 dsh_mul(const m3& m, f3 v) { return (m.c[0] * v.x + m.c[1] * v.y) + m.c[2] * v.z; }
TR_DEV f3 dsh_point(const m4& m, f3 p) { return F3(((m.c[0] * p.x + m.c[1] * p.y) + m.c[2] * p.z) + m.c[3] * 1.0f); }
TR_DEV float dsh_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
TR_DEV f3 dsh_normalize(f3 a) { const float l = sqrtf(dsh_dot(a, a)); return F3(a.x / l, a.y / l, a.z / l); }

TR_DEV f3 half4_rgb(unsigned long long t) {
    return F3(__half2float(__ushort_as_half((unsigned short)(t & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)((t >> 16) & 0xFFFFu))),
              __half2float(__ushort_as_half((unsigned short)((t >> 32) & 0xFFFFu))));
}

// get_sh_cosine_lobe and get_ggx_specular_lobe (spherical_harmonics.glsl:80-192): the factor of a band
template <int ORDER>
TR_DEV void dsh_band_scale(float* lobe, const float* band) {
#pragma unroll
    for (int b = 1, l = 1; b <= ORDER; ++b)
#pragma unroll
        for (int m = 0; m < 2 * b + 1; ++m, ++l) lobe[l] = lobe[l] * band[b];
}
template <int ORDER>
TR_DEV void dsh_cosine_lobe(f3 dir, float* lobe) {
    sh_basis<ORDER>(dir, lobe);
    const float band[5] = {1.0f, 2.0f / 3.0f, 1.0f / 4.0f, 0.0f, -1.0f / 24.0f};
    dsh_band_scale<ORDER>(lobe, band);
}
TR_DEV float dsh_zh(float r, float a0, float a1, float b1, float c1, float a2, float b2, float c2, float d, float e, float f) {
    return ((a0 + a1 * sh_cos(r * b1 + c1)) + a2 * sh_cos(r * b2 + c2)) + r * ((1.0f / sqrtf(d + r * r)) * e + f);
}
template <int ORDER>
TR_DEV void dsh_ggx_lobe(f3 dir, float r, float* lobe) {
    sh_basis<ORDER>(dir, lobe);
    float band[5] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (ORDER >= 1) band[1] = dsh_zh(r, 0.27793123f, 0.905501229f, 2.49220829f, 2.88755638f, 1.98743320f, 1.79537159f, 0.636261278f, 0.329615862f, 1.54054310f, -4.73179141e-04f);
    if (ORDER >= 2) band[2] = dsh_zh(r, 0.59372022f, 10.57518269f, 3.49132073f, 0.56672964f, 9.52855312f, 3.58608449f, 3.60689811f, 0.29109984f, 4.35171889f, -3.58678416f);
    if (ORDER >= 3) band[3] = dsh_zh(r, 0.2400839f, 21.6480923f, 3.92510137f, 0.50116945f, 19.90690569f, 4.01505002f, 3.55551139f, 0.25094573f, 7.58146856f, -6.47567145f);
    if (ORDER >= 4) band[4] = dsh_zh(r, 0.000250700498f, 5.53340572f, 3.98902127f, 0.705097221f, 3.23348085f, 4.63841986f, 3.25144230f, 0.211655471f, 9.84410536f, -8.76804538f);
    dsh_band_scale<ORDER>(lobe, band);
}

// Entry of coefficient 0 of probe (x, y, z), inside the volume for 0 <= x, y, z < R; coefficient l lies l * dsh_coef_stride entries further.
template <int ORDER>
TR_DEV size_t dsh_entry(const DshgiGrid& G, int x, int y, int z) {
    constexpr int C = (ORDER + 1) * (ORDER + 1);
    return ((size_t)z * ((size_t)G.res[1] * C) + (size_t)y) * (size_t)G.res[0] + (size_t)x;
}
TR_DEV size_t dsh_coef_stride(const DshgiGrid& G) { return (size_t)G.res[1] * (size_t)G.res[0]; }

// sample_sh_grid + calc_sh_irradiance + calc_sh_ggx_specular (spherical_harmonics.glsl:203-312) without holding an sh_probe
template <int ORDER, bool VISIBILITY>
TR_DEV void dsh_sample_grid(const DshgiGrid& G, f3 sample_pos, f3 sample_normal, const float* cosine, const float* ggx, f3& incoming_diffuse,
                            f3& incoming_reflection) {
    constexpr int C = (ORDER + 1) * (ORDER + 1);
    const f3 R = F3((float)G.res[0], (float)G.res[1], (float)G.res[2]);
    const f3 gp = sample_pos * 0.5f + 0.5f;
    const size_t stride = dsh_coef_stride(G);
    int lo[3], hi[3];
    float w[8], inv_weight = 1.0f;
    if (!VISIBILITY) {
        f3 f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float gc = comp(G.grid_clamp, a), r = comp(R, a);
            const float p = dsh_clamp(comp(gp, a), gc, 1.0f - gc);
            const float c = p * r - 0.5f;
            lo[a] = clampi((int)floorf(c), 0, G.res[a] - 1);
            hi[a] = lo[a] + 1 < G.res[a] - 1 ? lo[a] + 1 : G.res[a] - 1;
            const float fr = c - (float)lo[a];
            if (a == 0) f.x = fr; else if (a == 1) f.y = fr; else f.z = fr;
        }
        const f3 m = F3(1.0f - f.x, 1.0f - f.y, 1.0f - f.z);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = (((k & 1) ? f.x : m.x) * ((k & 2) ? f.y : m.y)) * ((k & 4) ? f.z : m.z);
    } else {
        const f3 voxel = gp * R - 0.5f;
        const f3 interp = F3(dsh_clamp(voxel.x, 0.0f, R.x - 1.0f), dsh_clamp(voxel.y, 0.0f, R.y - 1.0f), dsh_clamp(voxel.z, 0.0f, R.z - 1.0f));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int fl = (int)comp(interp, a);
            lo[a] = clampi(fl, 0, G.res[a] - 1);
            hi[a] = clampi(fl + 1, 0, G.res[a] - 1);
        }
        const f3 p_off = interp - F3((float)lo[0], (float)lo[1], (float)lo[2]);
        const f3 m_off = F3(1.0f - p_off.x, 1.0f - p_off.y, 1.0f - p_off.z);
        float sum_weight = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int sx = (k & 1) ? hi[0] : lo[0], sy = (k & 2) ? hi[1] : lo[1], sz = (k & 4) ? hi[2] : lo[2];
            const float weight = (((k & 1) ? p_off.x : m_off.x) * ((k & 2) ? p_off.y : m_off.y)) * ((k & 4) ? p_off.z : m_off.z);
            f3 sample_dir = F3((float)sx, (float)sy, (float)sz) - interp;
            const float sample_dist = sqrtf(dsh_dot(sample_dir, sample_dir));
            sample_dir = F3(sample_dir.x / sample_dist, sample_dir.y / sample_dist, sample_dir.z / sample_dist);
            const float normal_factor = dsh_clamp((dsh_dot(sample_normal, sample_dir) + 1.0f) * 0.5f, 0.0f, 1.0f);
            const f3 vd = -dsh_normalize(sample_dir * G.inv_grid_size);
            float basis[C];
            sh_basis<ORDER>(vd, basis);
            const DshHalfs corner = (DshHalfs)((DshTexels)G.texels + dsh_entry<ORDER>(G, sx, sy, sz)) + 3;      // .w alone: a register a read
            float visibility = 0.0f;
#pragma unroll
            for (int l = 0; l < C; ++l) {
                visibility = visibility + __half2float(__ushort_as_half(corner[l * stride * 4])) * basis[l];
                if (l % 8 == 7) DSH_FENCE(visibility, sum_weight);
            }
            const float visibility_factor = dsh_clamp((visibility - sample_dist) + 0.4f, 0.0f, 1.0f);
            w[k] = (weight * visibility_factor) * normal_factor;
            sum_weight = sum_weight + w[k];
            DSH_FENCE(sum_weight, w[k]);
        }
        inv_weight = sum_weight > 0.0f ? 1.0f / sum_weight : 0.0f;
    }
    DshTexels corner[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) corner[k] = (DshTexels)G.texels + dsh_entry<ORDER>(G, (k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]);
    f3 diffuse = F3(0.0f), reflection = F3(0.0f);
#pragma unroll
    for (int l = 0; l < C; ++l) {
        f3 t = F3(0.0f);
#pragma unroll
        for (int k = 0; k < 8; ++k) t = t + half4_rgb(corner[k][l * stride]) * w[k];
        if (VISIBILITY) t = t * inv_weight;
        diffuse = diffuse + t * cosine[l];
        reflection = reflection + t * ggx[l];
        if (l % DSH_GROUP == DSH_GROUP - 1) { DSH_FENCE(diffuse.x, reflection.x); DSH_FENCE(diffuse.y, reflection.y); DSH_FENCE(diffuse.z, reflection.z); }
    }
    incoming_diffuse = max3(diffuse, F3(0.0f));
    incoming_reflection = max3(reflection, F3(0.0f));
}

// texture(brdf_integration, vec2(cos_v, r)).xy: bilinear, clamp to edge
TR_DEV f2 dsh_brdf_integration(const f2* table, int w, int h, float cos_v, float r) {
    const float u = dsh_clamp(cos_v * (float)w - 0.5f, 0.0f, (float)w - 1.0f), v = dsh_clamp(r * (float)h - 0.5f, 0.0f, (float)h - 1.0f);
    const int i0 = clampi((int)floorf(u), 0, w - 1), j0 = clampi((int)floorf(v), 0, h - 1);
    const int i1 = i0 + 1 < w - 1 ? i0 + 1 : w - 1, j1 = j0 + 1 < h - 1 ? j0 + 1 : h - 1;
    const float fu = u - (float)i0, fv = v - (float)j0;
    const f2 t00 = table[(size_t)j0 * w + i0], t10 = table[(size_t)j0 * w + i1], t01 = table[(size_t)j1 * w + i0], t11 = table[(size_t)j1 * w + i1];
    return (t00 * (1.0f - fu) + t10 * fu) * (1.0f - fv) + (t01 * (1.0f - fu) + t11 * fu) * fv;
}

// eval_indirect_light + brdf_indirect + modulate_color (forward.frag:100-159, material.glsl:57-65) of a surface record with a grid
template <int ORDER, bool VISIBILITY>
TR_DEV f3 dsh_indirect(const DshgiGrid& G, const DshgiSurface& s, const f2* table, int table_w, int table_h) {
    constexpr int C = (ORDER + 1) * (ORDER + 1);
    const f3 sample_pos = dsh_point(G.pos_from_world, s.pos);
    const f3 sample_normal = dsh_normalize(dsh_mul(G.normal_from_world, s.smooth_normal));
    const f3 sh_normal = dsh_normalize(dsh_mul(G.normal_from_world, s.mapped_normal));
    const f3 ref = s.view - s.mapped_normal * (2.0f * dsh_dot(s.mapped_normal, s.view));
    const f3 sh_ref = dsh_normalize(dsh_mul(G.normal_from_world, ref));
    const float r = sqrtf(s.roughness);
    float cosine[C], ggx[C];
    dsh_cosine_lobe<ORDER>(sh_normal, cosine);
    dsh_ggx_lobe<ORDER>(sh_ref, r, ggx);
    f3 incoming_diffuse, incoming_reflection;
    dsh_sample_grid<ORDER, VISIBILITY>(G, sample_pos, sample_normal, cosine, ggx, incoming_diffuse, incoming_reflection);
    const float cos_v = fmax2(dsh_dot(s.mapped_normal, -s.view), 0.0f);
    const float fresnel = s.f0 + (fmax2(1.0f - s.roughness, s.f0) - s.f0) * sh_pow(1.0f - cos_v, 5.0f);
    const float kd = ((1.0f - fresnel) * (1.0f - s.metallic)) * (1.0f - s.transmittance);
    const f2 bi = dsh_brdf_integration(table, table_w, table_h, cos_v, r);
    const f3 diffuse = incoming_diffuse * kd;
    const f3 reflection = incoming_reflection * mixf(fresnel * bi.x + bi.y, 1.0f, s.metallic);
    const f3 albedo = F3(s.albedo);
    const float approx_fresnel = 0.02f;
    return diffuse * albedo * (1.0f - s.metallic) + reflection * mix3(F3(approx_fresnel), albedo, s.metallic) / mixf(approx_fresnel, 1.0f, s.metallic);
}

}  // namespace tr
