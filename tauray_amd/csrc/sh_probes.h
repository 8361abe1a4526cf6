// sh_path_tracer_stage + sh_compact_stage (src/sh_path_tracer_stage.{hh,cc}, shader/sh_path_tracer.rgen, shader/sh_compact.comp restated):
// the grid parameters, the path ids of a batch and the pinned order of operations of k_sh_raygen and k_sh_project (sh_probes.hip) behind the
// entry points trhip_sh_* (include/trhip.h).  tests/sh_probes_model.py repeats this file in float32, as the TAA model repeats taa.h.
//
// Layouts: grid RGBA32F [rz][ry * C][rx], coefficient l of probe (x, y, z) at (x, y + l * ry, z); grid_half the same entries as four halfs.
// A probe's linear index is p = x + rx * (y + ry * z).  A batch is a run of whole probes [probe_base, probe_base + n_probes) with
// n_probes * N paths; path `id` of a batch is (probe q, sample s) with id = q * N + s (probe-major, the default) or
// id = s * n_probes + q (sample-major, TR_SH_SAMPLE_MAJOR = 1).  A path's state depends on (x, y, z, s) alone, so the grids do not depend on the order or on the batches.
//
// Order of operations (plain fp32; every product, sum, quotient and square root is rounded on its own: the build has contraction off and
// the correctly rounded divide and square root; sin, cos and pow are the C library's double functions of the float argument, rounded to
// float once; N = samples_per_probe, R = the resolution, C = (order + 1)^2):
//   host         sample_counter = frame_counter * N (uint32, wrapping);  rotation_x = float(pcg(sample_counter)) / float(0xFFFFFFFFu);
//                rotation_y = float(pcg(sample_counter + 1)) / float(0xFFFFFFFFu);  cell_scale = (0.5f * float(R)) / scaling per axis;
//                normal_transform = mat3_cast(quat_cast(columns of the transform's upper 3 x 3, each normalized)) as glm computes them;
//                history_length += 1;  mix_ratio = max(1.0f / float(history_length), temporal_ratio);  coef_mult = (4.0f * pi_f) / float(N)
//   sampler      ls = init_local_sampler(uvec4(x, y, z, s)): coord.w += sample_counter, coord.z += rng_seed (pcg(seed) if seed != 0)
//   offset       point film: 0.  Otherwise u = float(pcg4d(ls.rs)) * 2^-32 per component (xyz);  box: u * 2.0f - 1.0f;
//                Blackman-Harris: sample_sphere(u.xy) * pow(abs(2.0f * sample_blackman_harris(u.z) - 1.0f), 1.0f / 3.0f)
//   position     local = (((float(p) + offset * film_radius) + 0.5f) / float(R)) * 2.0f - 1.0f per axis;
//                global = ((T[0] * local.x + T[1] * local.y) + T[2] * local.z) + T[3] * 1.0f   (columns of the transform)
//   direction    o = (float(s) + rotation_x) * 0.38196601125f;  u = (float(s) + rotation_y) / float(N);
//                cos_theta = 2.0f * u - 1.0f;  sin_theta = sqrtf(1.0f - cos_theta * cos_theta);  phi = (o * 2.0f) * pi_f;
//                local_dir = (cos(phi) * sin_theta, sin(phi) * sin_theta, cos_theta);
//                global_dir = normalize((Nt[0] * local_dir.x + Nt[1] * local_dir.y) + Nt[2] * local_dir.z)
//   seed         payload seed = pcg4d(ls.rs).x, after the offset's draw
//   value        (bounce loop: k_trace_* and k_shade with hide_lights and the first-bounce clamp)  approx_fresnel = 0.02f;
//                dd = diffuse.rgb * albedo * (1.0f - metallic);
//                rr = reflection.rgb * (approx_fresnel * (1.0f - metallic) + albedo * metallic) / (approx_fresnel * (1.0f - metallic) + 1.0f * metallic);
//                value = dd + rr
//   distance     dist = clamp(first_dist * length(local_dir * cell_scale), 0.0f, sqrtf(3.0f)); first_dist = length(first hit - origin), 0 on a miss
//   projection   coefs = (value, dist) * coef_mult;  term[l] = coefs * sh_basis(local_dir)[l] (sh_basis below, as written, left to right)
//   sum          thread t of SH_BLOCK = 256 adds the terms of samples t, t + 256, t + 512, ... in that order to 0;
//                then six butterfly steps inside each wave of 64, v = v + v[lane ^ off] for off = 32, 16, 8, 4, 2, 1;
//                then the four waves as (w0 + w1) + (w2 + w3)
//   blend        mix_ratio < 1: out = previous * (1.0f - mix_ratio) + new * mix_ratio; otherwise out = new (previous is not read)
//   half         __float2half_rn of out, per component
#pragma once
#include "common.h"

#ifndef TR_SH_SAMPLE_MAJOR
#define TR_SH_SAMPLE_MAJOR 0     // probe-major: the faster of the two on the device, by k_sh_project's reads (profiles/r16/sh_probes.txt)
#endif

namespace tr {

constexpr int SH_BLOCK = 256;                        // threads of a k_sh_project workgroup (one probe)
constexpr int SH_MAX_ORDER = 4;
constexpr int SH_MAX_COEFS = (SH_MAX_ORDER + 1) * (SH_MAX_ORDER + 1);
constexpr uint32_t SH_MAX_BATCH_PATHS = 1920u * 1080u;   // the frame the lane schedule of PtStage::render was tuned on
constexpr float SH_PI = 3.14159265358979323846f;
constexpr float SH_GOLDEN = 0.38196601125f;

struct ShGridData {                                  // grid_data_buffer of src/sh_path_tracer_stage.cc:10-19
    m4 transform;
    m3 normal_transform;
    uint grid_size[3];
    float mix_ratio;
    f3 cell_scale;
    float rotation_x, rotation_y;
};

struct ShProbeBatch {                                // what PtStage::render traces for a probe stage instead of a camera's pixels
    ShGridData grid;
    uint samples;                                    // N
    uint sample_counter, rng_seed;                   // of init_local_sampler
    uint probe_base, n_probes;
    uint n_paths() const { return n_probes * samples; }
};

TR_HD void sh_path_of_id(const ShProbeBatch& b, uint id, uint& q, uint& s) {
#if TR_SH_SAMPLE_MAJOR
    s = id / b.n_probes; q = id - s * b.n_probes;
#else
    q = id / b.samples; s = id - q * b.samples;
#endif
}
TR_HD uint sh_id_of_path(const ShProbeBatch& b, uint q, uint s) {
#if TR_SH_SAMPLE_MAJOR
    return s * b.n_probes + q;
#else
    return q * b.samples + s;
#endif
}

// The orientation of a transform as the reference's host computes it (get_matrix_orientation, src/math.cc:44-52): glm::quat_cast of the
// columns normalized, (x, y, z, w); and glm::mat3_cast of a quaternion.  In float like the reference's host.  Host only.
inline f4 orientation_quat(const m4& t) {
    float m[3][3];      // m[column][row]
    for (int c = 0; c < 3; ++c) {
        const f4 v = t.c[c];
        const float len = sqrtf(((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w);      // glm::normalize of the vec4 column
        m[c][0] = v.x / len; m[c][1] = v.y / len; m[c][2] = v.z / len;
    }
    const float fx = m[0][0] - m[1][1] - m[2][2], fy = m[1][1] - m[0][0] - m[2][2], fz = m[2][2] - m[0][0] - m[1][1], fw = m[0][0] + m[1][1] + m[2][2];
    int big = 0;
    float fbig = fw;
    if (fx > fbig) { fbig = fx; big = 1; }
    if (fy > fbig) { fbig = fy; big = 2; }
    if (fz > fbig) { fbig = fz; big = 3; }
    const float bv = sqrtf(fbig + 1.0f) * 0.5f, mult = 0.25f / bv;
    float qw, qx, qy, qz;
    switch (big) {
        case 0: qw = bv; qx = (m[1][2] - m[2][1]) * mult; qy = (m[2][0] - m[0][2]) * mult; qz = (m[0][1] - m[1][0]) * mult; break;
        case 1: qw = (m[1][2] - m[2][1]) * mult; qx = bv; qy = (m[0][1] + m[1][0]) * mult; qz = (m[2][0] + m[0][2]) * mult; break;
        case 2: qw = (m[2][0] - m[0][2]) * mult; qx = (m[0][1] + m[1][0]) * mult; qy = bv; qz = (m[1][2] + m[2][1]) * mult; break;
        default: qw = (m[0][1] - m[1][0]) * mult; qx = (m[2][0] + m[0][2]) * mult; qy = (m[1][2] + m[2][1]) * mult; qz = bv; break;
    }
    return F4(qx, qy, qz, qw);
}
inline m3 mat3_of_quat(f4 q) {
    const float qx = q.x, qy = q.y, qz = q.z, qw = q.w;
    const float qxx = qx * qx, qyy = qy * qy, qzz = qz * qz, qxz = qx * qz, qxy = qx * qy, qyz = qy * qz, qwx = qw * qx, qwy = qw * qy, qwz = qw * qz;
    m3 r;
    r.c[0] = F3(1.0f - 2.0f * (qyy + qzz), 2.0f * (qxy + qwz), 2.0f * (qxz - qwy));
    r.c[1] = F3(2.0f * (qxy - qwz), 1.0f - 2.0f * (qxx + qzz), 2.0f * (qyz + qwx));
    r.c[2] = F3(2.0f * (qxz + qwy), 2.0f * (qyz - qwx), 1.0f - 2.0f * (qxx + qyy));
    return r;
}
inline m3 matrix_orientation(const m4& t) { return mat3_of_quat(orientation_quat(t)); }

TR_HD float sh_sin(float x) { return (float)sin((double)x); }
TR_HD float sh_cos(float x) { return (float)cos((double)x); }
TR_HD float sh_pow(float x, float y) { return (float)pow((double)x, (double)y); }

// even_sample_sphere(s, N, (rotation_x, rotation_y)) (shader/math.glsl:305-315, 336-340)
TR_HD f3 sh_local_dir(uint s, uint n, float rotation_x, float rotation_y) {
    const float o = ((float)s + rotation_x) * SH_GOLDEN;
    const float u = ((float)s + rotation_y) / (float)n;
    const float cos_theta = 2.0f * u - 1.0f;
    const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
    const float phi = (o * 2.0f) * SH_PI;
    return F3(sh_cos(phi) * sin_theta, sh_sin(phi) * sin_theta, cos_theta);
}

// sh_basis (shader/spherical_harmonics.glsl:31-69): the first C entries of out
template <int ORDER>
TR_HD void sh_basis(f3 d, float* out) {
    const float x = d.x, y = d.y, z = d.z;
    const float x2 = x * x, y2 = y * y, z2 = z * z;
    out[0] = 0.2820947917738781f;
    if (ORDER >= 1) {
        out[1] = 0.4886025119029199f * y;
        out[2] = 0.4886025119029199f * z;
        out[3] = 0.4886025119029199f * x;
    }
    if (ORDER >= 2) {
        out[4] = 1.0925484305920792f * x * y;
        out[5] = 1.0925484305920792f * y * z;
        out[6] = 0.3153915652525201f * (3.0f * z2 - 1.0f);
        out[7] = 1.0925484305920792f * x * z;
        out[8] = 0.5462742152960396f * (x2 - y2);
    }
    if (ORDER >= 3) {
        out[9] = 0.5900435899266435f * y * (3.0f * x2 - y2);
        out[10] = 2.8906114426405543f * x * y * z;
        out[11] = 0.4570457994644658f * y * (5.0f * z2 - 1.0f);
        out[12] = 0.3731763325901155f * z * (5.0f * z2 - 3.0f);
        out[13] = 0.4570457994644658f * x * (5.0f * z2 - 1.0f);
        out[14] = 1.4453057213202771f * z * (x2 - y2);
        out[15] = 0.5900435899266435f * x * (x2 - 3.0f * y2);
    }
    if (ORDER >= 4) {
        out[16] = 2.503342941796705f * x * y * (x2 - y2);
        out[17] = 1.770130769779931f * y * z * (3.0f * x2 - y2);
        out[18] = 0.9461746957575602f * x * y * (7.0f * z2 - 1.0f);
        out[19] = 0.6690465435572893f * y * z * (7.0f * z2 - 3.0f);
        out[20] = 0.1057855469152043f * ((35.0f * z2 * z2 - 30.0f * z2) + 3.0f);
        out[21] = 0.6690465435572893f * x * z * (7.0f * z2 - 3.0f);
        out[22] = 0.4730873478787801f * (x2 - y2) * (7.0f * z2 - 1.0f);
        out[23] = 1.770130769779931f * x * z * (x2 - 3.0f * y2);
        out[24] = 0.6258357354491763f * ((x2 * x2 - 6.0f * x2 * y2) + y2 * y2);
    }
}

}  // namespace tr
