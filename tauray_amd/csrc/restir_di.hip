// ReSTIR DI for gfx950 - reservoir resampling of direct light, written after the reference's shader/restir_di.glsl,
// shader/restir_di_canonical_and_temporal.rgen and shader/restir_di_spatial.rgen, behind the entry points trhip_restir_di_* of include/trhip.h.
//   k_restir_di_canonical  per pixel of every viewport: the first hit and its surface (first_hit.h), the surface
//                          record, RIS over `candidates` light samples (a shadow ray in every target function), the temporal merge of
//                          the reprojected pixel's history reservoir
//   k_restir_di_spatial    per pixel: the neighbour search, the pairwise-MIS merge of the neighbours' canonical reservoirs (two shadow rays
//                          a neighbour), the chosen sample's shading (one more), the history reservoir and the colour
// Constants, layouts, the order of operations and the order of random draws: restir_di.h.  Both kernels are IEEE fp32, evaluated without
// contraction in a fixed order, no atomics: two runs of the same inputs give the same bits.  The front half is first_hit.h's, the one
// k_gbuffer and k_feature call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "restir_di.h"
#include "first_hit.h"
#include "stage_host.h"
#include "pt.h"
#include "trace.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;

struct RestirParams {
    int candidates;
    float search_radius, max_confidence, min_ray_dist;
    float prob_point, prob_tri, prob_dir, prob_env;
    uint rng_seed, frame;              // pcg(rng_seed) or 0; the stage's frame counter
    int has_history;
    RestirSurface* surface;            // this frame's half
    const RestirSurface* prev_surface; // the other half
    RestirReservoir* canonical;
    RestirReservoir* history;
    f4* out;
    RestirCandidateRecord* rec_candidates;      // null unless options.record, as the three below
    RestirTemporalRecord* rec_temporal;
    RestirSpatialRecord* rec_spatial;
    RestirFinalRecord* rec_final;
};

#define TR_U(x) __float_as_uint(x)

// tile_pixel's launch shape (first_hit.h).
// Two waves per SIMD: unbounded, the fp64 functions of RoundedMath took it to 256 VGPRs plus AGPR copies at one wave.
template <bool TWO_LEVEL, bool TEMPORAL>
__global__ __launch_bounds__(KB, 2) void k_restir_di_canonical(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirParams P, uint* overflow_flag) {
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
    RestirState r = restir_create();
    RestirTemporalRecord trec = {-1, -1, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    if (hit.instance_id >= 0) {
        SurfacePoint v;
        first_hit_surface(sv, hit, dir, ray_origin, v, dom.mat);
        dom.pos = v.pos; dom.mapped_normal = v.mapped_normal; dom.flat_normal = v.hard_normal;
        dom.view = normalize(v.pos - ray_origin);
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, 0u}, 2u * P.frame, P.rng_seed, SAMPLER_UNIFORM);

        bool reuse = false;
        int rx = -1, ry = -1;
        float prev_confidence = 0.0f;
        if (TEMPORAL) {      // get_reprojected_pixel, temporal_edge_detection (restir_di.glsl:138-153, 375-388)
            const f3 prev_pos = surface_prev_pos(sv, hit.instance_id, hit.primitive_id, hit.u, hit.v);
            const f3 m = get_camera_projection(sv.prev_cameras[viewport], projection, prev_pos);
            const f2 motion = F2(m.x, 1.0f - m.y) * F2((float)L.launch_w, (float)L.launch_h) - 0.5f;
            const int ix = (int)motion.x, iy = (int)motion.y;
            const f2 off = F2(motion.x - (float)ix, motion.y - (float)iy);
            const f4 rs = u4_to_unit(pcg4d(ls.rs));
            rx = ix + (off.x < rs.x ? 0 : 1); ry = iy + (off.y < rs.y ? 0 : 1);
            if (P.has_history && (uint)rx < L.launch_w && (uint)ry < L.launch_h) {
                f3 ppos, pflat;
                int pid;
                const RestirSurface* prev = P.prev_surface + layer * layer_px + (size_t)ry * L.launch_w + (uint)rx;
                restir_load_surface_head(prev, ppos, pid, pflat);
                const u4 w1 = restir_word(prev, 1);
                const f3 prev_normal = F3(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z));
                const float delta_pos = length(dom.pos - ppos);
                const float max_range = 0.01f * length(ray_origin - dom.pos) / (fabsf(dot(dom.view, dom.mapped_normal)) + 0.001f);
                reuse = !(dot(prev_normal, dom.mapped_normal) < 0.95f || delta_pos > max_range);
            }
            if (reuse) prev_confidence = __uint_as_float(restir_word(P.history + layer * layer_px + (size_t)ry * L.launch_w + (uint)rx, 0).w);
        }

        // resampled_importance_sampling (restir_di_canonical_and_temporal.rgen:58-125)
        const float mis_weight = 1.0f / ((float)P.candidates + prev_confidence);
        for (int i = 0; i < P.candidates; ++i) {
            const u4 rnd = pcg4d(ls.rs);
            RestirLightRecord Lr;
            float light_pdf;
            const RestirSample s = restir_sample_canonical(sv, P, rnd, dom.pos, Lr, light_pdf);
            f3 light_dir, light_norm;
            float light_dist2;
            const f3 contrib = restir_contribution(sv, s, Lr, dom, light_dir, light_dist2, light_norm);
            const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
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

        if (TEMPORAL) {
            trec.px = rx; trec.py = ry; trec.reuse = reuse ? 1u : 0u; trec.prev_confidence = prev_confidence;
            if (reuse) {
                const RestirState prev_r = restir_load(P.history + layer * layer_px + (size_t)ry * L.launch_w + (uint)rx);
                const RestirLightRecord Lr = restir_fetch_light(sv, prev_r.ls);
                f3 light_dir, light_norm;
                float light_dist2;
                const float target = rgb_to_luminance(restir_contribution(sv, prev_r.ls, Lr, dom, light_dir, light_dist2, light_norm));
                float weight = ((prev_r.confidence / (r.confidence + prev_r.confidence)) * target) * prev_r.uc_weight;
                if (isnan(weight)) weight = 0.0f;
                const float u = u4_to_unit(pcg4d(ls.rs)).x;
                const bool selected = restir_update(r, prev_r.ls, weight, u);
                if (selected) r.target_function = target;
                r.confidence = r.confidence + prev_r.confidence;
                r.uc_weight = restir_uc_weight(r);
                trec.target = target; trec.weight = weight; trec.draw = u; trec.selected = selected ? 1u : 0u;
            }
            r.confidence = fmin2(r.confidence, P.max_confidence);
        }
    }
    if (overflow) *overflow_flag = 1;
    restir_store_surface(P.surface + pix, dom, hit.instance_id >= 0 ? hit.instance_id : -1);
    restir_store(P.canonical + pix, restir_pack(r));
    if (P.rec_temporal) {
        restir_set_word(P.rec_temporal + pix, 0, u4{(uint)trec.px, (uint)trec.py, trec.reuse, TR_U(trec.prev_confidence)});
        restir_set_word(P.rec_temporal + pix, 1, u4{TR_U(trec.target), TR_U(trec.weight), TR_U(trec.draw), trec.selected});
    }
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

template <bool TWO_LEVEL, int SPATIAL>
__global__ __launch_bounds__(KB, 2) void k_restir_di_spatial(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirParams P, uint* overflow_flag) {
    __shared__ int s_stack_rows[TR_STACK_WORDS];
    int* const s_stack = s_stack_rows + TR_STACK_ROW0;
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const uint layer = blockIdx.z, viewport = list.v[layer];
    const size_t layer_px = (size_t)L.launch_w * L.launch_h;
    const size_t pix = layer * layer_px + (size_t)py * L.launch_w + (uint)px;
    const RestirSurface* surfaces = P.surface + layer * layer_px;
    const RestirReservoir* canonicals = P.canonical + layer * layer_px;
    RestirDomain dom;
    const int instance_id = restir_load_surface(P.surface + pix, dom);
    int overflow = 0;
    if (instance_id < 0) {      // the direct stage's miss colour (k_direct, path_tracer.hip): the visible directional lights, then the environment
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
        restir_store(P.history + pix, restir_pack(restir_create()));
        P.out[pix] = F4(light, 1.0f);
        const u4 zero = {0u, 0u, 0u, 0u};
        if (P.rec_final) { restir_set_word(P.rec_final + pix, 0, zero); restir_set_word(P.rec_final + pix, 1, zero); }
        if (P.rec_spatial)
            for (int i = 0; i < SPATIAL; ++i) {
                RestirSpatialRecord* rec = P.rec_spatial + (pix * SPATIAL + i);
                restir_set_word(rec, 0, u4{~0u, ~0u, 0u, 0u}); restir_set_word(rec, 1, zero); restir_set_word(rec, 2, zero); restir_set_word(rec, 3, zero);
            }
        return;
    }
    const RestirState canonical = restir_load(P.canonical + pix);
    RestirState r = restir_create();
    RestirFinalRecord frec = {F3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    if (SPATIAL > 0) {
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, 0u}, 2u * P.frame + 1u, P.rng_seed, SAMPLER_UNIFORM);
        constexpr int S = SPATIAL > 0 ? SPATIAL : 1;
        int sx[S], sy[S];
        uint good_bits = 0u;
#pragma unroll
        for (int i = 0; i < S; ++i) { sx[i] = -1; sy[i] = -1; }
        int good_neighbors = 0, bad_neighbors = 0;
        const CameraData& cam = sv.cameras[viewport];
        float inv_max_plane_dist;
        {   // get_inv_max_plane_dist (restir_di.glsl:398-403)
            float frustum_size = fmin2(fabsf(cam.proj_inverse.c[0].x * 2.0f), fabsf(cam.proj_inverse.c[1].y * 2.0f));
            frustum_size = frustum_size * fabsf(dot(F3(cam.view_inverse.c[2]), F3(cam.view_inverse.c[3]) - dom.pos));
            inv_max_plane_dist = 1.0f / frustum_size;
        }
        for (int i = 0; i < SPATIAL * 2; ++i) {
            const f4 rnd = u4_to_unit(pcg4d(ls.rs));
            const f2 d = P.search_radius * sample_blackman_harris_concentric_disk<RoundedMath>(F2(rnd.x, rnd.y));
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
            } else if (bad && good_neighbors + bad_neighbors < SPATIAL) {
                ++bad_neighbors;
                set_slot(sx, sy, good_bits, SPATIAL - bad_neighbors, nx, ny, false);
            }
        }
        float total_confidence = canonical.confidence;
#pragma unroll
        for (int i = 0; i < S; ++i)
            if (sx[i] >= 0) total_confidence = total_confidence + __uint_as_float(restir_word(canonicals + (size_t)sy[i] * L.launch_w + (uint)sx[i], 0).w);
        float canonical_m = canonical.confidence / total_confidence;
        const bool canonical_null = restir_is_null(canonical.ls);
        // one copy of the two re-evaluations and their traversals: the loop stays a loop, the slot is read by selects over constants
#pragma unroll 1
        for (int i = 0; i < SPATIAL; ++i) {
            int nx, ny;
            get_slot(sx, sy, i, nx, ny);
            RestirSpatialRecord srec = {nx, ny, (good_bits >> i) & 1u, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (nx >= 0) {
                const size_t npix = (size_t)ny * L.launch_w + (uint)nx;
                RestirDomain sample_domain;
                restir_load_surface(surfaces + npix, sample_domain);
                const RestirState n = restir_load(canonicals + npix);
                if (!restir_is_null(n.ls)) {
                    const RestirLightRecord Ln = restir_fetch_light(sv, n.ls);
                    f3 light_dir, light_norm;
                    float light_dist2;
                    const f3 contrib = restir_contribution(sv, n.ls, Ln, dom, light_dir, light_dist2, light_norm);
                    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
                    const float target = rgb_to_luminance(contrib * visibility);
                    const f3 x = dom.pos + light_dir * sqrtf(light_dist2);
                    const float jacob = n.ls.type > 1u ? 1.0f : restir_jacobian(sample_domain.pos, dom.pos, x, light_norm);
                    const float m = restir_mis_noncanonical(canonical.confidence, n.confidence, total_confidence, n.target_function, target, jacob);
                    float wi = ((target * m) * n.uc_weight) * jacob;
                    if (isnan(wi)) wi = 0.0f;
                    const float u = u4_to_unit(pcg4d(ls.rs)).x;
                    const bool selected = restir_update(r, n.ls, wi, u);
                    if (selected) r.target_function = target;
                    srec.selected = selected ? 1u : 0u; srec.target_n = target; srec.visibility_n = visibility; srec.jacobian_n = jacob; srec.m = m; srec.wi = wi; srec.draw = u;
                }
                r.confidence = r.confidence + n.confidence;
                if (!canonical_null) {
                    const RestirLightRecord Lc = restir_fetch_light(sv, canonical.ls);      // fetched per neighbour, not held across the loop
                    f3 light_dir, light_norm;
                    float light_dist2;
                    const f3 contrib = restir_contribution(sv, canonical.ls, Lc, sample_domain, light_dir, light_dist2, light_norm);
                    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, sample_domain.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
                    const float alt_target = rgb_to_luminance(contrib * visibility);
                    const f3 x = sample_domain.pos + light_dir * sqrtf(light_dist2);
                    const float jacob = canonical.ls.type > 1u ? 1.0f : restir_jacobian(dom.pos, sample_domain.pos, x, light_norm);
                    const float mc = restir_mis_canonical(canonical.confidence, n.confidence, total_confidence, canonical.target_function, alt_target, jacob);
                    canonical_m = canonical_m + mc;
                    srec.target_c = alt_target; srec.visibility_c = visibility; srec.jacobian_c = jacob; srec.mis_canonical = mc;
                }
            }
            if (P.rec_spatial) {
                RestirSpatialRecord* rec = P.rec_spatial + (pix * SPATIAL + i);
                restir_set_word(rec, 0, u4{(uint)srec.px, (uint)srec.py, srec.good, srec.selected});
                restir_set_word(rec, 1, u4{TR_U(srec.target_n), TR_U(srec.visibility_n), TR_U(srec.jacobian_n), TR_U(srec.m)});
                restir_set_word(rec, 2, u4{TR_U(srec.wi), TR_U(srec.draw), TR_U(srec.target_c), TR_U(srec.visibility_c)});
                restir_set_word(rec, 3, u4{TR_U(srec.jacobian_c), TR_U(srec.mis_canonical), 0u, 0u});
            }
        }
        float wi = (canonical_m * canonical.target_function) * canonical.uc_weight;
        if (isnan(wi)) wi = 0.0f;
        const float u = u4_to_unit(pcg4d(ls.rs)).x;
        const bool selected = restir_update(r, canonical.ls, wi, u);
        if (selected) r.target_function = canonical.target_function;
        r.confidence = r.confidence + canonical.confidence;
        r.uc_weight = restir_uc_weight(r);
        frec.canonical_m = canonical_m; frec.wi = wi; frec.draw = u; frec.selected = selected ? 1u : 0u;
    } else {
        r = canonical;
    }
    const RestirLightRecord Lf = restir_fetch_light(sv, r.ls);
    f3 light_dir, light_norm;
    float light_dist2;
    const f3 contrib = restir_contribution(sv, r.ls, Lf, dom, light_dir, light_dist2, light_norm);
    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
    if (overflow) *overflow_flag = 1;
    const f3 shaded = contrib * visibility;
    restir_store(P.history + pix, restir_pack(r));
    P.out[pix] = F4(shaded * r.uc_weight + dom.mat.emission, 1.0f);
    frec.contribution = contrib; frec.visibility = visibility;
    if (P.rec_final) {
        restir_set_word(P.rec_final + pix, 0, u4{TR_U(frec.contribution.x), TR_U(frec.contribution.y), TR_U(frec.contribution.z), TR_U(frec.visibility)});
        restir_set_word(P.rec_final + pix, 1, u4{TR_U(frec.canonical_m), TR_U(frec.wi), TR_U(frec.draw), frec.selected});
    }
}

using RestirKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, RestirParams, uint*);

template <bool TWO_LEVEL>
RestirKernel spatial_kernel(uint32_t spatial) {
    switch (spatial) {
        case 0: return k_restir_di_spatial<TWO_LEVEL, 0>;
        case 1: return k_restir_di_spatial<TWO_LEVEL, 1>;
        case 2: return k_restir_di_spatial<TWO_LEVEL, 2>;
        case 3: return k_restir_di_spatial<TWO_LEVEL, 3>;
        default: return k_restir_di_spatial<TWO_LEVEL, 4>;
    }
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_restir_di : StageHost<3> {
    trhip_device* dev = nullptr;
    trhip_restir_di_options opt = {};
    uint32_t w = 0, h = 0, layers = 0;
    uint32_t frame = 0;                      // frames since create or reset: the sampler's frame, the surface pair's parity
    std::vector<uint32_t> viewports;         // the last frame's list: layer i's history belongs to viewports[i]
    RestirSurface* surface[2] = {nullptr, nullptr};
    RestirReservoir *canonical = nullptr, *history = nullptr;
    RestirCandidateRecord* rec_candidates = nullptr;
    RestirTemporalRecord* rec_temporal = nullptr;
    RestirSpatialRecord* rec_spatial = nullptr;
    RestirFinalRecord* rec_final = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
};

static_assert(sizeof(trhip_restir_di_surface) == sizeof(RestirSurface) && sizeof(trhip_restir_di_reservoir) == sizeof(RestirReservoir), "downloads are the kernels' records");
static_assert(sizeof(trhip_restir_di_candidate) == sizeof(RestirCandidateRecord) && sizeof(trhip_restir_di_temporal) == sizeof(RestirTemporalRecord), "downloads are the kernels' records");
static_assert(sizeof(trhip_restir_di_spatial) == sizeof(RestirSpatialRecord) && sizeof(trhip_restir_di_final) == sizeof(RestirFinalRecord), "downloads are the kernels' records");

extern "C" {

int trhip_restir_di_create(trhip_device* dev, const trhip_restir_di_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_restir_di** out) {
    if (!out) return set_error("trhip_restir_di_create: null out");
    *out = nullptr;
    if (!opt) return set_error("trhip_restir_di_create: null options");
    if (opt->candidates < 1 || opt->candidates > (uint32_t)RESTIR_MAX_CANDIDATES)
        return set_error("trhip_restir_di_create: candidates " + std::to_string(opt->candidates) + " is outside 1..32");
    if (opt->spatial_samples > (uint32_t)RESTIR_MAX_SPATIAL)
        return set_error("trhip_restir_di_create: spatial_samples " + std::to_string(opt->spatial_samples) + " is outside 0..4");
    if (!(opt->search_radius > 0.0f) || !(opt->search_radius <= 1024.0f)) return set_error("trhip_restir_di_create: search_radius must be in (0, 1024]");
    if (!(opt->max_confidence >= 1.0f) || !std::isfinite(opt->max_confidence)) return set_error("trhip_restir_di_create: max_confidence must be finite and at least 1");
    if (opt->temporal_reuse != 0 && opt->temporal_reuse != 1) return set_error("trhip_restir_di_create: temporal_reuse must be 0 or 1");
    if (!(opt->min_ray_dist > 0.0f) || !std::isfinite(opt->min_ray_dist)) return set_error("trhip_restir_di_create: min_ray_dist must be finite and positive");
    if (opt->record != 0 && opt->record != 1) return set_error("trhip_restir_di_create: record must be 0 or 1");
    if (width == 0 || height == 0 || layers == 0) return set_error("trhip_restir_di_create: zero width, height or layer count");
    if (width > 16384 || height > 16384 || layers > 4096) return set_error("trhip_restir_di_create: image too large");
    if (!dev) return set_error("trhip_restir_di_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_restir_di* s = new trhip_restir_di;
    s->dev = dev; s->hip_device = device_index(dev);
    s->opt = *opt;
    s->w = width; s->h = height; s->layers = layers;
    const size_t n = s->pixels();
    s->alloc_zeroed(s->surface[0], n * sizeof(RestirSurface));
    s->alloc_zeroed(s->surface[1], n * sizeof(RestirSurface));
    s->alloc_zeroed(s->canonical, n * sizeof(RestirReservoir));
    s->alloc_zeroed(s->history, n * sizeof(RestirReservoir));
    if (opt->record) {
        s->alloc_zeroed(s->rec_candidates, n * opt->candidates * sizeof(RestirCandidateRecord));
        s->alloc_zeroed(s->rec_temporal, n * sizeof(RestirTemporalRecord));
        if (opt->spatial_samples) s->alloc_zeroed(s->rec_spatial, n * opt->spatial_samples * sizeof(RestirSpatialRecord));
        s->alloc_zeroed(s->rec_final, n * sizeof(RestirFinalRecord));
    }
    return stage_finish_create("trhip_restir_di_create", s, out);
}

void trhip_restir_di_destroy(trhip_restir_di* s) { stage_destroy(s); }

int trhip_restir_di_reset(trhip_restir_di* s) {
    if (!s) return set_error("trhip_restir_di_reset: null stage");
    s->frame = 0;
    return 0;
}

int trhip_restir_di_render(trhip_restir_di* s, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream) {
    if (!s) return set_error("trhip_restir_di_render: null stage");
    if (!viewports || !out_color_dev) return set_error("trhip_restir_di_render: null argument");
    DEVCHK(s->hip_device);
    DeviceScene* scene = device_scene(s->dev);
    if (int r = check_scene_ready("trhip_restir_di_render", scene->instance_count, scene->accel_built)) return r;
    if (int r = check_viewport_list("trhip_restir_di_render", viewports, count, s->layers, scene->camera_count)) return r;
    // History and the previous surface records are kept per layer, the position in the list: another list would merge another viewport's
    if (s->opt.temporal_reuse && s->frame > 0 && !std::equal(viewports, viewports + count, s->viewports.begin(), s->viewports.end()))
        return set_error("trhip_restir_di_render: the viewport list differs from the last frame's, whose history it would reuse: call trhip_restir_di_reset first");
    const LaunchCtx L = whole_image_launch(s->w, s->h);
    const size_t layer_px = (size_t)s->w * s->h;
    hipStream_t st = (hipStream_t)stream;
    RestirParams base{};
    base.candidates = (int)s->opt.candidates;
    base.search_radius = s->opt.search_radius; base.max_confidence = s->opt.max_confidence; base.min_ray_dist = s->opt.min_ray_dist;
    nee_probabilities(*scene, 1.0f, 1.0f, 1.0f, 1.0f, base.prob_point, base.prob_tri, base.prob_dir, base.prob_env);
    { uint seed = s->opt.rng_seed; base.rng_seed = seed != 0 ? pcg(seed) : 0; }                  // src/rt_stage.cc:82
    base.frame = s->frame;
    base.has_history = s->frame > 0;
    const bool temporal = s->opt.temporal_reuse != 0;
    const RestirKernel kernels[2] = {
        scene->two_level ? (temporal ? k_restir_di_canonical<true, true> : k_restir_di_canonical<true, false>)
                         : (temporal ? k_restir_di_canonical<false, true> : k_restir_di_canonical<false, false>),
        scene->two_level ? spatial_kernel<true>(s->opt.spatial_samples) : spatial_kernel<false>(s->opt.spatial_samples)};
    const int cur = (int)(s->frame & 1u);
    // The canonical kernels of every chunk first, then the spatial ones: a chunk's spatial launch reads only its own layers
    HIPCHK(hipEventRecord(s->ev[0], st));
    for (int pass = 0; pass < 2; ++pass) {
        for_each_viewport_chunk<ViewportList>(viewports, count, [&](uint32_t first, uint32_t n, const ViewportList& list) {
            RestirParams P = base;
            const size_t off = first * layer_px;
            P.surface = s->surface[cur] + off; P.prev_surface = s->surface[cur ^ 1] + off;
            P.canonical = s->canonical + off; P.history = s->history + off;
            P.out = (f4*)out_color_dev + off;
            P.rec_candidates = s->rec_candidates ? s->rec_candidates + off * s->opt.candidates : nullptr;
            P.rec_temporal = s->rec_temporal ? s->rec_temporal + off : nullptr;
            P.rec_spatial = s->rec_spatial ? s->rec_spatial + off * s->opt.spatial_samples : nullptr;
            P.rec_final = s->rec_final ? s->rec_final + off : nullptr;
            hipLaunchKernelGGL(kernels[pass], tile_grid(s->w, s->h, n), dim3(KB), 0, st, scene->view(), L, projection, list, P, device_overflow_flag(s->dev));
        });
        HIPCHK(hipEventRecord(s->ev[pass + 1], st));
    }
    HIPCHK(hipGetLastError());
    s->frames += 1;
    s->frame += 1;
    s->viewports.assign(viewports, viewports + count);
    return 0;
}

int trhip_restir_di_get_timings(trhip_restir_di* s, trhip_restir_di_timings* out) {
    if (int r = stage_total_ms("trhip_restir_di_get_timings", s, out)) return r;
    snprintf(out->canonical_name, sizeof(out->canonical_name), "restir di canonical");
    snprintf(out->spatial_name, sizeof(out->spatial_name), "restir di spatial");
    if (s->frames == 0) return 0;
    HIPCHK(hipEventElapsedTime(&out->canonical_ms, s->ev[0], s->ev[1]));
    HIPCHK(hipEventElapsedTime(&out->spatial_ms, s->ev[1], s->ev[2]));
    return 0;
}

int trhip_restir_di_download(trhip_restir_di* s, int which, void* host, size_t bytes) {
    return stage_download("trhip_restir_di_download", s, host, bytes, [&](const void*& src, size_t& size) {
        const size_t n = s->pixels();
        const bool decision = which >= TRHIP_RESTIR_DI_CANDIDATES && which <= TRHIP_RESTIR_DI_FINAL;
        if (decision && !s->opt.record) return set_error("trhip_restir_di_download: the decision records are only kept with record");
        switch (which) {
            case TRHIP_RESTIR_DI_SURFACE:      // the half the last frame wrote
                src = s->surface[(s->frame + 1u) & 1u]; size = n * sizeof(RestirSurface); break;
            case TRHIP_RESTIR_DI_CANONICAL: src = s->canonical; size = n * sizeof(RestirReservoir); break;
            case TRHIP_RESTIR_DI_HISTORY: src = s->history; size = n * sizeof(RestirReservoir); break;
            case TRHIP_RESTIR_DI_CANDIDATES: src = s->rec_candidates; size = n * s->opt.candidates * sizeof(RestirCandidateRecord); break;
            case TRHIP_RESTIR_DI_TEMPORAL: src = s->rec_temporal; size = n * sizeof(RestirTemporalRecord); break;
            case TRHIP_RESTIR_DI_SPATIAL:
                if (!s->rec_spatial) return set_error("trhip_restir_di_download: the stage has no spatial samples");
                src = s->rec_spatial; size = n * s->opt.spatial_samples * sizeof(RestirSpatialRecord);
                break;
            case TRHIP_RESTIR_DI_FINAL: src = s->rec_final; size = n * sizeof(RestirFinalRecord); break;
            default: return set_error("trhip_restir_di_download: unknown buffer");
        }
        return 0;
    });
}

}  // extern "C"
