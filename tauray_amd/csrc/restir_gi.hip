// ReSTIR GI for gfx950 - reservoir resampling of one bounce of indirect light, behind the entry points trhip_restir_gi_* of include/trhip.h.
//   k_restir_gi_initial    per pixel of every viewport: the first hit and its surface (first_hit.h), the surface record, one
//                          cosine-hemisphere ray and its closest hit x_s, x_s's surface, one light sample there with its shadow ray: the
//                          initial sample (x_s, n_s, L_o), its pdf and its target; the reprojected position for the temporal kernel
//   k_restir_gi_temporal   no rays: the initial sample's resampling weight, the reprojection and the merge of the history reservoir
//   k_restir_gi_spatial    the neighbour search, the pairwise-MIS merge of the neighbours' canonical reservoirs (two shadow rays a
//                          neighbour), the chosen sample's shading (one more), the history reservoir and the colour added to `in`
// Constants, layouts, the order of operations and the order of random draws: restir_gi.h (and restir_di.h, whose rule it keeps).  Three
// kernels, not DI's two: the initial kernel holds two closest-hit traversals and two shade_surface calls, and the merge that follows needs
// none of their registers.  IEEE fp32 without contraction in a fixed order, no atomics: two runs of the same inputs give the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "restir_gi.h"
#include "first_hit.h"
#include "stage_host.h"
#include "pt.h"
#include "trace.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;

struct RestirGiParams {
    float search_radius, max_confidence, min_ray_dist;
    float prob_point, prob_tri, prob_dir, prob_env;
    uint rng_seed, frame;              // pcg(rng_seed) or 0; the stage's frame counter
    int has_history;
    RestirSurface* surface;            // this frame's half
    const RestirSurface* prev_surface; // the other half
    RestirGiReservoir* canonical;
    RestirGiReservoir* history;
    RestirGiReproject* reproject;      // null without temporal reuse
    const f4* in;                      // null: (0, 0, 0, 1)
    f4* out;
    RestirGiInitialRecord* rec_initial;         // null unless options.record, as the five below
    RestirSurface* rec_secondary;
    RestirCandidateRecord* rec_light;
    RestirTemporalRecord* rec_temporal;
    RestirSpatialRecord* rec_spatial;
    RestirFinalRecord* rec_final;
};

#define TR_U(x) __float_as_uint(x)

TR_DEV bool finite3(f3 v) { return !(isnan(v.x) || isnan(v.y) || isnan(v.z) || isinf(v.x) || isinf(v.y) || isinf(v.z)); }

// tile_pixel's launch shape (first_hit.h).  Bounded to two waves per SIMD as DI's canonical kernel; the two traversals and the two
// shade_surface calls follow one another and share registers: 148 VGPRs, three waves, no spills.
template <bool TWO_LEVEL>
__global__ __launch_bounds__(KB, 2) void k_restir_gi_initial(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirGiParams P, uint* overflow_flag) {
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
    RestirDomain dom = {}, dom2 = {};
    RestirGiState r = restir_gi_create();          // the initial sample; uc_weight holds its pdf until the temporal kernel
    r.uc_weight = 1.0f;
    RestirGiInitialRecord irec = {};
    irec.instance_id = -1; irec.primitive_id = -1; irec.t = -1.0f;
    RestirCandidateRecord lrec = {};
    lrec.light = RESTIR_NULL_INDEX;
    HitRecord hit2;
    hit2.instance_id = -1;
    f2 motion = F2(0.0f);
    float origin_dist = 0.0f;
    if (hit.instance_id >= 0) {
        SurfacePoint v;
        first_hit_surface(sv, hit, dir, ray_origin, v, dom.mat);
        dom.pos = v.pos; dom.mapped_normal = v.mapped_normal; dom.flat_normal = v.hard_normal;
        dom.view = normalize(v.pos - ray_origin);
        if (P.reproject) {       // get_reprojected_pixel before its rounding (restir_di.h `reprojection`)
            const f3 prev_pos = surface_prev_pos(sv, hit.instance_id, hit.primitive_id, hit.u, hit.v);
            const f3 m = get_camera_projection(sv.prev_cameras[viewport], projection, prev_pos);
            motion = F2(m.x, 1.0f - m.y) * F2((float)L.launch_w, (float)L.launch_h) - 0.5f;
            origin_dist = length(ray_origin - dom.pos);
        }
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, RESTIR_GI_SAMPLER_W}, 3u * P.frame, P.rng_seed, SAMPLER_UNIFORM);
        const f4 u = u4_to_unit(pcg4d(ls.rs));
        const f3 local = sample_cosine_hemisphere<RoundedMath>(F2(u.x, u.y));
        const f3 out_dir = mul(create_tangent_space(dom.mapped_normal), local);
        const float pdf = pdf_cosine_hemisphere(local);
        const bool cast = !(dot(out_dir, dom.flat_normal) < 1e-6f || pdf <= 0.0f);
        irec.draw = F2(u.x, u.y); irec.pdf = pdf; irec.traced = cast ? 1u : 0u; irec.dir = out_dir;
        if (cast) {
            TraceStats st = {};
            trace_closest4<1, false, TWO_LEVEL>(sv, dom.pos, out_dir, P.min_ray_dist, __builtin_huge_valf(), 0u, s_stack + threadIdx.x, hit2, st, overflow);
        }
        if (hit2.instance_id >= 0) {
            irec.instance_id = hit2.instance_id; irec.primitive_id = hit2.primitive_id; irec.u = hit2.u; irec.v = hit2.v; irec.t = hit2.t;
            SurfacePoint v2;
            first_hit_surface(sv, hit2, out_dir, dom.pos, v2, dom2.mat);
            dom2.pos = v2.pos; dom2.mapped_normal = v2.mapped_normal; dom2.flat_normal = v2.hard_normal;
            dom2.view = normalize(v2.pos - dom.pos);
            const u4 rnd = pcg4d(ls.rs);
            RestirLightRecord Lr;
            float light_pdf;
            const RestirSample s = restir_sample_canonical(sv, P, rnd, dom2.pos, Lr, light_pdf);
            f3 light_dir, light_norm;
            float light_dist2;
            const f3 contrib = restir_contribution(sv, s, Lr, dom2, light_dir, light_dist2, light_norm);
            const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom2.pos, contrib, light_dir, light_dist2, s_stack + threadIdx.x, overflow);
            f3 L_o = (contrib * visibility) / light_pdf;
            if (!finite3(L_o)) L_o = F3(0.0f);
            irec.light_draw = rnd; irec.L_o = L_o;
            lrec.light = s.type << 30 | s.index; lrec.light_data = s.data; lrec.pdf = light_pdf; lrec.contribution = contrib; lrec.visibility = visibility;
            if (restir_casts(L_o)) {
                r.s.x = dom2.pos; r.s.n = dom2.flat_normal; r.s.L = L_o;
                r.uc_weight = pdf;
                f3 d;
                float d2;
                r.target_function = rgb_to_luminance(restir_gi_contribution(r.s, dom, d, d2));
                irec.target = r.target_function;
            }
        }
    }
    if (overflow) *overflow_flag = 1;
    restir_store_surface(P.surface + pix, dom, hit.instance_id >= 0 ? hit.instance_id : -1);
    restir_gi_store(P.canonical + pix, r);
    if (P.reproject) restir_set_word(P.reproject + pix, 0, u4{TR_U(motion.x), TR_U(motion.y), TR_U(origin_dist), 0u});
    if (P.rec_initial) {
        RestirGiInitialRecord* rec = P.rec_initial + pix;
        restir_set_word(rec, 0, u4{TR_U(irec.draw.x), TR_U(irec.draw.y), TR_U(irec.pdf), irec.traced});
        restir_set_word(rec, 1, u4{TR_U(irec.dir.x), TR_U(irec.dir.y), TR_U(irec.dir.z), TR_U(irec.t)});
        restir_set_word(rec, 2, u4{(uint)irec.instance_id, (uint)irec.primitive_id, TR_U(irec.u), TR_U(irec.v)});
        restir_set_word(rec, 3, irec.light_draw);
        restir_set_word(rec, 4, u4{TR_U(irec.L_o.x), TR_U(irec.L_o.y), TR_U(irec.L_o.z), TR_U(irec.target)});
        restir_store_surface(P.rec_secondary + pix, dom2, hit2.instance_id >= 0 ? hit2.instance_id : -1);
        RestirCandidateRecord* lr = P.rec_light + pix;
        restir_set_word(lr, 0, u4{lrec.light, TR_U(lrec.light_data.x), TR_U(lrec.light_data.y), TR_U(lrec.pdf)});
        restir_set_word(lr, 1, u4{TR_U(lrec.contribution.x), TR_U(lrec.contribution.y), TR_U(lrec.contribution.z), TR_U(lrec.visibility)});
        restir_set_word(lr, 2, u4{0u, 0u, 0u, 0u});
    }
}

// No rays and no traversal stack: the bound of four waves per SIMD leaves 128 registers; the one contribution and its fp64 pow take 78.
template <bool TEMPORAL>
__global__ __launch_bounds__(KB, 4) void k_restir_gi_temporal(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirGiParams P, uint* overflow_flag) {
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const uint layer = blockIdx.z, viewport = list.v[layer];
    const size_t layer_px = (size_t)L.launch_w * L.launch_h;
    const size_t pix = layer * layer_px + (size_t)py * L.launch_w + (uint)px;
    RestirDomain dom;
    const int instance_id = restir_load_surface(P.surface + pix, dom);
    RestirGiState r = restir_gi_create();
    RestirTemporalRecord trec = {-1, -1, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    float iweight = 0.0f, idraw = 0.0f;
    bool iselected = false;
    if (instance_id >= 0) {
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, RESTIR_GI_SAMPLER_W}, 3u * P.frame + 1u, P.rng_seed, SAMPLER_UNIFORM);
        bool reuse = false;
        int rx = -1, ry = -1;
        float prev_confidence = 0.0f;
        if (TEMPORAL) {      // get_reprojected_pixel's rounding, temporal_edge_detection (restir_di.h)
            const u4 rp = restir_word(P.reproject + pix, 0);
            const f2 motion = F2(__uint_as_float(rp.x), __uint_as_float(rp.y));
            const float origin_dist = __uint_as_float(rp.z);
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
                const float max_range = 0.01f * origin_dist / (fabsf(dot(dom.view, dom.mapped_normal)) + 0.001f);
                reuse = !(dot(prev_normal, dom.mapped_normal) < 0.95f || delta_pos > max_range);
            }
            if (reuse) prev_confidence = __uint_as_float(restir_word(P.history + layer * layer_px + (size_t)ry * L.launch_w + (uint)rx, 2).w);
        }
        // DI's resampled_importance_sampling with one candidate: the initial sample, whose pdf the initial kernel left in uc_weight's place
        const RestirGiState initial = restir_gi_load(P.canonical + pix);
        {
            const float mis_weight = 1.0f / (1.0f + prev_confidence);
            const float target = initial.target_function, pdf = initial.uc_weight;
            float weight = mis_weight * target / pdf;
            if (isnan(weight)) weight = 0.0f;
            const float u = u4_to_unit(pcg4d(ls.rs)).x;
            const bool selected = restir_gi_update(r, initial.s, weight, u);
            if (selected) r.target_function = target;
            r.confidence = r.confidence + 1.0f;
            iweight = weight; idraw = u; iselected = selected;
        }
        r.uc_weight = restir_gi_uc_weight(r);
        if (TEMPORAL) {
            trec.px = rx; trec.py = ry; trec.reuse = reuse ? 1u : 0u; trec.prev_confidence = prev_confidence;
            if (reuse) {
                const RestirGiState prev_r = restir_gi_load(P.history + layer * layer_px + (size_t)ry * L.launch_w + (uint)rx);
                f3 d;
                float d2;
                const float target = rgb_to_luminance(restir_gi_contribution(prev_r.s, dom, d, d2));
                float weight = ((prev_r.confidence / (r.confidence + prev_r.confidence)) * target) * prev_r.uc_weight;
                if (isnan(weight)) weight = 0.0f;
                const float u = u4_to_unit(pcg4d(ls.rs)).x;
                const bool selected = restir_gi_update(r, prev_r.s, weight, u);
                if (selected) r.target_function = target;
                r.confidence = r.confidence + prev_r.confidence;
                r.uc_weight = restir_gi_uc_weight(r);
                trec.target = target; trec.weight = weight; trec.draw = u; trec.selected = selected ? 1u : 0u;
            }
            r.confidence = fmin2(r.confidence, P.max_confidence);
        }
    }
    restir_gi_store(P.canonical + pix, r);
    if (P.rec_temporal) {
        restir_set_word(P.rec_temporal + pix, 0, u4{(uint)trec.px, (uint)trec.py, trec.reuse, TR_U(trec.prev_confidence)});
        restir_set_word(P.rec_temporal + pix, 1, u4{TR_U(trec.target), TR_U(trec.weight), TR_U(trec.draw), trec.selected});
        restir_set_word(P.rec_initial + pix, 5, u4{TR_U(iweight), TR_U(idraw), iselected ? 1u : 0u, 0u});
    }
}

// spatial_samples[k] = value for a k the compiler cannot see: selects over constants, the array stays in registers (as restir_di.hip)
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

// Two waves per SIMD as DI's spatial kernel: the shadow traversal under the fp64 lobes
template <bool TWO_LEVEL, int SPATIAL>
__global__ __launch_bounds__(KB, 2) void k_restir_gi_spatial(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirGiParams P, uint* overflow_flag) {
    __shared__ int s_stack_rows[TR_STACK_WORDS];
    int* const s_stack = s_stack_rows + TR_STACK_ROW0;
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const uint layer = blockIdx.z, viewport = list.v[layer];
    const size_t layer_px = (size_t)L.launch_w * L.launch_h;
    const size_t pix = layer * layer_px + (size_t)py * L.launch_w + (uint)px;
    const RestirSurface* surfaces = P.surface + layer * layer_px;
    const RestirGiReservoir* canonicals = P.canonical + layer * layer_px;
    RestirDomain dom;
    const int instance_id = restir_load_surface(P.surface + pix, dom);
    const f4 in = P.in ? P.in[pix] : F4(0.0f, 0.0f, 0.0f, 1.0f);
    int overflow = 0;
    if (instance_id < 0) {
        restir_gi_store(P.history + pix, restir_gi_create());
        P.out[pix] = in;
        const u4 zero = {0u, 0u, 0u, 0u};
        if (P.rec_final) { restir_set_word(P.rec_final + pix, 0, zero); restir_set_word(P.rec_final + pix, 1, zero); }
        if (P.rec_spatial)
            for (int i = 0; i < SPATIAL; ++i) {
                RestirSpatialRecord* rec = P.rec_spatial + (pix * SPATIAL + i);
                restir_set_word(rec, 0, u4{~0u, ~0u, 0u, 0u}); restir_set_word(rec, 1, zero); restir_set_word(rec, 2, zero); restir_set_word(rec, 3, zero);
            }
        return;
    }
    const RestirGiState canonical = restir_gi_load(P.canonical + pix);
    RestirGiState r = restir_gi_create();
    RestirFinalRecord frec = {F3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    if (SPATIAL > 0) {
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, RESTIR_GI_SAMPLER_W}, 3u * P.frame + 2u, P.rng_seed, SAMPLER_UNIFORM);
        constexpr int S = SPATIAL > 0 ? SPATIAL : 1;
        int sx[S], sy[S];
        uint good_bits = 0u;
#pragma unroll
        for (int i = 0; i < S; ++i) { sx[i] = -1; sy[i] = -1; }
        int good_neighbors = 0, bad_neighbors = 0;
        const CameraData& cam = sv.cameras[viewport];
        float inv_max_plane_dist;
        {   // get_inv_max_plane_dist (restir_di.h `neighbours`)
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
            if (sx[i] >= 0) total_confidence = total_confidence + __uint_as_float(restir_word(canonicals + (size_t)sy[i] * L.launch_w + (uint)sx[i], 2).w);
        float canonical_m = canonical.confidence / total_confidence;
        const bool canonical_null = restir_gi_is_null(canonical.s);
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
                const RestirGiState n = restir_gi_load(canonicals + npix);
                if (!restir_gi_is_null(n.s)) {
                    f3 sdir;
                    float sdist2;
                    const f3 contrib = restir_gi_contribution(n.s, dom, sdir, sdist2);
                    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, sdir, sdist2, s_stack + threadIdx.x, overflow);
                    const float target = rgb_to_luminance(contrib * visibility);
                    const float jacob = restir_jacobian(sample_domain.pos, dom.pos, n.s.x, n.s.n);
                    const float m = restir_mis_noncanonical(canonical.confidence, n.confidence, total_confidence, n.target_function, target, jacob);
                    float wi = ((target * m) * n.uc_weight) * jacob;
                    if (isnan(wi)) wi = 0.0f;
                    const float u = u4_to_unit(pcg4d(ls.rs)).x;
                    const bool selected = restir_gi_update(r, n.s, wi, u);
                    if (selected) r.target_function = target;
                    srec.selected = selected ? 1u : 0u; srec.target_n = target; srec.visibility_n = visibility; srec.jacobian_n = jacob; srec.m = m; srec.wi = wi; srec.draw = u;
                }
                r.confidence = r.confidence + n.confidence;
                if (!canonical_null) {
                    f3 sdir;
                    float sdist2;
                    const f3 contrib = restir_gi_contribution(canonical.s, sample_domain, sdir, sdist2);
                    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, sample_domain.pos, contrib, sdir, sdist2, s_stack + threadIdx.x, overflow);
                    const float alt_target = rgb_to_luminance(contrib * visibility);
                    const float jacob = restir_jacobian(dom.pos, sample_domain.pos, canonical.s.x, canonical.s.n);
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
        const bool selected = restir_gi_update(r, canonical.s, wi, u);
        if (selected) r.target_function = canonical.target_function;
        r.confidence = r.confidence + canonical.confidence;
        r.uc_weight = restir_gi_uc_weight(r);
        frec.canonical_m = canonical_m; frec.wi = wi; frec.draw = u; frec.selected = selected ? 1u : 0u;
    } else {
        r = canonical;
    }
    f3 sdir;
    float sdist2;
    const f3 contrib = restir_gi_contribution(r.s, dom, sdir, sdist2);
    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, sdir, sdist2, s_stack + threadIdx.x, overflow);
    if (overflow) *overflow_flag = 1;
    const f3 shaded = contrib * visibility;
    restir_gi_store(P.history + pix, r);
    P.out[pix] = F4(F3(in) + shaded * r.uc_weight, in.w);
    frec.contribution = contrib; frec.visibility = visibility;
    if (P.rec_final) {
        restir_set_word(P.rec_final + pix, 0, u4{TR_U(frec.contribution.x), TR_U(frec.contribution.y), TR_U(frec.contribution.z), TR_U(frec.visibility)});
        restir_set_word(P.rec_final + pix, 1, u4{TR_U(frec.canonical_m), TR_U(frec.wi), TR_U(frec.draw), frec.selected});
    }
}

using RestirGiKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, RestirGiParams, uint*);

template <bool TWO_LEVEL>
RestirGiKernel spatial_kernel(uint32_t spatial) {
    switch (spatial) {
        case 0: return k_restir_gi_spatial<TWO_LEVEL, 0>;
        case 1: return k_restir_gi_spatial<TWO_LEVEL, 1>;
        case 2: return k_restir_gi_spatial<TWO_LEVEL, 2>;
        case 3: return k_restir_gi_spatial<TWO_LEVEL, 3>;
        default: return k_restir_gi_spatial<TWO_LEVEL, 4>;
    }
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_restir_gi : StageHost<4> {
    trhip_device* dev = nullptr;
    trhip_restir_gi_options opt = {};
    uint32_t w = 0, h = 0, layers = 0;
    uint32_t frame = 0;                      // frames since create or reset: the sampler's frame, the surface pair's parity
    std::vector<uint32_t> viewports;         // the last frame's list: layer i's history belongs to viewports[i]
    RestirSurface* surface[2] = {nullptr, nullptr};
    RestirGiReservoir *canonical = nullptr, *history = nullptr;
    RestirGiReproject* reproject = nullptr;
    RestirGiInitialRecord* rec_initial = nullptr;
    RestirSurface* rec_secondary = nullptr;
    RestirCandidateRecord* rec_light = nullptr;
    RestirTemporalRecord* rec_temporal = nullptr;
    RestirSpatialRecord* rec_spatial = nullptr;
    RestirFinalRecord* rec_final = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
};

static_assert(sizeof(trhip_restir_gi_reservoir) == sizeof(RestirGiReservoir) && sizeof(trhip_restir_gi_initial) == sizeof(RestirGiInitialRecord), "downloads are the kernels' records");

extern "C" {

int trhip_restir_gi_create(trhip_device* dev, const trhip_restir_gi_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_restir_gi** out) {
    if (!out) return set_error("trhip_restir_gi_create: null out");
    *out = nullptr;
    if (!opt) return set_error("trhip_restir_gi_create: null options");
    if (opt->spatial_samples > (uint32_t)RESTIR_MAX_SPATIAL)
        return set_error("trhip_restir_gi_create: spatial_samples " + std::to_string(opt->spatial_samples) + " is outside 0..4");
    if (!(opt->search_radius > 0.0f) || !(opt->search_radius <= 1024.0f)) return set_error("trhip_restir_gi_create: search_radius must be in (0, 1024]");
    if (!(opt->max_confidence >= 1.0f) || !std::isfinite(opt->max_confidence)) return set_error("trhip_restir_gi_create: max_confidence must be finite and at least 1");
    if (opt->temporal_reuse != 0 && opt->temporal_reuse != 1) return set_error("trhip_restir_gi_create: temporal_reuse must be 0 or 1");
    if (!(opt->min_ray_dist > 0.0f) || !std::isfinite(opt->min_ray_dist)) return set_error("trhip_restir_gi_create: min_ray_dist must be finite and positive");
    if (opt->record != 0 && opt->record != 1) return set_error("trhip_restir_gi_create: record must be 0 or 1");
    if (width == 0 || height == 0 || layers == 0) return set_error("trhip_restir_gi_create: zero width, height or layer count");
    if (width > 16384 || height > 16384 || layers > 4096) return set_error("trhip_restir_gi_create: image too large");
    if (!dev) return set_error("trhip_restir_gi_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_restir_gi* s = new trhip_restir_gi;
    s->dev = dev; s->hip_device = device_index(dev);
    s->opt = *opt;
    s->w = width; s->h = height; s->layers = layers;
    const size_t n = s->pixels();
    s->alloc_zeroed(s->surface[0], n * sizeof(RestirSurface));
    s->alloc_zeroed(s->surface[1], n * sizeof(RestirSurface));
    s->alloc_zeroed(s->canonical, n * sizeof(RestirGiReservoir));
    s->alloc_zeroed(s->history, n * sizeof(RestirGiReservoir));
    if (opt->temporal_reuse) s->alloc_zeroed(s->reproject, n * sizeof(RestirGiReproject));
    if (opt->record) {
        s->alloc_zeroed(s->rec_initial, n * sizeof(RestirGiInitialRecord));
        s->alloc_zeroed(s->rec_secondary, n * sizeof(RestirSurface));
        s->alloc_zeroed(s->rec_light, n * sizeof(RestirCandidateRecord));
        s->alloc_zeroed(s->rec_temporal, n * sizeof(RestirTemporalRecord));
        if (opt->spatial_samples) s->alloc_zeroed(s->rec_spatial, n * opt->spatial_samples * sizeof(RestirSpatialRecord));
        s->alloc_zeroed(s->rec_final, n * sizeof(RestirFinalRecord));
    }
    return stage_finish_create("trhip_restir_gi_create", s, out);
}

void trhip_restir_gi_destroy(trhip_restir_gi* s) { stage_destroy(s); }

int trhip_restir_gi_reset(trhip_restir_gi* s) {
    if (!s) return set_error("trhip_restir_gi_reset: null stage");
    s->frame = 0;
    return 0;
}

int trhip_restir_gi_render(trhip_restir_gi* s, int projection, const uint32_t* viewports, uint32_t count, const void* in_color_dev, void* out_color_dev, void* stream) {
    if (!s) return set_error("trhip_restir_gi_render: null stage");
    if (!viewports || !out_color_dev) return set_error("trhip_restir_gi_render: null argument");
    DEVCHK(s->hip_device);
    DeviceScene* scene = device_scene(s->dev);
    if (int r = check_scene_ready("trhip_restir_gi_render", scene->instance_count, scene->accel_built)) return r;
    if (int r = check_viewport_list("trhip_restir_gi_render", viewports, count, s->layers, scene->camera_count)) return r;
    // History and the previous surface records are kept per layer, the position in the list: another list would merge another viewport's
    if (s->opt.temporal_reuse && s->frame > 0 && !std::equal(viewports, viewports + count, s->viewports.begin(), s->viewports.end()))
        return set_error("trhip_restir_gi_render: the viewport list differs from the last frame's, whose history it would reuse: call trhip_restir_gi_reset first");
    const LaunchCtx L = whole_image_launch(s->w, s->h);
    const size_t layer_px = (size_t)s->w * s->h;
    hipStream_t st = (hipStream_t)stream;
    RestirGiParams base{};
    base.search_radius = s->opt.search_radius; base.max_confidence = s->opt.max_confidence; base.min_ray_dist = s->opt.min_ray_dist;
    nee_probabilities(*scene, 1.0f, 1.0f, 1.0f, 1.0f, base.prob_point, base.prob_tri, base.prob_dir, base.prob_env);
    { uint seed = s->opt.rng_seed; base.rng_seed = seed != 0 ? pcg(seed) : 0; }
    base.frame = s->frame;
    base.has_history = s->frame > 0;
    const bool temporal = s->opt.temporal_reuse != 0;
    const RestirGiKernel kernels[3] = {
        scene->two_level ? k_restir_gi_initial<true> : k_restir_gi_initial<false>,
        temporal ? k_restir_gi_temporal<true> : k_restir_gi_temporal<false>,
        scene->two_level ? spatial_kernel<true>(s->opt.spatial_samples) : spatial_kernel<false>(s->opt.spatial_samples)};
    const int cur = (int)(s->frame & 1u);
    // Every chunk's kernels of one pass, then the next pass: a chunk's launch reads only its own layers
    HIPCHK(hipEventRecord(s->ev[0], st));
    for (int pass = 0; pass < 3; ++pass) {
        for_each_viewport_chunk<ViewportList>(viewports, count, [&](uint32_t first, uint32_t n, const ViewportList& list) {
            RestirGiParams P = base;
            const size_t off = first * layer_px;
            P.surface = s->surface[cur] + off; P.prev_surface = s->surface[cur ^ 1] + off;
            P.canonical = s->canonical + off; P.history = s->history + off;
            P.reproject = s->reproject ? s->reproject + off : nullptr;
            P.in = in_color_dev ? (const f4*)in_color_dev + off : nullptr;
            P.out = (f4*)out_color_dev + off;
            P.rec_initial = s->rec_initial ? s->rec_initial + off : nullptr;
            P.rec_secondary = s->rec_secondary ? s->rec_secondary + off : nullptr;
            P.rec_light = s->rec_light ? s->rec_light + off : nullptr;
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

int trhip_restir_gi_get_timings(trhip_restir_gi* s, trhip_restir_gi_timings* out) {
    if (int r = stage_total_ms("trhip_restir_gi_get_timings", s, out)) return r;
    snprintf(out->initial_name, sizeof(out->initial_name), "restir gi initial");
    snprintf(out->temporal_name, sizeof(out->temporal_name), "restir gi temporal");
    snprintf(out->spatial_name, sizeof(out->spatial_name), "restir gi spatial");
    if (s->frames == 0) return 0;
    HIPCHK(hipEventElapsedTime(&out->initial_ms, s->ev[0], s->ev[1]));
    HIPCHK(hipEventElapsedTime(&out->temporal_ms, s->ev[1], s->ev[2]));
    HIPCHK(hipEventElapsedTime(&out->spatial_ms, s->ev[2], s->ev[3]));
    return 0;
}

int trhip_restir_gi_download(trhip_restir_gi* s, int which, void* host, size_t bytes) {
    return stage_download("trhip_restir_gi_download", s, host, bytes, [&](const void*& src, size_t& size) {
        const size_t n = s->pixels();
        const bool decision = which >= TRHIP_RESTIR_GI_INITIAL && which <= TRHIP_RESTIR_GI_FINAL;
        if (decision && !s->opt.record) return set_error("trhip_restir_gi_download: the decision records are only kept with record");
        switch (which) {
            case TRHIP_RESTIR_GI_SURFACE:      // the half the last frame wrote
                src = s->surface[(s->frame + 1u) & 1u]; size = n * sizeof(RestirSurface); break;
            case TRHIP_RESTIR_GI_CANONICAL: src = s->canonical; size = n * sizeof(RestirGiReservoir); break;
            case TRHIP_RESTIR_GI_HISTORY: src = s->history; size = n * sizeof(RestirGiReservoir); break;
            case TRHIP_RESTIR_GI_INITIAL: src = s->rec_initial; size = n * sizeof(RestirGiInitialRecord); break;
            case TRHIP_RESTIR_GI_SECONDARY: src = s->rec_secondary; size = n * sizeof(RestirSurface); break;
            case TRHIP_RESTIR_GI_LIGHT: src = s->rec_light; size = n * sizeof(RestirCandidateRecord); break;
            case TRHIP_RESTIR_GI_TEMPORAL: src = s->rec_temporal; size = n * sizeof(RestirTemporalRecord); break;
            case TRHIP_RESTIR_GI_SPATIAL:
                if (!s->rec_spatial) return set_error("trhip_restir_gi_download: the stage has no spatial samples");
                src = s->rec_spatial; size = n * s->opt.spatial_samples * sizeof(RestirSpatialRecord);
                break;
            case TRHIP_RESTIR_GI_FINAL: src = s->rec_final; size = n * sizeof(RestirFinalRecord); break;
            default: return set_error("trhip_restir_gi_download: unknown buffer");
        }
        return 0;
    });
}

}  // extern "C"
