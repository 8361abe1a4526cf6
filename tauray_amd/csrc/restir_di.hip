// ReSTIR DI for gfx950 - reservoir resampling of direct light, written after the reference's shader/restir_di.glsl,
// shader/restir_di_canonical_and_temporal.rgen and shader/restir_di_spatial.rgen, behind the entry points trhip_restir_di_* of include/trhip.h.
//   k_restir_di_canonical  per pixel of every viewport: the first hit and its surface (first_hit.h), the surface
//                          record, RIS over `candidates` light samples (per-target: a shadow ray in every target function), the temporal merge of
//                          the reprojected pixel's history reservoir
//   k_restir_di_spatial    per pixel: the neighbour search, the pairwise-MIS merge of the neighbours' canonical reservoirs (two shadow rays
//                          a neighbour in the per-target mode, none in the others), the chosen sample's shading (one more, in every
//                          mode), the history reservoir and the colour
// VISIBILITY (trhip_restir_di_set_visibility; `visibility modes` of restir_di.h) is a template parameter of both: 0, per-target, traces
// inside every target function; with 1 and 2 the candidate loop and the per-slot loop hold no traversal at all, 2 traces the candidates'
// choice once behind the loop.
// The power-proportional light selection (trhip_restir_di_set_light_selection; `light selection` of restir_di.h) has its canonical kernel
// and its weights kernel in restir_di_power.hip; its host side - the table, the setter, the refresh, the power mode's frame - is here.
// The BSDF-sampled candidates (trhip_restir_di_set_bsdf_candidates; `bsdf candidates` of restir_di.h) have their canonical kernel in
// restir_di_bsdf.hip; the setter, their two record buffers and their frame are here.
// Sphere lights as area lights (trhip_restir_di_set_sphere_lights; `sphere lights` of restir_di.h) have both their kernels in
// restir_di_sphere.hip; the setter and the area mode's frame are here.
// Constants, layouts, the order of operations and the order of random draws: restir_di.h.  The temporal and the spatial merge and the
// host skeleton are restir_resample.h's, shared with ReSTIR GI.  Both kernels are IEEE fp32, evaluated without
// contraction in a fixed order, no atomics: two runs of the same inputs give the same bits.  The front half is first_hit.h's, the one
// k_gbuffer and k_feature call.
#include <string>
#include <type_traits>
#include <vector>

#include "restir_di_sphere.h"
#include "../../include/tauray_alias.hh"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;
using Kind = RestirDiKind;

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
// The shared and the sampled mode's kernels take one pointer more; the per-target kernels keep the arguments, and with them the code, they had
struct RestirParamsSampled : RestirParams {
    RestirSampledRecord* rec_sampled;           // null unless options.record
};
template <int VISIBILITY>
using ParamsOf = std::conditional_t<VISIBILITY == 0, RestirParams, RestirParamsSampled>;

// tile_pixel's launch shape (first_hit.h).
// Two waves per SIMD: unbounded, the fp64 functions of RoundedMath took it to 256 VGPRs plus AGPR copies at one wave.
template <bool TWO_LEVEL, bool TEMPORAL, int VISIBILITY>
__global__ __launch_bounds__(KB, 2) void k_restir_di_canonical(SceneView sv, LaunchCtx L, int projection, ViewportList list, ParamsOf<VISIBILITY> P, uint* overflow_flag) {
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
        if (TEMPORAL) {      // get_reprojected_pixel before its rounding (restir_di.glsl:138-153)
            const f3 prev_pos = surface_prev_pos(sv, hit.instance_id, hit.primitive_id, hit.u, hit.v);
            const f3 m = get_camera_projection(sv.prev_cameras[viewport], projection, prev_pos);
            const f2 motion = F2(m.x, 1.0f - m.y) * F2((float)L.launch_w, (float)L.launch_h) - 0.5f;
            rp = restir_reproject<Kind>(L, P.has_history, P.prev_surface + layer * layer_px, P.history + layer * layer_px, dom, motion, length(ray_origin - dom.pos), ls);
        }

        // resampled_importance_sampling (restir_di_canonical_and_temporal.rgen:58-125)
        const float mis_weight = 1.0f / ((float)P.candidates + rp.prev_confidence);
        for (int i = 0; i < P.candidates; ++i) {
            const u4 rnd = pcg4d(ls.rs);
            RestirLightRecord Lr;
            float light_pdf;
            const RestirSample s = restir_sample_canonical(sv, P, rnd, dom.pos, Lr, light_pdf);
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
        // SAMPLE_VISIBILITY (restir_di_canonical_and_temporal.rgen:115-122): one ray for the sample the candidates chose.  Its direction
        // and distance come from evaluating it once more, the loop keeps neither
        // (the per-target instances are the code they were: they write no `sampled` record, the host holds its constant)
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
    } else if constexpr (VISIBILITY != 0) {      // no surface: the null sample
        if (P.rec_sampled) restir_set_word(P.rec_sampled + pix, 0, u4{TR_U(VISIBILITY == 2 ? 0.0f : 1.0f), 0u, 0u, 0u});
    }
    if (overflow) *overflow_flag = 1;
    restir_store_surface(P.surface + pix, dom, hit.instance_id >= 0 ? hit.instance_id : -1);
    Kind::store(P.canonical + pix, r);
    if (P.rec_temporal) restir_write_temporal(P.rec_temporal + pix, trec);
}

template <bool TWO_LEVEL, int SPATIAL, int VISIBILITY>
__global__ __launch_bounds__(KB, 2) void k_restir_di_spatial(SceneView sv, LaunchCtx L, int projection, ViewportList list, ParamsOf<VISIBILITY> P, uint* overflow_flag) {
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
    if (VISIBILITY == 2) r.uc_weight = r.uc_weight * visibility;      // restir_di_spatial.rgen:266-269: ahead of the history and of the colour
    Kind::store(P.history + pix, r);
    P.out[pix] = F4(shaded * r.uc_weight + dom.mat.emission, 1.0f);
    frec.contribution = contrib; frec.visibility = visibility;
    if (P.rec_final) restir_write_final(P.rec_final + pix, frec);
}

template <int VISIBILITY>
using RestirKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, ParamsOf<VISIBILITY>, uint*);

template <bool TWO_LEVEL, int VISIBILITY>
RestirKernel<VISIBILITY> canonical_kernel(bool temporal) {
    return temporal ? k_restir_di_canonical<TWO_LEVEL, true, VISIBILITY> : k_restir_di_canonical<TWO_LEVEL, false, VISIBILITY>;
}
template <bool TWO_LEVEL, int VISIBILITY>
RestirKernel<VISIBILITY> spatial_kernel(uint32_t spatial) {
    switch (spatial) {
        case 0: return k_restir_di_spatial<TWO_LEVEL, 0, VISIBILITY>;
        case 1: return k_restir_di_spatial<TWO_LEVEL, 1, VISIBILITY>;
        case 2: return k_restir_di_spatial<TWO_LEVEL, 2, VISIBILITY>;
        case 3: return k_restir_di_spatial<TWO_LEVEL, 3, VISIBILITY>;
        default: return k_restir_di_spatial<TWO_LEVEL, 4, VISIBILITY>;
    }
}

constexpr const char* API = "trhip_restir_di";

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_restir_di : RestirStageHost<3> {
    trhip_restir_di_options opt = {};
    RestirReservoir *canonical = nullptr, *history = nullptr;
    RestirCandidateRecord* rec_candidates = nullptr;
    RestirSampledRecord* rec_sampled = nullptr;      // per-target: (1, 0) on every pixel, written by fill_sampled_constant, no kernel
    int visibility = TRHIP_RESTIR_VISIBILITY_PER_TARGET;      // trhip_restir_di_set_visibility
    // trhip_restir_di_set_light_selection (restir_di.h `light selection`).  The weights and the table are the stage's own allocations, grown
    // with the scene's light count; host_weights are the weights the table was built from, table_points / table_tris its two classes.
    int selection = TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM;
    float uniform_fraction = 0.1f;
    float* light_weights = nullptr;
    AliasEntry* light_table = nullptr;
    size_t light_capacity = 0;
    bool has_table = false;
    uint32_t table_points = 0, table_tris = 0;
    std::vector<float> host_weights;
    // trhip_restir_di_set_bsdf_candidates (restir_di.h `bsdf candidates`).  With record and B > 0 the candidate records are [pixel][L + B]
    // in an allocation of the setter's, next to the records of download 10; opt.candidates stays L and rec_candidates the buffer of create.
    uint32_t bsdf_candidates = 0;
    RestirCandidateRecord* rec_candidates_bsdf = nullptr;
    RestirBsdfRecord* rec_bsdf = nullptr;
    int sphere_lights = TRHIP_RESTIR_SPHERE_LIGHTS_POINT;      // trhip_restir_di_set_sphere_lights (restir_di.h `sphere lights`)
    ~trhip_restir_di() { (void)hipFree(light_weights); (void)hipFree(light_table); (void)hipFree(rec_candidates_bsdf); (void)hipFree(rec_bsdf); }
};
static_assert(sizeof(alias_entry) == sizeof(AliasEntry), "the host builder's entry is the kernels'");

static_assert(sizeof(trhip_restir_di_surface) == sizeof(RestirSurface) && sizeof(trhip_restir_di_reservoir) == sizeof(RestirReservoir), "downloads are the kernels' records");
static_assert(sizeof(trhip_restir_di_candidate) == sizeof(RestirCandidateRecord) && sizeof(trhip_restir_di_temporal) == sizeof(RestirTemporalRecord), "downloads are the kernels' records");
static_assert(sizeof(trhip_restir_di_spatial) == sizeof(RestirSpatialRecord) && sizeof(trhip_restir_di_final) == sizeof(RestirFinalRecord), "downloads are the kernels' records");
static_assert(sizeof(trhip_restir_di_sampled) == sizeof(RestirSampledRecord) && sizeof(trhip_restir_di_bsdf_candidate) == sizeof(RestirBsdfRecord), "downloads are the kernels' records");
static_assert(sizeof(trhip_restir_di_options) == 32, "the options keep their size");

// The per-target mode's `sampled` record: no ray and nothing multiplied, (visibility 1, uc_weight_before 0) on every pixel.  Written where
// the mode is decided - at create and when the setter goes back to per-target - never in a frame.  Waits for the device.
static hipError_t fill_sampled_constant(trhip_restir_di* s) {
    const std::vector<RestirSampledRecord> ones(s->pixels(), RestirSampledRecord{1.0f, 0.0f, 0u, 0u});
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(s->rec_sampled, ones.data(), ones.size() * sizeof(RestirSampledRecord), hipMemcpyHostToDevice);
    return e;
}

// A frame in one visibility mode: a mode's instances hold only that mode's code
template <int VISIBILITY>
static int restir_di_render_mode(trhip_restir_di* s, DeviceScene* scene, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream) {
    ParamsOf<VISIBILITY> base{};
    base.candidates = (int)s->opt.candidates;
    restir_fill_params(base, *s, *scene);
    const bool temporal = s->opt.temporal_reuse != 0;
    const RestirKernel<VISIBILITY> kernels[2] = {
        scene->two_level ? canonical_kernel<true, VISIBILITY>(temporal) : canonical_kernel<false, VISIBILITY>(temporal),
        scene->two_level ? spatial_kernel<true, VISIBILITY>(s->opt.spatial_samples) : spatial_kernel<false, VISIBILITY>(s->opt.spatial_samples)};
    // The canonical kernels of every chunk first, then the spatial ones
    return restir_run_passes(s, scene, projection, viewports, count, (hipStream_t)stream, base, kernels, 2, [&](ParamsOf<VISIBILITY>& P, size_t off) {
        P.canonical = s->canonical + off; P.history = s->history + off;
        P.out = (f4*)out_color_dev + off;
        P.rec_candidates = s->rec_candidates ? s->rec_candidates + off * s->opt.candidates : nullptr;
        if constexpr (VISIBILITY != 0) P.rec_sampled = s->rec_sampled ? s->rec_sampled + off : nullptr;
    });
}

// A frame of the power mode: the canonical pass is restir_di_power.hip's kernel with a parameter block of its own, the spatial pass the
// instance the uniform mode launches (it never sees a candidate's pdf)
template <int VISIBILITY>
static int restir_di_render_power(trhip_restir_di* s, DeviceScene* scene, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    RestirPowerParams cbase{};
    cbase.candidates = (int)s->opt.candidates;
    restir_fill_params(cbase, *s, *scene);
    cbase.light_table = s->light_table;
    ParamsOf<VISIBILITY> sbase{};
    sbase.candidates = (int)s->opt.candidates;
    restir_fill_params(sbase, *s, *scene);
    const RestirPowerKernel canonical = restir_di_power_canonical_kernel(scene->two_level, s->opt.temporal_reuse != 0, VISIBILITY);
    const RestirKernel<VISIBILITY> spatial = scene->two_level ? spatial_kernel<true, VISIBILITY>(s->opt.spatial_samples) : spatial_kernel<false, VISIBILITY>(s->opt.spatial_samples);
    if (int r = restir_begin_frame(s, st)) return r;
    if (int r = restir_run_pass(s, scene, projection, viewports, count, st, cbase, canonical, 0, [&](RestirPowerParams& P, size_t off) {
            P.canonical = s->canonical + off; P.history = s->history + off;
            P.out = (f4*)out_color_dev + off;
            P.rec_candidates = s->rec_candidates ? s->rec_candidates + off * s->opt.candidates : nullptr;
            P.rec_sampled = VISIBILITY != 0 && s->rec_sampled ? s->rec_sampled + off : nullptr;
        })) return r;
    if (int r = restir_run_pass(s, scene, projection, viewports, count, st, sbase, spatial, 1, [&](ParamsOf<VISIBILITY>& P, size_t off) {
            P.canonical = s->canonical + off; P.history = s->history + off;
            P.out = (f4*)out_color_dev + off;
            P.rec_candidates = s->rec_candidates ? s->rec_candidates + off * s->opt.candidates : nullptr;
            if constexpr (VISIBILITY != 0) P.rec_sampled = s->rec_sampled ? s->rec_sampled + off : nullptr;
        })) return r;
    return restir_end_frame(s, viewports, count);
}

// A frame with BSDF candidates: the canonical pass is restir_di_bsdf.hip's kernel with a parameter block of its own - its POWER instances
// when the selection is power -, the spatial pass the instance every other frame launches
template <int VISIBILITY>
static int restir_di_render_bsdf(trhip_restir_di* s, DeviceScene* scene, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const bool power = s->selection == TRHIP_RESTIR_LIGHT_SELECTION_POWER;
    const size_t per_pixel = (size_t)s->opt.candidates + s->bsdf_candidates;
    RestirBsdfParams cbase{};
    cbase.candidates = (int)s->opt.candidates;
    cbase.bsdf_candidates = (int)s->bsdf_candidates;
    restir_fill_params(cbase, *s, *scene);
    cbase.light_table = power ? s->light_table : nullptr;
    ParamsOf<VISIBILITY> sbase{};
    sbase.candidates = (int)s->opt.candidates;
    restir_fill_params(sbase, *s, *scene);
    const RestirBsdfKernel canonical = restir_di_bsdf_canonical_kernel(scene->two_level, s->opt.temporal_reuse != 0, VISIBILITY, power);
    const RestirKernel<VISIBILITY> spatial = scene->two_level ? spatial_kernel<true, VISIBILITY>(s->opt.spatial_samples) : spatial_kernel<false, VISIBILITY>(s->opt.spatial_samples);
    if (int r = restir_begin_frame(s, st)) return r;
    if (int r = restir_run_pass(s, scene, projection, viewports, count, st, cbase, canonical, 0, [&](RestirBsdfParams& P, size_t off) {
            P.canonical = s->canonical + off; P.history = s->history + off;
            P.out = (f4*)out_color_dev + off;
            // both or neither: the kernel tests the first
            const bool rec = s->rec_candidates_bsdf && s->rec_bsdf;
            P.rec_candidates = rec ? s->rec_candidates_bsdf + off * per_pixel : nullptr;
            P.rec_bsdf = rec ? s->rec_bsdf + off * per_pixel : nullptr;
            P.rec_sampled = VISIBILITY != 0 && s->rec_sampled ? s->rec_sampled + off : nullptr;
        })) return r;
    if (int r = restir_run_pass(s, scene, projection, viewports, count, st, sbase, spatial, 1, [&](ParamsOf<VISIBILITY>& P, size_t off) {
            P.canonical = s->canonical + off; P.history = s->history + off;
            P.out = (f4*)out_color_dev + off;
            P.rec_candidates = nullptr;      // the spatial pass reads no candidate record
            if constexpr (VISIBILITY != 0) P.rec_sampled = s->rec_sampled ? s->rec_sampled + off : nullptr;
        })) return r;
    return restir_end_frame(s, viewports, count);
}

// A frame of the area mode (`sphere lights`): both passes are restir_di_sphere.hip's kernels over one parameter block; the canonical
// instance is chosen by the selection and by whether there are BSDF candidates, whose record buffers it then writes
static int restir_di_render_sphere(trhip_restir_di* s, DeviceScene* scene, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const bool power = s->selection == TRHIP_RESTIR_LIGHT_SELECTION_POWER, bsdf = s->bsdf_candidates > 0;
    const bool sampled = s->visibility != TRHIP_RESTIR_VISIBILITY_PER_TARGET;
    const size_t per_pixel = (size_t)s->opt.candidates + s->bsdf_candidates;
    RestirBsdfParams base{};
    base.candidates = (int)s->opt.candidates;
    base.bsdf_candidates = (int)s->bsdf_candidates;
    restir_fill_params(base, *s, *scene);
    base.light_table = power ? s->light_table : nullptr;
    const RestirSphereKernel canonical = restir_di_sphere_canonical_kernel(scene->two_level, s->opt.temporal_reuse != 0, s->visibility, power, bsdf);
    const RestirSphereKernel spatial = restir_di_sphere_spatial_kernel(scene->two_level, s->opt.spatial_samples, s->visibility);
    const auto fill = [&](RestirBsdfParams& P, size_t off) {
        P.canonical = s->canonical + off; P.history = s->history + off;
        P.out = (f4*)out_color_dev + off;
        if (bsdf) {      // both or neither: the kernel tests the first
            const bool rec = s->rec_candidates_bsdf && s->rec_bsdf;
            P.rec_candidates = rec ? s->rec_candidates_bsdf + off * per_pixel : nullptr;
            P.rec_bsdf = rec ? s->rec_bsdf + off * per_pixel : nullptr;
        } else {
            P.rec_candidates = s->rec_candidates ? s->rec_candidates + off * s->opt.candidates : nullptr;
            P.rec_bsdf = nullptr;
        }
        P.rec_sampled = sampled && s->rec_sampled ? s->rec_sampled + off : nullptr;
    };
    if (int r = restir_begin_frame(s, st)) return r;
    if (int r = restir_run_pass(s, scene, projection, viewports, count, st, base, canonical, 0, fill)) return r;
    if (int r = restir_run_pass(s, scene, projection, viewports, count, st, base, spatial, 1, fill)) return r;
    return restir_end_frame(s, viewports, count);
}

// The table of the power mode from the scene's lights as they are now: the weights kernel, a download, the host builder
// (tauray_alias.hh), an upload.  Waits for the device, twice: a frame in flight reads the table.  force = false skips the build when
// the weights are byte-equal to those the table holds.
static int build_light_table(trhip_restir_di* s, const std::string& fn, bool force, uint32_t* rebuilt) {
    if (rebuilt) *rebuilt = 0;
    DEVCHK(s->hip_device);
    DeviceScene* scene = device_scene(s->dev);
    if (int r = check_scene_ready(fn.c_str(), scene->instance_count, scene->accel_built)) return r;
    const uint32_t n_point = scene->point_light_count, n_tri = scene->tri_light_count;
    const size_t n = (size_t)n_point + n_tri;
    if (n > s->light_capacity || !s->light_table) {
        HIPCHK(hipDeviceSynchronize());
        (void)hipFree(s->light_weights); (void)hipFree(s->light_table);
        s->light_weights = nullptr; s->light_table = nullptr; s->light_capacity = 0; s->has_table = false;
        const size_t cap = n > 0 ? n : 1;
        HIPCHK(hipMalloc((void**)&s->light_weights, cap * sizeof(float)));
        HIPCHK(hipMalloc((void**)&s->light_table, cap * sizeof(AliasEntry)));
        s->light_capacity = cap;
    }
    std::vector<float> weights(n);
    HIPCHK(restir_launch_light_weights(scene->view(), s->light_weights, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(weights.data(), s->light_weights, n * sizeof(float), hipMemcpyDeviceToHost));
    if (!force && s->has_table && n_point == s->table_points && n_tri == s->table_tris &&
        (n == 0 || memcmp(weights.data(), s->host_weights.data(), n * sizeof(float)) == 0)) return 0;
    const std::vector<alias_entry> table = build_light_selection_table(weights.data(), n_point, n_tri, s->uniform_fraction);
    if (n) HIPCHK(hipMemcpy(s->light_table, table.data(), n * sizeof(alias_entry), hipMemcpyHostToDevice));
    s->host_weights = weights;
    s->table_points = n_point; s->table_tris = n_tri; s->has_table = true;
    if (rebuilt) *rebuilt = 1;
    return 0;
}

extern "C" {

int trhip_restir_di_create(trhip_device* dev, const trhip_restir_di_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_restir_di** out) {
    return restir_create(API, dev, opt, width, height, layers, out,
        [&](const std::string& fn) {
            if (opt->candidates < 1 || opt->candidates > (uint32_t)RESTIR_MAX_CANDIDATES)
                return set_error(fn + ": candidates " + std::to_string(opt->candidates) + " is outside 1..32");
            return 0;
        },
        [&](trhip_restir_di* s, size_t n) {
            s->alloc_zeroed(s->canonical, n * sizeof(RestirReservoir));
            s->alloc_zeroed(s->history, n * sizeof(RestirReservoir));
            if (opt->record) {
                s->alloc_zeroed(s->rec_candidates, n * opt->candidates * sizeof(RestirCandidateRecord));
                s->alloc_zeroed(s->rec_sampled, n * sizeof(RestirSampledRecord));
                if (s->err == hipSuccess) s->err = fill_sampled_constant(s);      // a stage is created per-target
            }
        });
}

void trhip_restir_di_destroy(trhip_restir_di* s) { stage_destroy(s); }

int trhip_restir_di_reset(trhip_restir_di* s) { return restir_reset(API, s); }

int trhip_restir_di_set_visibility(trhip_restir_di* s, int mode) {
    static const char* const names[3] = {"per-target", "shared", "sampled"};
    const std::string fn = std::string(API) + "_set_visibility";
    if (!s) return set_error(fn + ": null stage");
    if (mode < TRHIP_RESTIR_VISIBILITY_PER_TARGET || mode > TRHIP_RESTIR_VISIBILITY_SAMPLED) return set_error(fn + ": mode " + std::to_string(mode) + " is outside 0..2");
    // a reservoir must not mix the samples of two target functions silently
    if (s->frame > 0 && mode != s->visibility)
        return set_error(fn + ": the stage holds history of the " + names[s->visibility] + " mode: call " + API + "_reset first");
    if (mode == TRHIP_RESTIR_VISIBILITY_PER_TARGET && mode != s->visibility && s->rec_sampled) {      // the other modes' kernels wrote the record
        DEVCHK(s->hip_device);
        HIPCHK(fill_sampled_constant(s));
    }
    s->visibility = mode;
    return 0;
}

int trhip_restir_di_set_light_selection(trhip_restir_di* s, int mode, float uniform_fraction) {
    static const char* const names[2] = {"uniform", "power"};
    const std::string fn = std::string(API) + "_set_light_selection";
    if (!s) return set_error(fn + ": null stage");
    if (mode < TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM || mode > TRHIP_RESTIR_LIGHT_SELECTION_POWER) return set_error(fn + ": mode " + std::to_string(mode) + " is outside 0..1");
    if (!(uniform_fraction > 0.0f) || !(uniform_fraction <= 1.0f)) return set_error(fn + ": uniform_fraction must be in (0, 1]");
    // a reservoir's uc_weight must not mix two candidate distributions silently
    if (s->frame > 0 && (mode != s->selection || uniform_fraction != s->uniform_fraction))
        return set_error(fn + ": the stage holds history of the " + names[s->selection] + " selection with uniform_fraction " + std::to_string(s->uniform_fraction) +
                         ": call " + API + "_reset first");
    if (mode == TRHIP_RESTIR_LIGHT_SELECTION_POWER) {
        const float before = s->uniform_fraction;
        s->uniform_fraction = uniform_fraction;
        if (int r = build_light_table(s, fn, true, nullptr)) { s->uniform_fraction = before; return r; }
    }
    s->uniform_fraction = uniform_fraction;
    s->selection = mode;
    return 0;
}

int trhip_restir_di_set_bsdf_candidates(trhip_restir_di* s, uint32_t n) {
    const std::string fn = std::string(API) + "_set_bsdf_candidates";
    if (!s) return set_error(fn + ": null stage");
    if (n > (uint32_t)RESTIR_MAX_BSDF_CANDIDATES) return set_error(fn + ": bsdf_candidates " + std::to_string(n) + " is outside 0..8");
    if (s->opt.candidates + n > (uint32_t)RESTIR_MAX_CANDIDATES)
        return set_error(fn + ": candidates " + std::to_string(s->opt.candidates) + " + bsdf_candidates " + std::to_string(n) + " is above 32");
    // uc_weight must not mix two candidate distributions silently (as decisions 22 and 27)
    if (s->frame > 0 && n != s->bsdf_candidates)
        return set_error(fn + ": the stage holds history of " + std::to_string(s->bsdf_candidates) + " bsdf candidates: call " + API + "_reset first");
    if (n != s->bsdf_candidates && s->opt.record) {      // the records of L + n candidates a pixel; a frame in flight writes the old ones
        DEVCHK(s->hip_device);
        HIPCHK(hipDeviceSynchronize());
        (void)hipFree(s->rec_candidates_bsdf); (void)hipFree(s->rec_bsdf);
        s->rec_candidates_bsdf = nullptr; s->rec_bsdf = nullptr;
        s->bsdf_candidates = 0;      // what the stage is left with when the allocation fails
        if (n > 0) {
            const size_t records = s->pixels() * ((size_t)s->opt.candidates + n);
            hipError_t e = hipMalloc((void**)&s->rec_candidates_bsdf, records * sizeof(RestirCandidateRecord));
            if (e == hipSuccess) e = hipMalloc((void**)&s->rec_bsdf, records * sizeof(RestirBsdfRecord));
            if (e == hipSuccess) e = hipMemset(s->rec_candidates_bsdf, 0, records * sizeof(RestirCandidateRecord));
            if (e == hipSuccess) e = hipMemset(s->rec_bsdf, 0, records * sizeof(RestirBsdfRecord));
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) {
                (void)hipFree(s->rec_candidates_bsdf); (void)hipFree(s->rec_bsdf);
                s->rec_candidates_bsdf = nullptr; s->rec_bsdf = nullptr;
                return set_error(fn + ": " + hipGetErrorString(e));
            }
        }
    }
    s->bsdf_candidates = n;
    return 0;
}

int trhip_restir_di_set_sphere_lights(trhip_restir_di* s, int mode) {
    static const char* const names[2] = {"point", "area"};
    const std::string fn = std::string(API) + "_set_sphere_lights";
    if (!s) return set_error(fn + ": null stage");
    if (mode < TRHIP_RESTIR_SPHERE_LIGHTS_POINT || mode > TRHIP_RESTIR_SPHERE_LIGHTS_AREA) return set_error(fn + ": mode " + std::to_string(mode) + " is outside 0..1");
    // a reservoir must not mix the samples of two meanings of light_data silently
    if (s->frame > 0 && mode != s->sphere_lights)
        return set_error(fn + ": the stage holds history of the " + names[s->sphere_lights] + " mode: call " + API + "_reset first");
    s->sphere_lights = mode;
    return 0;
}

int trhip_restir_di_refresh_light_selection(trhip_restir_di* s, uint32_t* rebuilt) {
    const std::string fn = std::string(API) + "_refresh_light_selection";
    if (rebuilt) *rebuilt = 0;
    if (!s) return set_error(fn + ": null stage");
    if (s->selection != TRHIP_RESTIR_LIGHT_SELECTION_POWER) return 0;
    return build_light_table(s, fn, false, rebuilt);
}

int trhip_restir_di_render(trhip_restir_di* s, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream) {
    DeviceScene* scene = nullptr;
    if (int r = restir_begin_render(API, s, viewports, count, out_color_dev, scene)) return r;
    const bool power = s->selection == TRHIP_RESTIR_LIGHT_SELECTION_POWER;
    if (power) {
        if (scene->point_light_count != s->table_points || scene->tri_light_count != s->table_tris)
            return set_error(std::string(API) + "_render: the scene has " + std::to_string(scene->point_light_count) + " point and " + std::to_string(scene->tri_light_count) +
                             " triangle lights, the light selection table was built for " + std::to_string(s->table_points) + " and " + std::to_string(s->table_tris) +
                             ": call " + API + "_refresh_light_selection first");
    }
    if (s->sphere_lights == TRHIP_RESTIR_SPHERE_LIGHTS_AREA) return restir_di_render_sphere(s, scene, projection, viewports, count, out_color_dev, stream);
    if (s->bsdf_candidates > 0) {
        switch (s->visibility) {
            case TRHIP_RESTIR_VISIBILITY_PER_TARGET: return restir_di_render_bsdf<0>(s, scene, projection, viewports, count, out_color_dev, stream);
            case TRHIP_RESTIR_VISIBILITY_SHARED: return restir_di_render_bsdf<1>(s, scene, projection, viewports, count, out_color_dev, stream);
            default: return restir_di_render_bsdf<2>(s, scene, projection, viewports, count, out_color_dev, stream);
        }
    }
    if (power) {
        switch (s->visibility) {
            case TRHIP_RESTIR_VISIBILITY_PER_TARGET: return restir_di_render_power<0>(s, scene, projection, viewports, count, out_color_dev, stream);
            case TRHIP_RESTIR_VISIBILITY_SHARED: return restir_di_render_power<1>(s, scene, projection, viewports, count, out_color_dev, stream);
            default: return restir_di_render_power<2>(s, scene, projection, viewports, count, out_color_dev, stream);
        }
    }
    switch (s->visibility) {
        case TRHIP_RESTIR_VISIBILITY_PER_TARGET: return restir_di_render_mode<0>(s, scene, projection, viewports, count, out_color_dev, stream);
        case TRHIP_RESTIR_VISIBILITY_SHARED: return restir_di_render_mode<1>(s, scene, projection, viewports, count, out_color_dev, stream);
        default: return restir_di_render_mode<2>(s, scene, projection, viewports, count, out_color_dev, stream);
    }
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
    const int shared[4] = {TRHIP_RESTIR_DI_SURFACE, TRHIP_RESTIR_DI_TEMPORAL, TRHIP_RESTIR_DI_SPATIAL, TRHIP_RESTIR_DI_FINAL};
    // the weights and the table of the power mode are no decision records: they are there with and without `record`
    if (s && (which == TRHIP_RESTIR_DI_LIGHT_WEIGHTS || which == TRHIP_RESTIR_DI_LIGHT_TABLE) && !(s->selection == TRHIP_RESTIR_LIGHT_SELECTION_POWER && s->has_table))
        return set_error(std::string(API) + "_download: the stage has no light selection table (" + API + "_set_light_selection)");
    if (s && which == TRHIP_RESTIR_DI_BSDF_CANDIDATES && s->opt.record && s->bsdf_candidates == 0)
        return set_error(std::string(API) + "_download: the stage has no bsdf candidates (" + API + "_set_bsdf_candidates)");
    const bool decision = (which >= TRHIP_RESTIR_DI_CANDIDATES && which <= TRHIP_RESTIR_DI_SAMPLED) || which == TRHIP_RESTIR_DI_BSDF_CANDIDATES;
    return restir_download(API, s, which, host, bytes, decision, shared,
        [&](size_t n, const void*& src, size_t& size) {
            switch (which) {
                case TRHIP_RESTIR_DI_CANONICAL: src = s->canonical; size = n * sizeof(RestirReservoir); return true;
                case TRHIP_RESTIR_DI_HISTORY: src = s->history; size = n * sizeof(RestirReservoir); return true;
                case TRHIP_RESTIR_DI_SAMPLED: src = s->rec_sampled; size = n * sizeof(RestirSampledRecord); return true;
                case TRHIP_RESTIR_DI_LIGHT_WEIGHTS: src = s->light_weights; size = ((size_t)s->table_points + s->table_tris) * sizeof(float); return true;
                case TRHIP_RESTIR_DI_LIGHT_TABLE: src = s->light_table; size = ((size_t)s->table_points + s->table_tris) * sizeof(AliasEntry); return true;
                case TRHIP_RESTIR_DI_CANDIDATES:      // [pixel][L + B]: with B > 0 the setter's buffer
                    src = s->bsdf_candidates ? s->rec_candidates_bsdf : s->rec_candidates;
                    size = n * ((size_t)s->opt.candidates + s->bsdf_candidates) * sizeof(RestirCandidateRecord); return true;
                case TRHIP_RESTIR_DI_BSDF_CANDIDATES: src = s->rec_bsdf; size = n * ((size_t)s->opt.candidates + s->bsdf_candidates) * sizeof(RestirBsdfRecord); return true;
                default: return false;
            }
        });
}

}  // extern "C"
