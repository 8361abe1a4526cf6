// ReSTIR GI for gfx950 - reservoir resampling of indirect light, behind the entry points trhip_restir_gi_* of include/trhip.h.
//   k_restir_gi_initial    per pixel of every viewport: the first hit and its surface (first_hit.h), the surface record, one
//                          cosine-hemisphere ray and its closest hit x_s, x_s's surface, one light sample there with its shadow ray: the
//                          initial sample (x_s, n_s, L_o), its pdf and its target; the reprojected position for the temporal kernel
//   k_restir_gi_initial_path  (restir_gi_path.hip) the same with L_o continued from x_s over bounces - 1 further vertices, launched in
//                          k_restir_gi_initial's place by a stage with bounces > 1 (`path` of restir_gi.h)
//   k_restir_gi_temporal   no rays: the initial sample's resampling weight, the reprojection and the merge of the history reservoir
//   k_restir_gi_spatial    the neighbour search, the pairwise-MIS merge of the neighbours' canonical reservoirs (two shadow rays a
//                          neighbour), the chosen sample's shading (one more), the history reservoir and the colour added to `in`
// Constants, layouts, the order of operations and the order of random draws: restir_gi.h (and restir_di.h, whose rule it keeps).  The
// temporal and the spatial merge and the host skeleton are restir_resample.h's, shared with ReSTIR DI.  Three
// kernels, not DI's two: the initial kernel holds two closest-hit traversals and two shade_surface calls, and the merge that follows needs
// none of their registers.  IEEE fp32 without contraction in a fixed order, no atomics: two runs of the same inputs give the same bits.
#include <algorithm>
#include <string>
#include <vector>

#include "restir_gi_path.h"

namespace tr {
namespace {

using Kind = RestirGiKind;

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
    Kind::State r = Kind::create();                // the initial sample; uc_weight holds its pdf until the temporal kernel
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
                Kind::Eval e;
                r.target_function = rgb_to_luminance(Kind::contribution(sv, r.s, dom, e));
                irec.target = r.target_function;
            }
        }
    }
    if (overflow) *overflow_flag = 1;
    restir_store_surface(P.surface + pix, dom, hit.instance_id >= 0 ? hit.instance_id : -1);
    Kind::store(P.canonical + pix, r);
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
    Kind::State r = Kind::create();
    RestirTemporalRecord trec = restir_no_temporal();
    float iweight = 0.0f, idraw = 0.0f;
    bool iselected = false;
    if (instance_id >= 0) {
        LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, RESTIR_GI_SAMPLER_W}, 3u * P.frame + 1u, P.rng_seed, SAMPLER_UNIFORM);
        RestirReprojection rp;
        if (TEMPORAL) {      // the initial kernel's reprojection record
            const u4 w = restir_word(P.reproject + pix, 0);
            rp = restir_reproject<Kind>(L, P.has_history, P.prev_surface + layer * layer_px, P.history + layer * layer_px, dom,
                                        F2(__uint_as_float(w.x), __uint_as_float(w.y)), __uint_as_float(w.z), ls);
        }
        // DI's resampled_importance_sampling with one candidate: the initial sample, whose pdf the initial kernel left in uc_weight's place
        const Kind::State initial = Kind::load(P.canonical + pix);
        {
            const float mis_weight = 1.0f / (1.0f + rp.prev_confidence);
            const float target = initial.target_function, pdf = initial.uc_weight;
            float weight = mis_weight * target / pdf;
            if (isnan(weight)) weight = 0.0f;
            const float u = u4_to_unit(pcg4d(ls.rs)).x;
            const bool selected = restir_update(r, initial.s, weight, u);
            if (selected) r.target_function = target;
            r.confidence = r.confidence + 1.0f;
            iweight = weight; idraw = u; iselected = selected;
        }
        r.uc_weight = restir_uc_weight(r);
        if (TEMPORAL) restir_temporal_merge<Kind>(sv, L, rp, P.history + layer * layer_px, dom, P.max_confidence, ls, r, trec);
    }
    Kind::store(P.canonical + pix, r);
    if (P.rec_temporal) {
        restir_write_temporal(P.rec_temporal + pix, trec);
        restir_set_word(P.rec_initial + pix, 5, u4{TR_U(iweight), TR_U(idraw), iselected ? 1u : 0u, 0u});
    }
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
    RestirDomain dom;
    const int instance_id = restir_load_surface(P.surface + pix, dom);
    // `in` is not held across the merge (four registers where the kernels sit at 256): with spatial samples it is read where it is
    // added to; without, at the top, next to the other loads
    const auto read_in = [&] { return P.in ? P.in[pix] : F4(0.0f, 0.0f, 0.0f, 1.0f); };
    f4 in;
    if (SPATIAL == 0) in = read_in();
    int overflow = 0;
    if (instance_id < 0) {
        Kind::store(P.history + pix, Kind::create());
        P.out[pix] = SPATIAL == 0 ? in : read_in();
        restir_clear_records<SPATIAL>(P.rec_final, P.rec_spatial, pix);
        return;
    }
    const Kind::State canonical = Kind::load(P.canonical + pix);
    Kind::State r = canonical;
    RestirFinalRecord frec = {F3(0.0f), 0.0f, 0.0f, 0.0f, 0.0f, 0u};
    if (SPATIAL > 0) {
        const LocalSampler ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, RESTIR_GI_SAMPLER_W}, 3u * P.frame + 2u, P.rng_seed, SAMPLER_UNIFORM);
        const RestirMerged<Kind> m = restir_spatial_merge<Kind, TWO_LEVEL, SPATIAL>(sv, L, sv.cameras[viewport], P.search_radius, P.min_ray_dist,
            P.surface + layer * layer_px, P.canonical + layer * layer_px, P.rec_spatial, px, py, pix, dom, canonical, ls, s_stack + threadIdx.x, overflow);
        r = m.r; frec = m.frec; overflow = m.overflow;
    }
    Kind::Eval e;
    const f3 contrib = Kind::contribution(sv, r.s, dom, e);
    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, dom.pos, contrib, e.dir, e.dist2, s_stack + threadIdx.x, overflow);
    if (overflow) *overflow_flag = 1;
    const f3 shaded = contrib * visibility;
    Kind::store(P.history + pix, r);
    if (SPATIAL > 0) in = read_in();
    P.out[pix] = F4(F3(in) + shaded * r.uc_weight, in.w);
    frec.contribution = contrib; frec.visibility = visibility;
    if (P.rec_final) restir_write_final(P.rec_final + pix, frec);
}

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

constexpr const char* API = "trhip_restir_gi";

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_restir_gi : RestirStageHost<4> {
    trhip_restir_gi_options opt = {};
    RestirGiReservoir *canonical = nullptr, *history = nullptr;
    RestirGiReproject* reproject = nullptr;
    RestirGiInitialRecord* rec_initial = nullptr;
    RestirSurface* rec_secondary = nullptr;
    RestirCandidateRecord* rec_light = nullptr;
    uint32_t bounces = 1;                          // trhip_restir_gi_set_bounces
    RestirGiPathRecord* rec_path = nullptr;        // [pixels][bounces - 1]; null unless options.record and bounces > 1, as the one below
    RestirSurface* rec_path_surface = nullptr;
};

static_assert(sizeof(trhip_restir_gi_reservoir) == sizeof(RestirGiReservoir) && sizeof(trhip_restir_gi_initial) == sizeof(RestirGiInitialRecord) &&
              sizeof(trhip_restir_gi_path) == sizeof(RestirGiPathRecord), "downloads are the kernels' records");

extern "C" {

int trhip_restir_gi_create(trhip_device* dev, const trhip_restir_gi_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_restir_gi** out) {
    return restir_create(API, dev, opt, width, height, layers, out, [](const std::string&) { return 0; }, [&](trhip_restir_gi* s, size_t n) {
        s->alloc_zeroed(s->canonical, n * sizeof(RestirGiReservoir));
        s->alloc_zeroed(s->history, n * sizeof(RestirGiReservoir));
        if (opt->temporal_reuse) s->alloc_zeroed(s->reproject, n * sizeof(RestirGiReproject));
        if (opt->record) {
            s->alloc_zeroed(s->rec_initial, n * sizeof(RestirGiInitialRecord));
            s->alloc_zeroed(s->rec_secondary, n * sizeof(RestirSurface));
            s->alloc_zeroed(s->rec_light, n * sizeof(RestirCandidateRecord));
        }
    });
}

void trhip_restir_gi_destroy(trhip_restir_gi* s) { stage_destroy(s); }

int trhip_restir_gi_reset(trhip_restir_gi* s) { return restir_reset(API, s); }

int trhip_restir_gi_set_bounces(trhip_restir_gi* s, uint32_t bounces) {
    const std::string fn = std::string(API) + "_set_bounces";
    if (bounces < 1u || bounces > RESTIR_GI_MAX_BOUNCES) return set_error(fn + ": bounces " + std::to_string(bounces) + " is outside 1..8");
    if (!s) return set_error(fn + ": null stage");
    // a reservoir must not mix the samples of two estimators silently
    if (s->frame > 0 && bounces != s->bounces)
        return set_error(fn + ": the stage holds history of " + std::to_string(s->bounces) + " bounces: call " + API + "_reset first");
    if (bounces == s->bounces) return 0;
    if (s->opt.record) {     // the path records have one entry per extra vertex
        DEVCHK(s->hip_device);
        HIPCHK(hipDeviceSynchronize());
        for (void* old : {(void*)s->rec_path, (void*)s->rec_path_surface}) {
            if (!old) continue;
            s->allocations.erase(std::find(s->allocations.begin(), s->allocations.end(), old));
            HIPCHK(hipFree(old));
        }
        s->rec_path = nullptr; s->rec_path_surface = nullptr;
        s->bounces = 1;
        if (bounces > 1u) {
            const size_t n = s->pixels() * (bounces - 1u);
            s->alloc_zeroed(s->rec_path, n * sizeof(RestirGiPathRecord));
            s->alloc_zeroed(s->rec_path_surface, n * sizeof(RestirSurface));
            if (s->err == hipSuccess) s->err = hipDeviceSynchronize();
            if (s->err != hipSuccess) {
                const hipError_t e = s->err;
                s->err = hipSuccess;
                return set_error(fn + ": " + hipGetErrorString(e));
            }
        }
    }
    s->bounces = bounces;
    return 0;
}

int trhip_restir_gi_render(trhip_restir_gi* s, int projection, const uint32_t* viewports, uint32_t count, const void* in_color_dev, void* out_color_dev, void* stream) {
    DeviceScene* scene = nullptr;
    if (int r = restir_begin_render(API, s, viewports, count, out_color_dev, scene)) return r;
    RestirGiParams base{};
    restir_fill_params(base, *s, *scene);
    const bool temporal = s->opt.temporal_reuse != 0;
    const bool path = s->bounces > 1u;
    // restir_run_passes fills the parameters of every chunk of a pass, then the next pass's: the first `chunks` fills are the initial pass's
    constexpr uint32_t per_launch = sizeof(ViewportList::v) / sizeof(ViewportList::v[0]);
    const uint32_t chunks = (count + per_launch - 1u) / per_launch;
    uint32_t filled = 0;
    const RestirGiKernel kernels[3] = {
        path ? restir_gi_initial_path_kernel(scene->two_level)
             : (scene->two_level ? k_restir_gi_initial<true> : k_restir_gi_initial<false>),
        temporal ? k_restir_gi_temporal<true> : k_restir_gi_temporal<false>,
        scene->two_level ? spatial_kernel<true>(s->opt.spatial_samples) : spatial_kernel<false>(s->opt.spatial_samples)};
    return restir_run_passes(s, scene, projection, viewports, count, (hipStream_t)stream, base, kernels, 3, [&](RestirGiParams& P, size_t off) {
        P.canonical = s->canonical + off; P.history = s->history + off;
        P.reproject = s->reproject ? s->reproject + off : nullptr;
        P.in = in_color_dev ? (const f4*)in_color_dev + off : nullptr;
        P.out = (f4*)out_color_dev + off;
        P.rec_initial = s->rec_initial ? s->rec_initial + off : nullptr;
        P.rec_secondary = s->rec_secondary ? s->rec_secondary + off : nullptr;
        P.rec_light = s->rec_light ? s->rec_light + off : nullptr;
        if (path && filled++ < chunks)
            restir_gi_set_path_args(P, {s->bounces, s->rec_path ? s->rec_path + off * (s->bounces - 1u) : nullptr,
                                        s->rec_path_surface ? s->rec_path_surface + off * (s->bounces - 1u) : nullptr});
    });
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
    const int shared[4] = {TRHIP_RESTIR_GI_SURFACE, TRHIP_RESTIR_GI_TEMPORAL, TRHIP_RESTIR_GI_SPATIAL, TRHIP_RESTIR_GI_FINAL};
    const bool path = which == TRHIP_RESTIR_GI_PATH || which == TRHIP_RESTIR_GI_PATH_SURFACE;
    if (s && host && path && s->opt.record && s->bounces == 1u) return set_error(std::string(API) + "_download: a stage of one bounce has no path records");
    return restir_download(API, s, which, host, bytes, which >= TRHIP_RESTIR_GI_INITIAL && which <= TRHIP_RESTIR_GI_PATH_SURFACE, shared,
        [&](size_t n, const void*& src, size_t& size) {
            switch (which) {
                case TRHIP_RESTIR_GI_PATH: src = s->rec_path; size = n * (s->bounces - 1u) * sizeof(RestirGiPathRecord); return true;
                case TRHIP_RESTIR_GI_PATH_SURFACE: src = s->rec_path_surface; size = n * (s->bounces - 1u) * sizeof(RestirSurface); return true;
                case TRHIP_RESTIR_GI_CANONICAL: src = s->canonical; size = n * sizeof(RestirGiReservoir); return true;
                case TRHIP_RESTIR_GI_HISTORY: src = s->history; size = n * sizeof(RestirGiReservoir); return true;
                case TRHIP_RESTIR_GI_INITIAL: src = s->rec_initial; size = n * sizeof(RestirGiInitialRecord); return true;
                case TRHIP_RESTIR_GI_SECONDARY: src = s->rec_secondary; size = n * sizeof(RestirSurface); return true;
                case TRHIP_RESTIR_GI_LIGHT: src = s->rec_light; size = n * sizeof(RestirCandidateRecord); return true;
                default: return false;
            }
        });
}

}  // extern "C"
