// SH probe-grid baking for gfx950: sh_path_tracer_stage + sh_compact_stage (src/sh_path_tracer_stage.{hh,cc}, shader/sh_path_tracer.rgen,
// src/sh_grid.{hh,cc}, shader/sh_compact.comp restated) behind the entry points trhip_sh_* of include/trhip.h - the server half of the
// reference's DDISH-GI.  A grid is rendered in batches of whole probes; per batch
//   k_sh_raygen -> the bounce loop of PtStage::render (k_trace_* and the general k_shade, lanes and fused launches as for a frame, with
//   hidden lights and the first-bounce clamp) -> k_sh_project
// k_sh_raygen fills the path state of every (probe, sample) of the batch; k_sh_project sums a probe's samples onto the SH basis in a fixed
// tree, blends with the stage's history and writes the RGBA32F grid and its RGBA16F copy (sh_compact).  Constants, layouts, the path ids
// and the order of operations: sh_probes.h.  Both kernels are IEEE fp32, evaluated without contraction in a fixed order, no float
// atomics: the grids depend on neither the batches nor the lanes nor the path-id order.  Built with the flags of api.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "pt_state.h"
#include "pt.h"
#include "sh_probes.h"
#include "stage_host.h"

namespace tr {
namespace {

// sh_path_tracer.rgen:52-77 for path i of the launch: sampler, probe-space offset, position, direction; then the start of evaluate_ray
// (path_tracer.glsl:376-384) as k_raygen leaves it
__global__ __launch_bounds__(KB) void k_sh_raygen(PtParams P, PathBuffers pb, ShProbeBatch B) {
    if (blockIdx.x == 0) for (uint k = threadIdx.x; k < P.bounce_words; k += KB) pb.bounce[k] = 0;   // queue lengths and work cursors, as k_raygen
    uint i = blockIdx.x * KB + threadIdx.x;
    if (i >= P.n_ids) return;
    i += P.id_offset;
    uint q, s;
    sh_path_of_id(B, i, q, s);
    const ShGridData& G = B.grid;
    const uint p = B.probe_base + q;
    const uint x = p % G.grid_size[0], y = (p / G.grid_size[0]) % G.grid_size[1], z = p / (G.grid_size[0] * G.grid_size[1]);
    LocalSampler ls = init_local_sampler(u4{x, y, z, s}, B.sample_counter, B.rng_seed, SAMPLER_UNIFORM);
    f3 offset = F3(0.0f);
    if (P.opt.film != 0) {
        const f4 r = u4_to_unit(pcg4d(ls.rs));      // generate_spatial_sample
        if (P.opt.film == 1) offset = F3(r.x, r.y, r.z) * 2.0f - 1.0f;
        else {      // sample_blackman_harris_ball (math.glsl:329-334)
            const float cos_theta = 2.0f * r.x - 1.0f, sin_theta = sqrtf(1.0f - cos_theta * cos_theta), phi = (r.y * 2.0f) * SH_PI;
            const f3 v = F3(sh_cos(phi) * sin_theta, sh_sin(phi) * sin_theta, cos_theta);
            // sample_blackman_harris (math.glsl:220-228)
            float u = r.z;
            const bool flip = u > 0.5f;
            u = flip ? 1.0f - u : u;
            const float bh = ((((0.29627329f * u + -0.33518669f * sh_pow(u, 0.5f)) + -0.51620529f * sh_pow(u, 0.3333333333f)) + 1.87406934f * sh_pow(u, 0.25f)) +
                              -0.66315464f * sh_pow(u, 0.2f));
            const float sb = flip ? 1.0f - bh : bh;
            offset = v * sh_pow(fabsf(2.0f * sb - 1.0f), 1.0f / 3.0f);
        }
    }
    const f3 cell = F3((float)x, (float)y, (float)z);
    const f3 res = F3((float)G.grid_size[0], (float)G.grid_size[1], (float)G.grid_size[2]);
    const f3 local = (((cell + offset * P.opt.film_radius) + 0.5f) / res) * 2.0f - 1.0f;
    const f3 origin = F3(((G.transform.c[0] * local.x + G.transform.c[1] * local.y) + G.transform.c[2] * local.z) + G.transform.c[3] * 1.0f);
    const f3 ldir = sh_local_dir(s, B.samples, G.rotation_x, G.rotation_y);
    const f3 dir = normalize((G.normal_transform.c[0] * ldir.x + G.normal_transform.c[1] * ldir.y) + G.normal_transform.c[2] * ldir.z);
    u4 misc = {0, 0, i, 0};
    misc.x = pcg4d(ls.rs).x;      // payload.random_seed = pcg4d(lsampler.rs.seed).x  (path_tracer.glsl:384)
    pb.org_pdf[i] = F4(origin, 0.0f);            // bsdf_pdf = 0
    pb.dir_reg[i] = F4(dir, 1.0f);               // regularization = 1
    pb.atten_alpha[i] = F4(1, 1, 1, 1);          // attenuation = 1
    pb.rng[i] = ls.rs;
    pb.misc[i] = misc;
}

struct ShProjectParams {
    ShProbeBatch batch;
    float coef_mult;
    const f4* previous;      // the float grid before this render (read only while mix_ratio < 1); may be `grid` itself: a probe's entries are its block's
    f4* grid;
    __half* grid_half;       // four halfs per entry
};

// One workgroup per probe of the batch: sh_path_tracer.rgen:88-110 with the sum over the samples in the tree of sh_probes.h, then sh_compact.
template <int ORDER>
__global__ __launch_bounds__(SH_BLOCK) void k_sh_project(PathBuffers pb, ShProjectParams P) {
    constexpr int C = (ORDER + 1) * (ORDER + 1);
    __shared__ f4 s_part[SH_BLOCK / 64][C];
    const ShGridData& G = P.batch.grid;
    const uint q = blockIdx.x, n = P.batch.samples;
    f4 acc[C];
#pragma unroll
    for (int l = 0; l < C; ++l) acc[l] = F4(0.0f);
    for (uint s = threadIdx.x; s < n; s += SH_BLOCK) {
        const uint id = sh_id_of_path(P.batch, q, s);
        const f4 d = pb.diffuse[id], r = pb.reflection[id], fm = pb.first_mat[id];
        const float first_dist = pb.first_dist[id];
        // modulate_color(first_hit_material, diffuse.rgb, reflection.rgb) (material.glsl:57-65)
        const f3 albedo = F3(fm);
        const float metallic = fm.w, approx_fresnel = 0.02f;
        const f3 dd = F3(d) * albedo * (1.0f - metallic);
        const f3 rr = F3(r) * mix3(F3(approx_fresnel), albedo, metallic) / mixf(approx_fresnel, 1.0f, metallic);
        const f3 value = dd + rr;
        const f3 ldir = sh_local_dir(s, n, G.rotation_x, G.rotation_y);
        const float dist = clampf(first_dist * length(ldir * G.cell_scale), 0.0f, sqrtf(3.0f));
        const f4 coefs = F4(value, dist) * P.coef_mult;
        float basis[C];
        sh_basis<ORDER>(ldir, basis);
#pragma unroll
        for (int l = 0; l < C; ++l) acc[l] = acc[l] + coefs * basis[l];
    }
    const uint lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int l = 0; l < C; ++l) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            acc[l].x = acc[l].x + __shfl_xor(acc[l].x, off); acc[l].y = acc[l].y + __shfl_xor(acc[l].y, off);
            acc[l].z = acc[l].z + __shfl_xor(acc[l].z, off); acc[l].w = acc[l].w + __shfl_xor(acc[l].w, off);
        }
        if (lane == 0) s_part[wave][l] = acc[l];
    }
    __syncthreads();
    if (threadIdx.x >= (uint)C) return;
    const uint l = threadIdx.x;
    f4 out = (s_part[0][l] + s_part[1][l]) + (s_part[2][l] + s_part[3][l]);
    const uint p = P.batch.probe_base + q;
    const uint rx = G.grid_size[0], ry = G.grid_size[1];
    const uint x = p % rx, y = (p / rx) % ry, z = p / (rx * ry);
    const size_t e = ((size_t)z * ((size_t)ry * C) + (y + l * ry)) * rx + x;
    if (G.mix_ratio < 1.0f) out = mix4(P.previous[e], out, G.mix_ratio);
    P.grid[e] = out;
    __half* h = P.grid_half + e * 4;
    h[0] = __float2half_rn(out.x); h[1] = __float2half_rn(out.y); h[2] = __float2half_rn(out.z); h[3] = __float2half_rn(out.w);
}
static_assert(SH_BLOCK == 256, "k_sh_project combines four waves of 64");

}  // namespace

void launch_sh_raygen(uint blocks, hipStream_t stream, const PtParams& P, const PathBuffers& pb, const ShProbeBatch& batch) {
    hipLaunchKernelGGL(k_sh_raygen, dim3(blocks), dim3(KB), 0, stream, P, pb, batch);
}

}  // namespace tr

using namespace tr;

struct trhip_sh : StageHost<2> {
    std::vector<hipEvent_t> project_events;      // detailed timing: a pair around every k_sh_project launch of the last render
    size_t timed_events = 0;
    trhip_device* dev = nullptr;
    PtStage* pt = nullptr;
    trhip_sh_options opt = {};
    trhip_pt_options path = {};
    m4 transform = {{F4(1, 0, 0, 0), F4(0, 1, 0, 0), F4(0, 0, 1, 0), F4(0, 0, 0, 1)}};
    f3 scaling = F3(1.0f);
    uint32_t frame_counter = 0, history_length = 0, batch_probes = 0;
    f4* grid = nullptr;
    __half* grid_half = nullptr;
    hipStream_t last_stream = nullptr;
    ~trhip_sh() { delete pt; for (hipEvent_t e : project_events) (void)hipEventDestroy(e); }
    int coefs() const { return (opt.order + 1) * (opt.order + 1); }
    size_t probes() const { return (size_t)opt.resolution[0] * opt.resolution[1] * opt.resolution[2]; }
    size_t entries() const { return probes() * (size_t)coefs(); }
};

namespace {

// grid_data_buffer (sh_path_tracer_stage::update, src/sh_path_tracer_stage.cc:115-137), in float like the reference's host
ShGridData pack_grid_data(const m4& transform, f3 scaling, const uint32_t resolution[3], uint32_t samples, uint32_t frame_counter, uint32_t history_length,
                          float temporal_ratio) {
    ShGridData g{};
    g.transform = transform;
    g.normal_transform = matrix_orientation(transform);
    for (int i = 0; i < 3; ++i) g.grid_size[i] = resolution[i];
    const float inv_history = 1.0f / (float)history_length;
    g.mix_ratio = inv_history > temporal_ratio ? inv_history : temporal_ratio;
    g.cell_scale = F3((0.5f * (float)resolution[0]) / scaling.x, (0.5f * (float)resolution[1]) / scaling.y, (0.5f * (float)resolution[2]) / scaling.z);
    uint c0 = frame_counter * samples, c1 = c0 + 1u;
    g.rotation_x = (float)pcg(c0) / (float)0xFFFFFFFFu;
    g.rotation_y = (float)pcg(c1) / (float)0xFFFFFFFFu;
    return g;
}
ShGridData grid_data_of(const trhip_sh* s, uint32_t history_length) {
    return pack_grid_data(s->transform, s->scaling, s->opt.resolution, s->opt.samples_per_probe, s->frame_counter, history_length, s->opt.temporal_ratio);
}
void unpack_grid_data(const ShGridData& g, trhip_sh_grid_data* out) {
    memset(out, 0, sizeof(*out));
    memcpy(out->transform, &g.transform, sizeof(out->transform));
    for (int c = 0; c < 3; ++c) { out->normal_transform[4 * c] = g.normal_transform.c[c].x; out->normal_transform[4 * c + 1] = g.normal_transform.c[c].y; out->normal_transform[4 * c + 2] = g.normal_transform.c[c].z; }
    out->normal_transform[15] = 1.0f;
    for (int i = 0; i < 3; ++i) out->grid_size[i] = g.grid_size[i];
    out->mix_ratio = g.mix_ratio;
    out->cell_scale[0] = g.cell_scale.x; out->cell_scale[1] = g.cell_scale.y; out->cell_scale[2] = g.cell_scale.z;
    out->rotation_x = g.rotation_x; out->rotation_y = g.rotation_y;
}

}  // namespace

extern "C" {

int trhip_sh_create(trhip_device* dev, const trhip_pt_options* path, const trhip_sh_options* opt, trhip_sh** out) {
    if (!out) return set_error("trhip_sh_create: null out");
    *out = nullptr;
    if (!path || !opt) return set_error("trhip_sh_create: null options");
    if (opt->resolution[0] == 0 || opt->resolution[1] == 0 || opt->resolution[2] == 0) return set_error("trhip_sh_create: zero resolution");
    if (opt->resolution[0] > 1024 || opt->resolution[1] > 1024 || opt->resolution[2] > 1024) return set_error("trhip_sh_create: resolution above 1024 on an axis");
    if (opt->order < 0 || opt->order > SH_MAX_ORDER) return set_error("trhip_sh_create: order " + std::to_string(opt->order) + " is outside 0..4");
    if (opt->samples_per_probe < 1) return set_error("trhip_sh_create: samples_per_probe must be >= 1");
    if (opt->samples_per_probe > SH_MAX_BATCH_PATHS)
        return set_error("trhip_sh_create: samples_per_probe above " + std::to_string(SH_MAX_BATCH_PATHS) + ": a batch holds whole probes");
    if (!(opt->temporal_ratio >= 0.0f) || !(opt->temporal_ratio <= 1.0f)) return set_error("trhip_sh_create: temporal_ratio must be in [0, 1]");
    if (path->sampler != 0)
        return set_error("trhip_sh_create: sampler " + std::to_string(path->sampler) + ": only sampler = 0 (uniform-random) is accepted; the Sobol samplers take their index from a pixel launch");
    if (path->max_bounces < 1) return set_error("trhip_sh_create: max_bounces must be >= 1");
    if (path->film < 0 || path->film > 2) return set_error("trhip_sh_create: unknown film " + std::to_string(path->film));
    if (!dev) return set_error("trhip_sh_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_sh* s = new trhip_sh;
    s->dev = dev; s->hip_device = device_index(dev);
    s->opt = *opt;
    // the path options the stage reads (include/trhip.h); everything else is what sh_path_tracer.rgen compiles in
    trhip_pt_options& o = s->path;
    o = trhip_pt_options{};
    o.max_bounces = path->max_bounces; o.min_ray_dist = path->min_ray_dist; o.rng_seed = path->rng_seed; o.sampler = 0;
    o.samples_per_pixel = 1; o.samples_per_pass = 1;
    o.film = path->film; o.film_radius = path->film_radius; o.mis_mode = path->mis_mode; o.russian_roulette_delta = path->russian_roulette_delta;
    o.indirect_clamping = path->indirect_clamping; o.regularization_gamma = path->regularization_gamma;
    o.nee_point = path->nee_point; o.nee_directional = path->nee_directional; o.nee_envmap = path->nee_envmap; o.nee_triangles = path->nee_triangles;
    o.bounce_mode = path->bounce_mode; o.tri_light_mode = path->tri_light_mode;
    o.hide_lights = 1;
    s->pt = new PtStage(device_scene(dev), o);
    s->pt->probe_mode = true;
    s->alloc_zeroed(s->grid, s->entries() * sizeof(f4));
    s->alloc_zeroed(s->grid_half, s->entries() * 4 * sizeof(__half));
    return stage_finish_create("trhip_sh_create", s, out);
}

void trhip_sh_destroy(trhip_sh* s) { stage_destroy(s); }

int trhip_sh_set_transform(trhip_sh* s, const float transform[16], const float scaling[3]) {
    if (!s || !transform || !scaling) return set_error("trhip_sh_set_transform: null argument");
    for (int i = 0; i < 16; ++i) if (!std::isfinite(transform[i])) return set_error("trhip_sh_set_transform: the transform is not finite");
    for (int i = 0; i < 3; ++i) if (!std::isfinite(scaling[i]) || scaling[i] == 0.0f) return set_error("trhip_sh_set_transform: the scaling is not finite or zero");
    for (int c = 0; c < 3; ++c)
        if (transform[4 * c] == 0.0f && transform[4 * c + 1] == 0.0f && transform[4 * c + 2] == 0.0f)
            return set_error("trhip_sh_set_transform: the transform has a zero axis");
    memcpy(&s->transform, transform, sizeof(m4));
    s->scaling = F3(scaling[0], scaling[1], scaling[2]);
    return 0;
}

int trhip_sh_set_frame_counter(trhip_sh* s, uint32_t frame_counter) {
    if (!s) return set_error("trhip_sh_set_frame_counter: null stage");
    s->frame_counter = frame_counter;
    return 0;
}

int trhip_sh_reset_history(trhip_sh* s) {
    if (!s) return set_error("trhip_sh_reset_history: null stage");
    s->history_length = 0;
    return 0;
}

int trhip_sh_set_lanes(trhip_sh* s, int lanes) {
    if (!s) return set_error("trhip_sh_set_lanes: null stage");
    if (lanes < 0) return set_error("trhip_sh_set_lanes: lanes must be >= 0");
    s->pt->lanes = lanes;
    return 0;
}

int trhip_sh_set_batch_probes(trhip_sh* s, uint32_t probes) {
    if (!s) return set_error("trhip_sh_set_batch_probes: null stage");
    if ((uint64_t)probes * s->opt.samples_per_probe > SH_MAX_BATCH_PATHS)
        return set_error("trhip_sh_set_batch_probes: " + std::to_string(probes) + " probes of " + std::to_string(s->opt.samples_per_probe) +
                         " samples are more than the " + std::to_string(SH_MAX_BATCH_PATHS) + " paths of a batch");
    s->batch_probes = probes;
    return 0;
}

int trhip_sh_set_shading_arithmetic(trhip_sh* s, int ieee) {
    if (!s) return set_error("trhip_sh_set_shading_arithmetic: null stage");
    s->pt->ieee_shading = ieee ? 1 : 0;
    return 0;
}

int trhip_sh_get_grid_data(trhip_sh* s, trhip_sh_grid_data* out) {
    if (!s || !out) return set_error("trhip_sh_get_grid_data: null argument");
    unpack_grid_data(grid_data_of(s, s->history_length + 1), out);      // of the next render
    return 0;
}

int trhip_sh_pack_grid_data(const float transform[16], const float scaling[3], const uint32_t resolution[3], uint32_t samples_per_probe, uint32_t frame_counter,
                            uint32_t history_length, float temporal_ratio, trhip_sh_grid_data* out) {
    if (!transform || !scaling || !resolution || !out) return set_error("trhip_sh_pack_grid_data: null argument");
    if (history_length == 0) return set_error("trhip_sh_pack_grid_data: history_length counts the render itself: it is at least 1");
    m4 t;
    memcpy(&t, transform, sizeof(t));
    unpack_grid_data(pack_grid_data(t, F3(scaling[0], scaling[1], scaling[2]), resolution, samples_per_probe, frame_counter, history_length, temporal_ratio), out);
    return 0;
}

int trhip_sh_render(trhip_sh* s, void* stream) {
    if (!s) return set_error("trhip_sh_render: null stage");
    DEVCHK(s->hip_device);
    DeviceScene* scene = device_scene(s->dev);
    if (int r = check_scene_ready("trhip_sh_render", scene->instance_count, scene->accel_built)) return r;
    hipStream_t st = (hipStream_t)stream;
    s->last_stream = st;
    const uint32_t n = s->opt.samples_per_probe;
    const size_t probes = s->probes();
    const uint32_t fit = SH_MAX_BATCH_PATHS / n;
    const uint32_t per_batch = (uint32_t)std::min<size_t>(probes, s->batch_probes ? s->batch_probes : fit);
    ShProjectParams PP{};
    PP.batch.grid = grid_data_of(s, s->history_length + 1);
    PP.batch.samples = n;
    PP.batch.sample_counter = s->frame_counter * n;
    { uint seed = s->path.rng_seed; PP.batch.rng_seed = seed != 0 ? pcg(seed) : 0; }      // src/rt_stage.cc:82
    PP.coef_mult = (4.0f * SH_PI) / (float)n;
    PP.previous = s->grid; PP.grid = s->grid; PP.grid_half = s->grid_half;
    const bool timing = s->pt->detailed_timing != 0;
    size_t used_events = 0;
    auto project_event = [&]() -> hipError_t {
        if (used_events == s->project_events.size()) { hipEvent_t e; if (hipError_t r = hipEventCreate(&e)) return r; s->project_events.push_back(e); }
        return hipEventRecord(s->project_events[used_events++], st);
    };
    HIPCHK(hipEventRecord(s->ev[0], st));
    for (size_t base = 0; base < probes; base += per_batch) {
        PP.batch.probe_base = (uint32_t)base;
        PP.batch.n_probes = (uint32_t)std::min<size_t>(per_batch, probes - base);
        s->pt->probes = &PP.batch;
        const int rc = s->pt->render(trhip_pt_targets{}, 0, 0, 1, st);
        s->pt->probes = nullptr;
        if (rc) return rc;
        const PathBuffers pb = *s->pt->path_buffers();
        const dim3 grid(PP.batch.n_probes), block(SH_BLOCK);
        if (timing) HIPCHK(project_event());
        switch (s->opt.order) {
            case 0: hipLaunchKernelGGL(k_sh_project<0>, grid, block, 0, st, pb, PP); break;
            case 1: hipLaunchKernelGGL(k_sh_project<1>, grid, block, 0, st, pb, PP); break;
            case 2: hipLaunchKernelGGL(k_sh_project<2>, grid, block, 0, st, pb, PP); break;
            case 3: hipLaunchKernelGGL(k_sh_project<3>, grid, block, 0, st, pb, PP); break;
            default: hipLaunchKernelGGL(k_sh_project<4>, grid, block, 0, st, pb, PP); break;
        }
        if (timing) HIPCHK(project_event());
    }
    s->timed_events = used_events;
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipGetLastError());
    s->history_length += 1;
    s->frame_counter += 1;
    s->frames += 1;
    return 0;
}

int trhip_sh_get_grids(trhip_sh* s, void** grid_dev, void** grid_half_dev) {
    if (!s) return set_error("trhip_sh_get_grids: null stage");
    if (grid_dev) *grid_dev = s->grid;
    if (grid_half_dev) *grid_half_dev = s->grid_half;
    return 0;
}

int trhip_sh_download(trhip_sh* s, int which, void* host, size_t bytes) {
    return stage_download("trhip_sh_download", s, host, bytes, [&](const void*& src, size_t& size) {
        switch (which) {
            case TRHIP_SH_GRID: src = s->grid; size = s->entries() * sizeof(f4); break;
            case TRHIP_SH_GRID_HALF: src = s->grid_half; size = s->entries() * 4 * sizeof(__half); break;
            default: return set_error("trhip_sh_download: unknown buffer");
        }
        return 0;
    });
}

int trhip_sh_get_counters(trhip_sh* s, trhip_counters* out) {
    if (!s || !out) return set_error("trhip_sh_get_counters: null argument");
    DEVCHK(s->hip_device);
    return s->pt->get_counters(out, s->last_stream);
}

int trhip_sh_get_primary_start(trhip_sh* s, trhip_primary_start_info* out) {      // trhip_pt_get_primary_start of the bounce loop: never in effect
    if (!s || !out) return set_error("trhip_sh_get_primary_start: null argument");
    const int e = s->pt->primary_start_in_effect();
    if (e < 0) return set_error("trhip_sh_get_primary_start: TRHIP_PRIMARY_START is not auto or off");
    out->mode = s->pt->primary_start; out->in_effect = e; out->last_frame = s->pt->last_primary_start; out->pad = 0;
    return 0;
}

int trhip_sh_set_profiling(trhip_sh* s, int count_work, int detailed_timing) {
    if (!s) return set_error("trhip_sh_set_profiling: null stage");
    s->pt->count_work = count_work; s->pt->detailed_timing = detailed_timing;
    if (!detailed_timing) s->timed_events = 0;
    return 0;
}

int trhip_sh_get_timings(trhip_sh* s, trhip_sh_timings* out) {
    if (int r = stage_total_ms("trhip_sh_get_timings", s, out)) return r;
    snprintf(out->name, sizeof(out->name), "SH path tracing");
    if (s->frames == 0) return 0;
    trhip_timings t;
    if (int r = s->pt->get_timings(&t)) return r;      // cumulative since trhip_sh_reset_counters, only collected under detailed timing
    out->raygen_ms = t.raygen_ms; out->trace_closest_ms = t.trace_closest_ms; out->trace_shadow_ms = t.trace_shadow_ms; out->shade_ms = t.shade_ms;
    for (size_t i = 0; i + 1 < s->timed_events; i += 2) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, s->project_events[i], s->project_events[i + 1]));
        out->project_ms += ms;
    }
    return 0;
}

int trhip_sh_reset_counters(trhip_sh* s) {
    if (!s) return set_error("trhip_sh_reset_counters: null stage");
    DEVCHK(s->hip_device);
    HIPCHK(hipStreamSynchronize(s->last_stream));
    return s->pt->reset_counters();
}

}  // extern "C"
