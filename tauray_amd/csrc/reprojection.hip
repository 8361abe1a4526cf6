// Sparse light fields for gfx950: the first-hit G-buffer pass of viewports that are not path traced (k_gbuffer), spatial_reprojection_stage
// (src/spatial_reprojection_stage.{hh,cc}, shader/spatial_reprojection.comp restated: k_spatial_reprojection) and
// temporal_reprojection_stage (src/temporal_reprojection_stage.{hh,cc}, shader/temporal_reprojection.comp restated:
// k_temporal_reprojection), with the entry points trhip_gbuffer_render, trhip_spatial_reprojection_* and trhip_temporal_reprojection_*
// of include/trhip.h.  Layouts: reprojection.h.  Everything is fp32 and evaluated without contraction in a fixed order, no atomics: two
// runs of the same inputs give the same bits.  k_gbuffer's first hit is first_hit.h's, the one k_feature (api.hip) calls.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "reprojection.h"
#include "first_hit.h"
#include "stage_host.h"
#include "taps.h"
#include "pt.h"
#include "trace.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;

TR_DEV f2 octahedral_pack(f3 n) {        // math.glsl:480-485, as write_first_hit_gbuffer (path_tracer.hip) evaluates it
    const f3 nn = n / (fabsf(n.x) + fabsf(n.y) + fabsf(n.z));
    return nn.z >= 0.0f ? F2(nn.x, nn.y)
                        : F2((1 - fabsf(nn.y)) * ((nn.x >= 0.0f ? 1.0f : 0.0f) * 2 - 1), (1 - fabsf(nn.x)) * ((nn.y >= 0.0f ? 1.0f : 0.0f) * 2 - 1));
}

// ---------------------------------------------------------------------------------------------------
// The primary hit of k_feature (api.hip) for `count` viewports at once: pos = feature 3, instance id = feature 9, normal = the packing of
// feature 1; a miss writes the ray origin, the packed -direction and -1, as the path tracer's targets do (k_first_hit_gbuffer).
template <bool TWO_LEVEL>
__global__ __launch_bounds__(KB) void k_gbuffer(SceneView sv, LaunchCtx L, int projection, ViewportList list, float min_ray_dist,
                                                f2* normal, f4* pos, int* instance_id, uint* overflow_flag) {
    __shared__ int s_stack_rows[TR_STACK_WORDS];
    int* const s_stack = s_stack_rows + TR_STACK_ROW0;
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const uint layer = blockIdx.z;
    const CameraData cam = sv.cameras[list.v[layer]];
    f3 ray_origin, dir;
    HitRecord hit;
    int overflow;
    first_hit<TWO_LEVEL>(sv, L, cam, projection, px, py, min_ray_dist, s_stack + threadIdx.x, ray_origin, dir, hit, overflow);
    if (overflow) *overflow_flag = 1;
    f3 p = ray_origin, n = -dir;
    int id = -1;
    if (hit.instance_id >= 0) {
        SurfacePoint v;
        SampledMaterial mat;
        first_hit_surface(sv, hit, dir, ray_origin, v, mat);
        p = v.pos; n = v.mapped_normal; id = hit.instance_id;
    }
    const size_t pix = ((size_t)layer * L.launch_h + (uint)py) * L.launch_w + (uint)px;
    if (normal) normal[pix] = octahedral_pack(n);
    if (pos) pos[pix] = F4(p, 0.0f);
    if (instance_id) instance_id[pix] = id;
}

// ---------------------------------------------------------------------------------------------------
// The tap logic both stages share (tap_position, tap_weights: taps.h; the success threshold there is REPROJ_MIN_WEIGHT).

struct TapSource {      // one layer of G-buffer and colour that taps are taken from
    const f4* color; const f2* normal; const f4* pos; const int* instance_id;      // instance_id may be null
    bool pos_w_marks;   // a history layer: pos.w != 0 = no surface
};

TR_DEV bool no_surface(const f4 p, const int* ids, size_t pix, bool pos_w_marks) {
    if (pos_w_marks) return p.w != 0.0f;
    return any_nan(F3(p)) || (ids && ids[pix] < 0);
}

// Keep bits of the four taps at (tx, ty): inside the image, a surface, dot(n_tap, n) > 0.99, |pos - pos_tap|^2 < 0.01.
TR_DEV uint keep_taps(const TapSource& S, int w, int h, int tx, int ty, f3 n, f3 p) {
    uint bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = tx + (k & 1), y = ty + (k >> 1);
        if (x < 0 || y < 0 || x >= w || y >= h) continue;
        const size_t s = (size_t)y * w + x;
        const f4 pp = S.pos[s];
        if (no_surface(pp, S.instance_id, s, S.pos_w_marks)) continue;
        const f3 d = p - F3(pp);
        if (dot(octahedral_unpack(S.normal[s]), n) > REPROJ_NORMAL_COS && dot(d, d) < REPROJ_DISTANCE_SQ) bits |= 1u << k;
    }
    return bits;
}

TR_DEV f4 blend_taps(const f4* img, int w, int tx, int ty, uint bits, const float cw[4]) {
    f4 r = F4(0.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f4 t = F4(0.0f);
        if (bits & (1u << k)) t = img[(size_t)(ty + (k >> 1)) * w + (tx + (k & 1))];
        r = r + t * cw[k];
    }
    return r;
}

// One try: the taps of `S` around uv.  True when the kept weight exceeds 1e-5; then `out` is the blended colour.
TR_DEV bool try_taps(const TapSource& S, int w, int h, f2 uv, f3 n, f3 p, f4& out, uint& bits, int& tx, int& ty) {
    float qx, qy;
    tap_position(uv, w, h, tx, ty, qx, qy);
    bits = keep_taps(S, w, h, tx, ty, n, p);
    float cw[4];
    if (!(tap_weights(qx, qy, bits, cw) > REPROJ_MIN_WEIGHT)) return false;
    out = blend_taps(S.color, w, tx, ty, bits, cw);
    return true;
}

TR_DEV ReprojRecord make_record(int kind, int slot, uint bits, int tx, int ty) {
    ReprojRecord r;
    r.kind = (uint8_t)kind; r.slot = (uint8_t)slot; r.bits = (uint8_t)bits; r.zero = 0; r.ox = (int16_t)tx; r.oy = (int16_t)ty;
    return r;
}

// ---------------------------------------------------------------------------------------------------
struct SpatialParams {
    int w, h, total, sources;
    const CameraData* cameras;      // the scene's current cameras, [total] at least
    const int* source_viewport;     // [sources]
    const int* layer_of;            // [total]: >= 0: source slot; < 0: destination layer -(v + 1)
    const f4* src_color; const f2* src_normal; const f4* src_pos; const int* src_id;
    const f2* dst_normal; const f4* dst_pos; const int* dst_id;
    f4* out;
    f4 default_value;
    ReprojRecord* record;           // [total - sources][h][w]
};

// Depth of world position p under source s and its screen position; false: behind the camera plane (w <= 0) or not in front of the far plane.
TR_DEV bool project_to_source(const SpatialParams& P, int s, f3 p, float& depth, f2& uv) {
    const f4 c = mul(P.cameras[P.source_viewport[s]].view_proj, F4(p, 1.0f));      // s is wave-uniform: the matrix arrives through scalar loads
    if (!(c.w > 0.0f)) return false;
    depth = c.z / c.w;
    uv = F2((c.x / c.w) * 0.5f + 0.5f, (c.y / c.w) * 0.5f + 0.5f);
    return depth < 1.0f;
}

// One thread per output pixel; blockIdx.z = viewport in natural order.
__global__ __launch_bounds__(KB) void k_spatial_reprojection(SpatialParams P) {
    int x, y;
    tile_pixel(x, y);
    if (x >= P.w || y >= P.h) return;
    const int vp = (int)blockIdx.z;
    const size_t layer_px = (size_t)P.w * P.h, in_layer = (size_t)y * P.w + x;
    const int lo = P.layer_of[vp];
    f4* const out = P.out + (size_t)vp * layer_px + in_layer;
    if (lo >= 0) { *out = P.src_color[(size_t)lo * layer_px + in_layer]; return; }
    const size_t dpix = (size_t)(-(lo + 1)) * layer_px + in_layer;
    const f4 pp = P.dst_pos[dpix];
    f4 result = P.default_value;
    ReprojRecord rec = make_record(REPROJ_NONE, 0, 0, 0, 0);
    if (no_surface(pp, P.dst_id, dpix, false)) {
        for (int s = 0; s < P.sources; ++s) {
            const size_t spix = (size_t)s * layer_px + in_layer;
            if (no_surface(P.src_pos[spix], P.src_id, spix, false)) { result = P.src_color[spix]; rec = make_record(REPROJ_SKY_COPY, s, 0, 0, 0); break; }
        }
    } else {
        const f3 p = F3(pp), n = octahedral_unpack(P.dst_normal[dpix]);
        // the candidate: the source that sees the point nearest (smallest z / w below 1; ties go to the first)
        int cand = -1;
        float cand_depth = 1.0f;
        for (int s = 0; s < P.sources; ++s) {
            float depth; f2 uv;
            if (project_to_source(P, s, p, depth, uv) && depth < cand_depth) { cand = s; cand_depth = depth; }
        }
        // the candidate first; if it fails, the others in order, each only if it is nearer than the best accepted so far
        float best = 1.0f;
        for (int i = (cand >= 0 ? -1 : 0); i < P.sources; ++i) {
            const int s = i < 0 ? cand : i;
            if (i >= 0 && s == cand) continue;
            float depth; f2 uv;
            if (!project_to_source(P, s, p, depth, uv) || !(depth < best)) continue;
            const TapSource S = {P.src_color + (size_t)s * layer_px, P.src_normal + (size_t)s * layer_px, P.src_pos + (size_t)s * layer_px,
                                 P.src_id ? P.src_id + (size_t)s * layer_px : nullptr, false};
            f4 c; uint bits; int tx, ty;
            if (try_taps(S, P.w, P.h, uv, n, p, c, bits, tx, ty)) {
                result = c; best = depth; rec = make_record(REPROJ_REPROJECTED, s, bits, tx, ty);
                if (i < 0) break;
            }
        }
    }
    *out = result;
    P.record[dpix] = rec;
}

// ---------------------------------------------------------------------------------------------------
struct TemporalParams {
    int w, h, layers, have_history;
    float ratio;
    f4* color; const f2* normal; const f4* pos; const f2* motion; const int* instance_id;
    const f4* color_prev; const f2* normal_prev; const f4* pos_prev;      // pos.w = 1: no surface
    f4* color_cur; f2* normal_cur; f4* pos_cur;
    ReprojRecord* record;
};

__global__ __launch_bounds__(KB) void k_temporal_reprojection(TemporalParams P) {
    int x, y;
    tile_pixel(x, y);
    if (x >= P.w || y >= P.h) return;
    const size_t layer_px = (size_t)P.w * P.h, base = (size_t)blockIdx.z * layer_px, pix = base + (size_t)y * P.w + x;
    const f4 pp = P.pos[pix];
    const f2 packed = P.normal[pix];
    const bool nosurf = no_surface(pp, P.instance_id, pix, false);
    f4 col = P.color[pix];
    ReprojRecord rec = make_record(REPROJ_NONE, 0, 0, 0, 0);
    if (P.have_history && !nosurf) {
        const TapSource S = {P.color_prev + base, P.normal_prev + base, P.pos_prev + base, nullptr, true};
        f4 c; uint bits; int tx, ty;
        if (try_taps(S, P.w, P.h, P.motion[pix], octahedral_unpack(packed), F3(pp), c, bits, tx, ty)) {
            const f4 blended = mix4(col, c, P.ratio);
            if (!(isnan(blended.x) || isnan(blended.y) || isnan(blended.z) || isnan(blended.w))) {
                col = blended;
                P.color[pix] = col;
                rec = make_record(REPROJ_REPROJECTED, 0, bits, tx, ty);
            }
        }
    }
    P.color_cur[pix] = col;
    P.normal_cur[pix] = packed;
    P.pos_cur[pix] = F4(pp.x, pp.y, pp.z, nosurf ? 1.0f : 0.0f);
    P.record[pix] = rec;
}

int check_size(const char* who, uint32_t w, uint32_t h, uint32_t layers) {
    if (w == 0 || h == 0 || layers == 0) return set_error(std::string(who) + ": zero width, height or layer count");
    if (w > 16384 || h > 16384 || layers > 4096) return set_error(std::string(who) + ": image too large");      // the record's tap origin is int16
    return 0;
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_spatial_reprojection : StageHost<> {
    trhip_device* dev = nullptr;
    uint32_t w = 0, h = 0, total = 0, sources = 0;
    f4 default_value = {0, 0, 0, 0};
    int* source_viewport = nullptr;      // device
    int* layer_of = nullptr;             // device
    ReprojRecord* record = nullptr;
    size_t record_count() const { return (size_t)(total - sources) * w * h; }
};

struct trhip_temporal_reprojection : StageHost<> {
    uint32_t w = 0, h = 0, layers = 0;
    float ratio = 0;
    int cur = 0;                         // the history a frame reads; it writes cur ^ 1
    bool have_history = false;
    f4* color[2] = {};
    f2* normal[2] = {};
    f4* pos[2] = {};
    ReprojRecord* record = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
};

extern "C" {

int trhip_gbuffer_render(trhip_device* dev, int projection, const uint32_t* viewports, uint32_t count, float min_ray_dist,
                         const trhip_gbuffer_targets* targets, uint32_t width, uint32_t height, void* stream) {
    if (!dev) return set_error("trhip_gbuffer_render: null trhip_device (no HIP device: there is no CPU fallback)");
    if (!targets) return set_error("trhip_gbuffer_render: null targets");
    if (count == 0) return 0;
    if (!viewports) return set_error("trhip_gbuffer_render: null viewport list");
    if (check_size("trhip_gbuffer_render", width, height, count)) return 1;
    DEVCHK(device_index(dev));
    DeviceScene* scene = device_scene(dev);
    if (!scene->accel_built) return set_error("trhip_gbuffer_render: call trhip_scene_build_accel first");
    if (int r = check_viewport_list("trhip_gbuffer_render", viewports, count, 0, scene->camera_count)) return r;
    const LaunchCtx L = whole_image_launch(width, height);
    const size_t layer_px = (size_t)width * height;
    for_each_viewport_chunk<ViewportList>(viewports, count, [&](uint32_t first, uint32_t n, const ViewportList& list) {
        f2* normal = targets->normal ? (f2*)targets->normal + first * layer_px : nullptr;
        f4* pos = targets->pos ? (f4*)targets->pos + first * layer_px : nullptr;
        int* ids = targets->instance_id ? (int*)targets->instance_id + first * layer_px : nullptr;
        hipLaunchKernelGGL(scene->two_level ? k_gbuffer<true> : k_gbuffer<false>, tile_grid(width, height, n), dim3(KB), 0, (hipStream_t)stream, scene->view(), L,
                           projection, list, min_ray_dist, normal, pos, ids, device_overflow_flag(dev));
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int trhip_spatial_reprojection_create(trhip_device* dev, uint32_t width, uint32_t height, uint32_t total_viewports, const uint32_t* source_viewports,
                                      uint32_t source_count, const float default_value[4], trhip_spatial_reprojection** out) {
    if (!out) return set_error("trhip_spatial_reprojection_create: null out");
    *out = nullptr;
    if (check_size("trhip_spatial_reprojection_create", width, height, total_viewports)) return 1;
    if (!source_viewports || source_count == 0) return set_error("trhip_spatial_reprojection_create: no source viewports");
    if (source_count >= total_viewports) return set_error("trhip_spatial_reprojection_create: every viewport is a source: nothing to reproject");
    if (source_count > (uint32_t)REPROJ_MAX_SOURCES) return set_error("trhip_spatial_reprojection_create: more than 255 source viewports");
    if (!default_value) return set_error("trhip_spatial_reprojection_create: null default_value");
    std::vector<int> layer_of(total_viewports, -1), src(source_count);
    for (uint32_t i = 0; i < source_count; ++i) {
        const uint32_t v = source_viewports[i];
        if (v >= total_viewports) return set_error("trhip_spatial_reprojection_create: source viewport " + std::to_string(v) + " out of range (" + std::to_string(total_viewports) + " viewports)");
        if (layer_of[v] >= 0) return set_error("trhip_spatial_reprojection_create: source viewport " + std::to_string(v) + " listed twice");
        layer_of[v] = (int)i; src[i] = (int)v;
    }
    int d = 0;
    for (uint32_t v = 0; v < total_viewports; ++v) if (layer_of[v] < 0) layer_of[v] = -(d++ + 1);
    if (!dev) return set_error("trhip_spatial_reprojection_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_spatial_reprojection* s = new trhip_spatial_reprojection;
    s->dev = dev; s->hip_device = device_index(dev);
    s->w = width; s->h = height; s->total = total_viewports; s->sources = source_count;
    s->default_value = F4(default_value[0], default_value[1], default_value[2], default_value[3]);
    s->alloc_zeroed(s->source_viewport, src.size() * sizeof(int));
    if (s->err == hipSuccess) s->err = hipMemcpy(s->source_viewport, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice);
    s->alloc_zeroed(s->layer_of, layer_of.size() * sizeof(int));
    if (s->err == hipSuccess) s->err = hipMemcpy(s->layer_of, layer_of.data(), layer_of.size() * sizeof(int), hipMemcpyHostToDevice);
    s->alloc_zeroed(s->record, s->record_count() * sizeof(ReprojRecord));
    return stage_finish_create("trhip_spatial_reprojection_create", s, out);
}

void trhip_spatial_reprojection_destroy(trhip_spatial_reprojection* s) { stage_destroy(s); }

int trhip_spatial_reprojection_run(trhip_spatial_reprojection* s, const trhip_reprojection_images* sources, const trhip_reprojection_images* destinations,
                                   void* color_out, void* stream) {
    if (!s) return set_error("trhip_spatial_reprojection_run: null stage");
    if (!sources || !destinations || !color_out) return set_error("trhip_spatial_reprojection_run: null images");
    if (!sources->color || !sources->normal || !sources->pos || !sources->instance_id)
        return set_error("trhip_spatial_reprojection_run: the sources need color, normal, pos and instance_id");
    if (!destinations->normal || !destinations->pos || !destinations->instance_id)
        return set_error("trhip_spatial_reprojection_run: the destinations need normal, pos and instance_id");
    DEVCHK(s->hip_device);
    DeviceScene* scene = device_scene(s->dev);
    if (scene->camera_count < s->total || !scene->cameras)
        return set_error("trhip_spatial_reprojection_run: the scene has " + std::to_string(scene->camera_count) + " cameras, the stage " + std::to_string(s->total) + " viewports");
    SpatialParams P{};
    P.w = (int)s->w; P.h = (int)s->h; P.total = (int)s->total; P.sources = (int)s->sources;
    P.cameras = scene->cameras; P.source_viewport = s->source_viewport; P.layer_of = s->layer_of;
    P.src_color = (const f4*)sources->color; P.src_normal = (const f2*)sources->normal; P.src_pos = (const f4*)sources->pos; P.src_id = (const int*)sources->instance_id;
    P.dst_normal = (const f2*)destinations->normal; P.dst_pos = (const f4*)destinations->pos; P.dst_id = (const int*)destinations->instance_id;
    P.out = (f4*)color_out; P.default_value = s->default_value; P.record = s->record;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(k_spatial_reprojection, tile_grid(s->w, s->h, s->total), dim3(KB), 0, st, P);
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipGetLastError());
    s->frames += 1;
    return 0;
}

int trhip_spatial_reprojection_get_timings(trhip_spatial_reprojection* s, trhip_reprojection_timings* out) {
    return stage_total_ms("trhip_spatial_reprojection_get_timings", s, out);
}

int trhip_spatial_reprojection_download(trhip_spatial_reprojection* s, int which, void* host, size_t bytes) {
    return stage_download("trhip_spatial_reprojection_download", s, host, bytes, [&](const void*& src, size_t& size) {
        if (which != TRHIP_REPROJECTION_DECISIONS) return set_error("trhip_spatial_reprojection_download: unknown buffer");
        src = s->record; size = s->record_count() * sizeof(ReprojRecord);
        return 0;
    });
}

int trhip_temporal_reprojection_create(trhip_device* dev, uint32_t width, uint32_t height, uint32_t layers, float ratio, trhip_temporal_reprojection** out) {
    if (!out) return set_error("trhip_temporal_reprojection_create: null out");
    *out = nullptr;
    if (check_size("trhip_temporal_reprojection_create", width, height, layers)) return 1;
    if (!(ratio > 0.0f) || !(ratio < 1.0f)) return set_error("trhip_temporal_reprojection_create: ratio must be in (0, 1)");
    if (!dev) return set_error("trhip_temporal_reprojection_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_temporal_reprojection* t = new trhip_temporal_reprojection;
    t->hip_device = device_index(dev);
    t->w = width; t->h = height; t->layers = layers; t->ratio = ratio;
    const size_t px = t->pixels();
    for (int i = 0; i < 2; ++i) { t->alloc_zeroed(t->color[i], px * sizeof(f4)); t->alloc_zeroed(t->normal[i], px * sizeof(f2)); t->alloc_zeroed(t->pos[i], px * sizeof(f4)); }
    t->alloc_zeroed(t->record, px * sizeof(ReprojRecord));
    return stage_finish_create("trhip_temporal_reprojection_create", t, out);
}

void trhip_temporal_reprojection_destroy(trhip_temporal_reprojection* t) { stage_destroy(t); }

int trhip_temporal_reprojection_reset_history(trhip_temporal_reprojection* t) {
    if (!t) return set_error("trhip_temporal_reprojection_reset_history: null stage");
    t->have_history = false;
    return 0;
}

int trhip_temporal_reprojection_run(trhip_temporal_reprojection* t, const trhip_reprojection_images* images, void* stream) {
    if (!t) return set_error("trhip_temporal_reprojection_run: null stage");
    if (!images) return set_error("trhip_temporal_reprojection_run: null images");
    if (!images->color || !images->normal || !images->pos || !images->screen_motion)
        return set_error("trhip_temporal_reprojection_run: color, normal, pos and screen_motion are required (only instance_id may be null)");
    DEVCHK(t->hip_device);
    TemporalParams P{};
    P.w = (int)t->w; P.h = (int)t->h; P.layers = (int)t->layers; P.have_history = t->have_history ? 1 : 0; P.ratio = t->ratio;
    P.color = (f4*)images->color; P.normal = (const f2*)images->normal; P.pos = (const f4*)images->pos; P.motion = (const f2*)images->screen_motion;
    P.instance_id = (const int*)images->instance_id;
    const int c = t->cur, nx = c ^ 1;
    P.color_prev = t->color[c]; P.normal_prev = t->normal[c]; P.pos_prev = t->pos[c];
    P.color_cur = t->color[nx]; P.normal_cur = t->normal[nx]; P.pos_cur = t->pos[nx];
    P.record = t->record;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(t->ev[0], st));
    hipLaunchKernelGGL(k_temporal_reprojection, tile_grid(t->w, t->h, t->layers), dim3(KB), 0, st, P);
    HIPCHK(hipEventRecord(t->ev[1], st));
    HIPCHK(hipGetLastError());
    t->cur = nx;
    t->have_history = true;
    t->frames += 1;
    return 0;
}

int trhip_temporal_reprojection_get_timings(trhip_temporal_reprojection* t, trhip_reprojection_timings* out) {
    return stage_total_ms("trhip_temporal_reprojection_get_timings", t, out);
}

int trhip_temporal_reprojection_download(trhip_temporal_reprojection* t, int which, void* host, size_t bytes) {
    return stage_download("trhip_temporal_reprojection_download", t, host, bytes, [&](const void*& src, size_t& size) {
        const size_t px = t->pixels();
        const int c = t->cur;      // what the last frame wrote
        switch (which) {
            case TRHIP_REPROJECTION_DECISIONS: src = t->record; size = px * sizeof(ReprojRecord); break;
            case TRHIP_REPROJECTION_PREVIOUS_COLOR: src = t->color[c]; size = px * sizeof(f4); break;
            case TRHIP_REPROJECTION_PREVIOUS_NORMAL: src = t->normal[c]; size = px * sizeof(f2); break;
            case TRHIP_REPROJECTION_PREVIOUS_POS: src = t->pos[c]; size = px * sizeof(f4); break;
            default: return set_error("trhip_temporal_reprojection_download: unknown buffer");
        }
        return 0;
    });
}

}  // extern "C"
