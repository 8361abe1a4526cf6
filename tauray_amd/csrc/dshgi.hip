// dshgi_renderer's indirect light for gfx950 - the consumer half of the reference's DDISH-GI (src/dshgi_renderer.{hh,cc}, shader/forward.frag,
// shader/spherical_harmonics.glsl restated) behind the entry points trhip_dshgi_* and trhip_brdf_integration_generate of include/trhip.h.
//   k_dshgi_indirect      per pixel of every viewport: the first hit and its surface (first_hit.h), the instance's SH
//                         grid sampled at the hit (trilinear or probe visibility), the cosine and GGX lobes, brdf_indirect, modulate_color;
//                         the result is added to the direct stage's colour
//   k_brdf_integration    the split-sum scale and bias table the reference loads from data/brdf_integration.exr
// The reference rasterises the first hit and lights it with shadow maps; here the first hit is a ray and direct light is the direct stage's
// (DESIGN.md section 20).  Constants, layouts and the order of operations: dshgi.h.  Both kernels are IEEE fp32, evaluated without
// contraction in a fixed order, no atomics: two runs of the same inputs give the same bits.  The front half is first_hit.h's, the one
// k_gbuffer and k_feature call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dshgi.h"
#include "first_hit.h"
#include "stage_host.h"
#include "pt.h"
#include "trace.h"

namespace tr {
namespace {

constexpr int KB = TR_BLOCK;

struct DshgiParams {
    const DshgiGrid* grids;
    const int* instance_grid;          // per instance: its grid, -1 = none
    const f2* table;
    int table_w, table_h;
    const f4* direct;                  // may be null, may be `out`
    f4* out;
    f4* indirect;                      // the indirect term alone (TRHIP_DSHGI_INDIRECT)
    DshgiSurface* surface;             // null unless record_surface
};

// tile_pixel's launch shape: coherent primary rays, and the pixels of a wave fall into a few grid cells, so its texel reads collapse onto
// a few lines.
template <bool TWO_LEVEL, int ORDER, bool VISIBILITY>
__global__ __launch_bounds__(KB) void k_dshgi_indirect(SceneView sv, LaunchCtx L, int projection, ViewportList list, float min_ray_dist, DshgiParams P,
                                                       uint* overflow_flag) {
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
    DshgiSurface s = {};
    s.grid = -1; s.instance_id = -1;
    f3 indirect = F3(0.0f);
    if (hit.instance_id >= 0) {
        SurfacePoint v;
        SampledMaterial mat;
        first_hit_surface(sv, hit, dir, ray_origin, v, mat);
        s.pos = v.pos; s.smooth_normal = v.smooth_normal; s.mapped_normal = v.mapped_normal;
        s.view = dsh_normalize(v.pos - ray_origin);
        s.albedo = mat.albedo; s.metallic = mat.metallic; s.roughness = mat.roughness; s.f0 = mat.f0; s.transmittance = mat.transmittance;
        s.instance_id = hit.instance_id;
        s.grid = P.instance_grid[hit.instance_id];
        if (s.grid >= 0) indirect = dsh_indirect<ORDER, VISIBILITY>(P.grids[s.grid], s, P.table, P.table_w, P.table_h);
    }
    const size_t pix = ((size_t)layer * L.launch_h + (uint)py) * L.launch_w + (uint)px;
    const f4 d = P.direct ? P.direct[pix] : F4(0.0f);
    P.out[pix] = P.direct ? F4(d.x + indirect.x, d.y + indirect.y, d.z + indirect.z, d.w) : F4(indirect, 0.0f);
    P.indirect[pix] = F4(indirect, 0.0f);
    if (P.surface) P.surface[pix] = s;
}

// One thread per cell; the samples in order (dshgi.h).
__global__ __launch_bounds__(KB) void k_brdf_integration(int size, int samples, f2* out) {
    const uint cell = blockIdx.x * KB + threadIdx.x;
    if (cell >= (uint)size * (uint)size) return;
    const int i = (int)(cell % (uint)size), j = (int)(cell / (uint)size);
    const float cos_v = ((float)i + 0.5f) / (float)size, pr = ((float)j + 0.5f) / (float)size, a = pr * pr;
    const f3 V = F3(sqrtf(1.0f - cos_v * cos_v), 0.0f, cos_v);
    float scale = 0.0f, bias = 0.0f;
    for (int s = 0; s < samples; ++s) {
        const float u1 = ((float)s + 0.5f) / (float)samples, u2 = (float)__brev((uint)s) * 2.3283064365386963e-10f;
        const float phi = (2.0f * SH_PI) * u1;
        const float ct = sqrtf((1.0f - u2) / (1.0f + (a * a - 1.0f) * u2)), st = sqrtf(1.0f - ct * ct);
        const f3 H = F3(st * sh_cos(phi), st * sh_sin(phi), ct);
        const float vh = dsh_dot(V, H);
        const f3 Ld = H * (2.0f * vh) - V;
        if (!(Ld.z > 0.0f) || !(vh > 0.0f)) continue;
        const float g = ggx_masking_shadowing(V.z, vh, Ld.z, dsh_dot(Ld, H), a);
        const float gv = (g * vh) / (H.z * V.z), fc = sh_pow(1.0f - vh, 5.0f);
        scale = scale + (1.0f - fc) * gv;
        bias = bias + fc * gv;
    }
    out[cell] = F2(scale / (float)samples, bias / (float)samples);
}

// glm::affineInverse and mat4(inverse(get_matrix_orientation(transform))) in float, as the reference's host computes them (dshgi.h "host")
m4 affine_inverse(const m4& t) {
    const float m[3][3] = {{t.c[0].x, t.c[0].y, t.c[0].z}, {t.c[1].x, t.c[1].y, t.c[1].z}, {t.c[2].x, t.c[2].y, t.c[2].z}};      // m[column][row]
    const float inv_det = 1.0f / ((m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2])) +
                                  m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]));
    float r[3][3];
    r[0][0] = (m[1][1] * m[2][2] - m[2][1] * m[1][2]) * inv_det;
    r[1][0] = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * inv_det;
    r[2][0] = (m[1][0] * m[2][1] - m[2][0] * m[1][1]) * inv_det;
    r[0][1] = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * inv_det;
    r[1][1] = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) * inv_det;
    r[2][1] = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * inv_det;
    r[0][2] = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) * inv_det;
    r[1][2] = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * inv_det;
    r[2][2] = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) * inv_det;
    const f4 p = t.c[3];
    m4 o;
    for (int c = 0; c < 3; ++c) o.c[c] = F4(r[c][0], r[c][1], r[c][2], 0.0f);
    o.c[3] = F4(-((r[0][0] * p.x + r[1][0] * p.y) + r[2][0] * p.z), -((r[0][1] * p.x + r[1][1] * p.y) + r[2][1] * p.z),
                -((r[0][2] * p.x + r[1][2] * p.y) + r[2][2] * p.z), 1.0f);
    return o;
}
m3 inverse_orientation(const m4& t) {
    const f4 q = orientation_quat(t);
    const float d = (q.w * q.w + q.x * q.x) + (q.y * q.y + q.z * q.z);
    return mat3_of_quat(F4(-q.x / d, -q.y / d, -q.z / d, q.w / d));
}
f3 host_point(const m4& m, f3 p) { return F3(((m.c[0] * p.x + m.c[1] * p.y) + m.c[2] * p.z) + m.c[3] * 1.0f); }

bool finite16(const float* v, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// sh_grid::point_distance (src/sh_grid.cc:116-133) with the grid's pos_from_world
float point_distance(const m4& pos_from_world, float radius, f3 p) {
    const f3 l = host_point(pos_from_world, p);
    const f3 al = F3(fabsf(l.x), fabsf(l.y), fabsf(l.z));
    if (al.x <= 1.0f && al.y <= 1.0f && al.z <= 1.0f) return 0.0f;
    const float guard = 1.0f + radius;
    if (al.x <= guard && al.y <= guard && al.z <= guard) {
        const f3 q = al - 1.0f, qp = max3(q, F3(0.0f));
        return sqrtf((qp.x * qp.x + qp.y * qp.y) + qp.z * qp.z) + fmin2(fmax2(q.x, fmax2(q.y, q.z)), 0.0f);
    }
    return -1.0f;
}

using DshgiKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, float, DshgiParams, uint*);

template <bool TWO_LEVEL, bool VISIBILITY>
DshgiKernel dshgi_kernel(int order) {
    switch (order) {
        case 0: return k_dshgi_indirect<TWO_LEVEL, 0, VISIBILITY>;
        case 1: return k_dshgi_indirect<TWO_LEVEL, 1, VISIBILITY>;
        case 2: return k_dshgi_indirect<TWO_LEVEL, 2, VISIBILITY>;
        case 3: return k_dshgi_indirect<TWO_LEVEL, 3, VISIBILITY>;
        default: return k_dshgi_indirect<TWO_LEVEL, 4, VISIBILITY>;
    }
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_dshgi : StageHost<2> {
    trhip_device* dev = nullptr;
    trhip_dshgi_options opt = {};
    uint32_t w = 0, h = 0, layers = 0;
    DshgiGrid* grids = nullptr;             // device
    size_t grid_capacity = 0, grid_count = 0;
    std::vector<DshgiGrid> host_grids;
    int* instance_grid = nullptr;           // device
    size_t instance_capacity = 0;
    std::vector<int32_t> host_instance_grid;
    f2* table = nullptr;                    // device, the stage's copy
    size_t table_capacity = 0;
    uint32_t table_w = 0, table_h = 0;
    f4* indirect = nullptr;
    DshgiSurface* surface = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
    // A device array of at least n entries behind p; the old one is freed once nothing runs.
    template <class T>
    hipError_t reserve(T*& p, size_t& capacity, size_t n) {
        if (n <= capacity) return hipSuccess;
        if (hipError_t e = hipDeviceSynchronize()) return e;
        void* q = nullptr;
        if (hipError_t e = hipMalloc(&q, n * sizeof(T))) return e;
        bool replaced = false;
        for (void*& a : allocations)
            if (p && a == (void*)p) { (void)hipFree(a); a = q; replaced = true; break; }
        if (!replaced) allocations.push_back(q);
        p = (T*)q;
        capacity = n;
        return hipSuccess;
    }
};

static_assert(sizeof(trhip_dshgi_surface) == sizeof(DshgiSurface), "TRHIP_DSHGI_SURFACE downloads the kernel's record");

extern "C" {

int trhip_dshgi_pick_grid(const float* transforms, const float* scalings, const uint32_t* resolutions, const float* radii, uint32_t count,
                          const float position[3], int32_t* index) {
    if (!index) return set_error("trhip_dshgi_pick_grid: null index");
    *index = -1;
    if (count == 0) return 0;
    if (!transforms || !scalings || !resolutions || !radii || !position) return set_error("trhip_dshgi_pick_grid: null argument");
    const f3 p = F3(position[0], position[1], position[2]);
    // get_sh_grid (src/scene.cc:163-193)
    float closest_distance = __builtin_huge_valf(), densest = 0.0f;
    int best = -1;
    for (uint32_t g = 0; g < count; ++g) {
        m4 t;
        memcpy(&t, transforms + 16 * g, sizeof(t));
        const float distance = point_distance(affine_inverse(t), radii[g], p);
        if (distance >= 0.0f && distance <= closest_distance) {
            closest_distance = distance;
            if (distance == 0.0f) {
                const float* sc = scalings + 3 * g;
                const uint32_t* r = resolutions + 3 * g;
                const float volume = ((sc[0] * 2.0f) * (sc[1] * 2.0f)) * (sc[2] * 2.0f);
                const float density = (float)(r[0] * r[1] * r[2]) / volume;
                if (density > densest) { densest = density; best = (int)g; }
            } else best = (int)g;
        }
    }
    if (best < 0) {      // get_largest_sh_grid (src/scene.cc:195-211)
        float largest = 0.0f;
        for (uint32_t g = 0; g < count; ++g) {
            const float* sc = scalings + 3 * g;
            const float volume = ((sc[0] * 2.0f) * (sc[1] * 2.0f)) * (sc[2] * 2.0f);
            if (volume > largest) { largest = volume; best = (int)g; }
        }
    }
    *index = best;
    return 0;
}

int trhip_brdf_integration_generate(trhip_device* dev, uint32_t size, uint32_t samples, void* out_dev_rg32f, void* stream) {
    if (!dev) return set_error("trhip_brdf_integration_generate: null trhip_device (no HIP device: there is no CPU fallback)");
    if (size == 0 || size > 4096) return set_error("trhip_brdf_integration_generate: size must be in 1..4096");
    if (samples == 0 || samples > (1u << 20)) return set_error("trhip_brdf_integration_generate: samples must be in 1..1048576");
    if (!out_dev_rg32f) return set_error("trhip_brdf_integration_generate: null table");
    DEVCHK(device_index(dev));
    const uint cells = size * size;
    hipLaunchKernelGGL(k_brdf_integration, dim3((cells + KB - 1) / KB), dim3(KB), 0, (hipStream_t)stream, (int)size, (int)samples, (f2*)out_dev_rg32f);
    HIPCHK(hipGetLastError());
    return 0;
}

int trhip_dshgi_create(trhip_device* dev, const trhip_dshgi_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_dshgi** out) {
    if (!out) return set_error("trhip_dshgi_create: null out");
    *out = nullptr;
    if (!opt) return set_error("trhip_dshgi_create: null options");
    if (opt->order < 0 || opt->order > SH_MAX_ORDER) return set_error("trhip_dshgi_create: order " + std::to_string(opt->order) + " is outside 0..4");
    if (width == 0 || height == 0 || layers == 0) return set_error("trhip_dshgi_create: zero width, height or layer count");
    if (width > 16384 || height > 16384 || layers > 4096) return set_error("trhip_dshgi_create: image too large");
    if (!dev) return set_error("trhip_dshgi_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_dshgi* s = new trhip_dshgi;
    s->dev = dev; s->hip_device = device_index(dev);
    s->opt = *opt;
    s->w = width; s->h = height; s->layers = layers;
    s->alloc_zeroed(s->indirect, s->pixels() * sizeof(f4));
    if (opt->record_surface) s->alloc_zeroed(s->surface, s->pixels() * sizeof(DshgiSurface));
    return stage_finish_create("trhip_dshgi_create", s, out);
}

void trhip_dshgi_destroy(trhip_dshgi* s) { stage_destroy(s); }

int trhip_dshgi_set_grids(trhip_dshgi* s, const trhip_dshgi_grid* grids, uint32_t count) {
    if (!s) return set_error("trhip_dshgi_set_grids: null stage");
    if (count == 0 || !grids) return set_error("trhip_dshgi_set_grids: no grids");
    std::vector<DshgiGrid> packed(count);
    for (uint32_t g = 0; g < count; ++g) {
        const trhip_dshgi_grid& in = grids[g];
        const std::string who = "trhip_dshgi_set_grids: grid " + std::to_string(g);
        if (!in.grid_half_dev) return set_error(who + " has no device image");
        for (int a = 0; a < 3; ++a)
            if (in.resolution[a] == 0 || in.resolution[a] > 1024) return set_error(who + ": resolution outside 1..1024 on an axis");
        if (!finite16(in.transform, 16) || !finite16(in.scaling, 3)) return set_error(who + ": the transform is not finite");
        for (int c = 0; c < 3; ++c)
            if (in.transform[4 * c] == 0.0f && in.transform[4 * c + 1] == 0.0f && in.transform[4 * c + 2] == 0.0f) return set_error(who + ": the transform has a zero axis");
        m4 t;
        memcpy(&t, in.transform, sizeof(t));
        DshgiGrid& G = packed[g];
        G.texels = in.grid_half_dev;
        G.pos_from_world = affine_inverse(t);
        G.normal_from_world = inverse_orientation(t);
        if (!finite16(&G.pos_from_world.c[0].x, 16)) return set_error(who + ": the transform is singular");
        const f3 R = F3((float)in.resolution[0], (float)in.resolution[1], (float)in.resolution[2]);
        for (int a = 0; a < 3; ++a) G.res[a] = (int)in.resolution[a];
        G.grid_clamp = F3(0.5f / R.x, 0.5f / R.y, 0.5f / R.z);
        G.inv_grid_size = F3(1.0f / R.x, 1.0f / R.y, 1.0f / R.z);
    }
    for (int32_t g : s->host_instance_grid)
        if (g >= (int32_t)count) return set_error("trhip_dshgi_set_grids: an instance's grid index " + std::to_string(g) + " is out of range: " + std::to_string(count) + " grids");
    DEVCHK(s->hip_device);
    HIPCHK(s->reserve(s->grids, s->grid_capacity, count));
    HIPCHK(hipMemcpy(s->grids, packed.data(), count * sizeof(DshgiGrid), hipMemcpyHostToDevice));
    s->host_grids = std::move(packed);
    s->grid_count = count;
    return 0;
}

int trhip_dshgi_set_instance_grids(trhip_dshgi* s, const int32_t* instance_grids, uint32_t count) {
    if (!s) return set_error("trhip_dshgi_set_instance_grids: null stage");
    if (count == 0 || !instance_grids) return set_error("trhip_dshgi_set_instance_grids: no instances");
    if (s->grid_count == 0) return set_error("trhip_dshgi_set_instance_grids: no grids set (trhip_dshgi_set_grids)");
    for (uint32_t i = 0; i < count; ++i)
        if (instance_grids[i] < -1 || instance_grids[i] >= (int32_t)s->grid_count)
            return set_error("trhip_dshgi_set_instance_grids: instance " + std::to_string(i) + ": grid index " + std::to_string(instance_grids[i]) + " is out of range: " +
                             std::to_string(s->grid_count) + " grids");
    DEVCHK(s->hip_device);
    HIPCHK(s->reserve(s->instance_grid, s->instance_capacity, count));
    HIPCHK(hipMemcpy(s->instance_grid, instance_grids, count * sizeof(int32_t), hipMemcpyHostToDevice));
    s->host_instance_grid.assign(instance_grids, instance_grids + count);
    return 0;
}

int trhip_dshgi_set_brdf_integration(trhip_dshgi* s, const void* table_dev, uint32_t w, uint32_t h) {
    if (!s) return set_error("trhip_dshgi_set_brdf_integration: null stage");
    if (!table_dev) return set_error("trhip_dshgi_set_brdf_integration: null table");
    if (w == 0 || h == 0 || w > 4096 || h > 4096) return set_error("trhip_dshgi_set_brdf_integration: the table's size must be in 1..4096");
    DEVCHK(s->hip_device);
    HIPCHK(s->reserve(s->table, s->table_capacity, (size_t)w * h));
    HIPCHK(hipMemcpy(s->table, table_dev, (size_t)w * h * sizeof(f2), hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    s->table_w = w; s->table_h = h;
    return 0;
}

int trhip_dshgi_render(trhip_dshgi* s, int projection, const uint32_t* viewports, uint32_t count, float min_ray_dist, const void* direct_color_dev,
                       void* out_color_dev, void* stream) {
    if (!s) return set_error("trhip_dshgi_render: null stage");
    if (!viewports || !out_color_dev) return set_error("trhip_dshgi_render: null argument");
    DEVCHK(s->hip_device);
    DeviceScene* scene = device_scene(s->dev);
    if (int r = check_scene_ready("trhip_dshgi_render", scene->instance_count, scene->accel_built)) return r;
    if (s->grid_count == 0) return set_error("trhip_dshgi_render: no grids set (trhip_dshgi_set_grids)");
    if (s->host_instance_grid.size() != scene->instance_count)
        return set_error("trhip_dshgi_render: " + std::to_string(s->host_instance_grid.size()) + " instance grids set (trhip_dshgi_set_instance_grids), the scene has " +
                         std::to_string(scene->instance_count) + " instances");
    for (int32_t g : s->host_instance_grid)
        if (g >= (int32_t)s->grid_count) return set_error("trhip_dshgi_render: grid index " + std::to_string(g) + " is out of range: " + std::to_string(s->grid_count) + " grids");
    if (!s->table) return set_error("trhip_dshgi_render: no BRDF-integration table (trhip_dshgi_set_brdf_integration)");
    if (int r = check_viewport_list("trhip_dshgi_render", viewports, count, s->layers, scene->camera_count)) return r;
    const LaunchCtx L = whole_image_launch(s->w, s->h);
    const size_t layer_px = (size_t)s->w * s->h;
    const bool visibility = s->opt.use_probe_visibility != 0;
    const DshgiKernel kernel = scene->two_level ? (visibility ? dshgi_kernel<true, true>(s->opt.order) : dshgi_kernel<true, false>(s->opt.order))
                                                : (visibility ? dshgi_kernel<false, true>(s->opt.order) : dshgi_kernel<false, false>(s->opt.order));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(s->ev[0], st));
    for_each_viewport_chunk<ViewportList>(viewports, count, [&](uint32_t first, uint32_t n, const ViewportList& list) {
        DshgiParams P{};
        P.grids = s->grids; P.instance_grid = s->instance_grid; P.table = s->table; P.table_w = (int)s->table_w; P.table_h = (int)s->table_h;
        P.direct = direct_color_dev ? (const f4*)direct_color_dev + first * layer_px : nullptr;
        P.out = (f4*)out_color_dev + first * layer_px;
        P.indirect = s->indirect + first * layer_px;
        P.surface = s->surface ? s->surface + first * layer_px : nullptr;
        hipLaunchKernelGGL(kernel, tile_grid(s->w, s->h, n), dim3(KB), 0, st, scene->view(), L, projection, list, min_ray_dist, P, device_overflow_flag(s->dev));
    });
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipGetLastError());
    s->frames += 1;
    return 0;
}

int trhip_dshgi_get_timings(trhip_dshgi* s, trhip_dshgi_timings* out) {
    if (int r = stage_total_ms("trhip_dshgi_get_timings", s, out)) return r;
    snprintf(out->name, sizeof(out->name), "dshgi indirect");
    return 0;
}

int trhip_dshgi_download(trhip_dshgi* s, int which, void* host, size_t bytes) {
    return stage_download("trhip_dshgi_download", s, host, bytes, [&](const void*& src, size_t& size) {
        switch (which) {
            case TRHIP_DSHGI_INDIRECT: src = s->indirect; size = s->pixels() * sizeof(f4); break;
            case TRHIP_DSHGI_SURFACE:
                if (!s->surface) return set_error("trhip_dshgi_download: the surface record is only kept with record_surface");
                src = s->surface; size = s->pixels() * sizeof(DshgiSurface);
                break;
            default: return set_error("trhip_dshgi_download: unknown buffer");
        }
        return 0;
    });
}

}  // extern "C"
