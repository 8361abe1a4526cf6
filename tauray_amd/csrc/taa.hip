// Temporal antialiasing for gfx950: taa_stage (src/taa_stage.{hh,cc}, shader/taa.comp restated: k_taa) behind the entry points trhip_taa_*
// of include/trhip.h.  One kernel per frame: a 3 x 3 neighbourhood k-DOP of the mapped colours, edge dilation towards the nearest surface of
// the window, a bicubic read of the stage's history at the unjittered motion, the history clipped into the k-DOP and blended.  Constants,
// layouts and the order of operations: taa.h.  Everything is fp32 and evaluated without contraction in a fixed order, no atomics: two runs
// of the same inputs give the same bits.  Built with the flags of api.hip.
#include <cmath>
#include <cstring>
#include <string>

#include "taa.h"
#include "build.h"
#include "stage_host.h"

namespace tr {
namespace {

constexpr int KB = TAA_TILE * TAA_TILE;

struct TaaParams {
    int w, h;
    float gamma, inv_gamma, alpha;
    int perspective;
    uint base_camera;
    const CameraData* cameras;
    const CameraData* prev_cameras;
    const f4* src; f4* dst;      // dst may be null: the result is then only the new history
    const f2* motion; const f4* pos; const int* ids;      // pos: edge dilation only; ids may be null
    const f4* hist_in; f4* hist_out;
    uint8_t* decisions;
};

// The four functions of the colour map: float32 functions of a float32 argument, evaluated at double and rounded once (taa.h).  The
// device library's float versions are good to one or two ulps; TR_TAA_FLOAT_MAP=1 builds the kernel with them (a variant build, for
// measuring what the double evaluation costs: profiles/r13/taa.txt).
#ifndef TR_TAA_FLOAT_MAP
#define TR_TAA_FLOAT_MAP 0
#endif
#if TR_TAA_FLOAT_MAP
TR_DEV float log2_r1(float x) { return log2f(x); }
TR_DEV float exp2_r1(float x) { return exp2f(x); }
TR_DEV float log_r1(float x) { return logf(x); }
TR_DEV float exp_r1(float x) { return expf(x); }
#else
TR_DEV float log2_r1(float x) { return (float)log2((double)x); }
TR_DEV float exp2_r1(float x) { return (float)exp2((double)x); }
TR_DEV float log_r1(float x) { return (float)log((double)x); }
TR_DEV float exp_r1(float x) { return (float)exp((double)x); }
#endif

template <bool SHIMMER>
TR_DEV float map_channel(float c, float gamma) {
    float r = c <= 0.0f ? 0.0f : exp2_r1(gamma * log2_r1(c));
    if (SHIMMER) r = r > 1e-5f ? log_r1(r) : -10.0f;
    return r;
}

template <bool SHIMMER>
TR_DEV float unmap_channel(float c, float inv_gamma) {
    if (SHIMMER) c = exp_r1(c);
    return c <= 0.0f ? 0.0f : exp2_r1(inv_gamma * log2_r1(c));
}

template <bool SHIMMER>
TR_DEV f3 map_color(f3 c, float gamma) { return F3(map_channel<SHIMMER>(c.x, gamma), map_channel<SHIMMER>(c.y, gamma), map_channel<SHIMMER>(c.z, gamma)); }

TR_DEV f3 history_texel(const f4* hist, int w, int h, int x, int y) { return F3(hist[(size_t)clampi(y, 0, h - 1) * w + clampi(x, 0, w - 1)]); }

// One thread per output pixel: a workgroup is a 16 x 16 tile of layer blockIdx.z, a wave an 8 x 8 quarter of it.
template <bool EDGE, bool SHIMMER>
__global__ __launch_bounds__(KB) void k_taa(TaaParams P) {
    constexpr float AX[TAA_AXES][3] = {TAA_AXIS_TABLE};
    __shared__ f4 s_halo[TAA_HALO * TAA_HALO];      // mapped colour, depth
    const int w = P.w, h = P.h;
    const size_t base = (size_t)blockIdx.z * (size_t)w * h;
    const CameraData& cam = P.cameras[P.base_camera + blockIdx.z];
    const f3 cam_origin = F3(cam.origin), forward = F3(-cam.view_inverse.c[2].x, -cam.view_inverse.c[2].y, -cam.view_inverse.c[2].z);
    const int x0 = (int)blockIdx.x * TAA_TILE - 1, y0 = (int)blockIdx.y * TAA_TILE - 1;
    for (int i = (int)threadIdx.x; i < TAA_HALO * TAA_HALO; i += KB) {
        const int hy = i / TAA_HALO, hx = i - hy * TAA_HALO;
        const int gx = x0 + hx, gy = y0 + hy;
        const bool inside = gx >= 0 && gx < w && gy >= 0 && gy < h;
        const size_t q = base + (size_t)clampi(gy, 0, h - 1) * w + clampi(gx, 0, w - 1);
        const f3 m = map_color<SHIMMER>(F3(P.src[q]), P.gamma);
        float depth = __builtin_huge_valf();
        if (EDGE && inside && !(P.ids && P.ids[q] < 0)) depth = dot(F3(P.pos[q]) - cam_origin, forward);
        s_halo[i] = F4(m, depth);
    }
    __syncthreads();
    const uint t = threadIdx.x, wave = t >> 6, k = t & 63u;
    const int lx = (int)(((wave & 1u) << 3) + (k & 7u)), ly = (int)(((wave >> 1) << 3) + (k >> 3));
    const int x = (int)blockIdx.x * TAA_TILE + lx, y = (int)blockIdx.y * TAA_TILE + ly;
    if (x >= w || y >= h) return;
    const size_t pix = base + (size_t)y * w + x;
    const f4 src = P.src[pix];
    const f4 col = F4(src.x, src.y, src.z, src.w);      // by component: copied as a block, the struct would live in memory (LDS) for the whole kernel
    const f3 m = F3(s_halo[(ly + 1) * TAA_HALO + lx + 1]);

    float lo[TAA_AXES], hi[TAA_AXES];
#pragma unroll
    for (int a = 0; a < TAA_AXES; ++a) {
        const float r = dot(m, F3(AX[a][0], AX[a][1], AX[a][2]));
        lo[a] = r - TAA_KDOP_DILATION; hi[a] = r + TAA_KDOP_DILATION;
    }
    float closest = __builtin_huge_valf();
    int ox = 0, oy = 0;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const f4 n = s_halo[(ly + 1 + dy) * TAA_HALO + lx + 1 + dx];
            if (EDGE && n.w < closest) { closest = n.w; ox = dx; oy = dy; }
            if (dx == 0 && dy == 0) continue;
#pragma unroll
            for (int a = 0; a < TAA_AXES; ++a) {
                const float r = dot(F3(n), F3(AX[a][0], AX[a][1], AX[a][2]));
                lo[a] = fminf(r - TAA_KDOP_DILATION, lo[a]);
                hi[a] = fmaxf(r + TAA_KDOP_DILATION, hi[a]);
            }
        }
    }

    // the motion of the nearest pixel of the window, without this frame's and last frame's jitter
    const size_t mq = base + (size_t)(y + oy) * w + (x + ox);      // inside the image: an outside neighbour has depth +inf and is never chosen
    f2 motion = P.motion[mq];
    const bool nosurf = P.ids ? P.ids[mq] < 0 : (isnan(motion.x) || isnan(motion.y));
    const CameraData& prev = P.prev_cameras[P.base_camera + blockIdx.z];
    if (nosurf && P.perspective) {
        const float u = (((float)x + 0.5f) / (float)w) * 2.0f - 1.0f, v = (((float)h - ((float)y + 0.5f)) / (float)h) * 2.0f - 1.0f;
        const f4 tv = mul(cam.proj_inverse, F4(u, v, 1.0f, 1.0f));
        const f3 dir = normalize(F3(mul(cam.view_inverse, F4(tv.x, tv.y, tv.z, 0.0f))));
        const f4 c = mul(prev.view_proj, F4(dir, 0.0f));
        motion = F2((c.x / c.w) * 0.5f + 0.5f, (c.y / c.w) * 0.5f + 0.5f);
    }
    motion = F2(motion.x + (prev.pan.z - cam.pan.z) * 0.5f, motion.y + (prev.pan.w - cam.pan.w) * 0.5f);
    const float psx = 1.0f / (float)w, psy = 1.0f / (float)h;
    const float uvx = motion.x - (float)ox * psx, uvy = (1.0f - motion.y) - (float)oy * psy;
    uint8_t decision = (uint8_t)((ox + 1) * 3 + (oy + 1)) | (nosurf ? TAA_DECISION_NO_SURFACE : 0);
    if (!(uvx >= 0.0f) || !(uvy >= 0.0f) || uvx > 1.0f + 2.0f * psx || uvy > 1.0f + 2.0f * psy) {
        if (P.dst) P.dst[pix] = col;
        P.hist_out[pix] = col;
        P.decisions[pix] = decision | TAA_DECISION_OUTSIDE;
        return;
    }

    // bicubic history (Catmull-Rom through five bilinear fetches, as twelve texels)
    const f4* hist = P.hist_in + base;
    const float posx = uvx * (float)w, posy = uvy * (float)h;
    const float cxf = floorf(posx - 0.5f), cyf = floorf(posy - 0.5f);
    const float fx = posx - (cxf + 0.5f), fy = posy - (cyf + 0.5f);
    const int cx = (int)cxf, cy = (int)cyf;
    const float fx2 = fx * fx, fx3 = fx * fx2, fy2 = fy * fy, fy3 = fy * fy2;
    const float w0x = (-0.5f * fx3 + fx2) - 0.5f * fx, w1x = (1.5f * fx3 - 2.5f * fx2) + 1.0f, w2x = (-1.5f * fx3 + 2.0f * fx2) + 0.5f * fx, w3x = 0.5f * fx3 - 0.5f * fx2;
    const float w0y = (-0.5f * fy3 + fy2) - 0.5f * fy, w1y = (1.5f * fy3 - 2.5f * fy2) + 1.0f, w2y = (-1.5f * fy3 + 2.0f * fy2) + 0.5f * fy, w3y = 0.5f * fy3 - 0.5f * fy2;
    const float w12x = w1x + w2x, w12y = w1y + w2y;
    const float qx = w2x / w12x, qy = w2y / w12y;
    const f3 A = mix3(history_texel(hist, w, h, cx, cy - 1), history_texel(hist, w, h, cx + 1, cy - 1), qx);
    const f3 B = mix3(history_texel(hist, w, h, cx - 1, cy), history_texel(hist, w, h, cx - 1, cy + 1), qy);
    const f3 Cc = mix3(mix3(history_texel(hist, w, h, cx, cy), history_texel(hist, w, h, cx + 1, cy), qx),
                       mix3(history_texel(hist, w, h, cx, cy + 1), history_texel(hist, w, h, cx + 1, cy + 1), qx), qy);
    const f3 D = mix3(history_texel(hist, w, h, cx + 2, cy), history_texel(hist, w, h, cx + 2, cy + 1), qy);
    const f3 E = mix3(history_texel(hist, w, h, cx, cy + 2), history_texel(hist, w, h, cx + 1, cy + 2), qx);
    const float wa = w12x * w0y, wb = w0x * w12y, wc = w12x * w12y, wd = w3x * w12y, we = w12x * w3y;
    const float total_w = (((wa + wb) + wc) + wd) + we;
    const f3 sum = (((A * wa + B * wb) + Cc * wc) + D * wd) + E * we;
    const f3 prev_col = max3(sum / total_w, F3(0.0f));

    // clip the history into the window's k-DOP along the line towards this frame's colour, blend
    const f3 delta = map_color<SHIMMER>(prev_col, P.gamma) - m;
    float near = -1e9f, far = 1e9f;
#pragma unroll
    for (int a = 0; a < TAA_AXES; ++a) {
        const f3 axis = F3(AX[a][0], AX[a][1], AX[a][2]);
        const float inv = 1.0f / dot(delta, axis), pp = dot(m, axis);
        const float t0 = (lo[a] - pp) * inv, t1 = (hi[a] - pp) * inv;
        near = fmaxf(near, fminf(t0, t1));
        far = fminf(far, fmaxf(t0, t1));
    }
    const float tt = (near <= far && (near > 0.0f || far > 0.0f)) ? (near > 0.0f ? near : far) : -1.0f;
    const float len = clampf(tt, 0.0f, 1.0f);
    const f3 mixed = mix3(m + len * delta, m, P.alpha);
    const f4 out = F4(unmap_channel<SHIMMER>(mixed.x, P.inv_gamma), unmap_channel<SHIMMER>(mixed.y, P.inv_gamma), unmap_channel<SHIMMER>(mixed.z, P.inv_gamma), col.w);
    if (P.dst) P.dst[pix] = out;
    P.hist_out[pix] = out;
    P.decisions[pix] = decision;
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_taa : StageHost<> {
    trhip_device* dev = nullptr;
    uint32_t w = 0, h = 0, layers = 0;
    trhip_taa_options opt = {};
    int cur = 0;                         // the history a frame reads; it writes cur ^ 1
    bool have_history = false;
    f4* history[2] = {};
    uint8_t* decisions = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
};

extern "C" {

int trhip_taa_create(trhip_device* dev, const trhip_taa_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_taa** out) {
    if (!out) return set_error("trhip_taa_create: null out");
    *out = nullptr;
    if (!opt) return set_error("trhip_taa_create: null options");
    if (width == 0 || height == 0 || layers == 0) return set_error("trhip_taa_create: zero width, height or layer count");
    if (width > 16384 || height > 16384 || layers > 4096) return set_error("trhip_taa_create: image too large");
    if (!(opt->alpha > 0.0f) || !(opt->alpha <= 1.0f)) return set_error("trhip_taa_create: alpha must be in (0, 1]");
    if (!(opt->gamma > 0.0f) || std::isinf(opt->gamma)) return set_error("trhip_taa_create: gamma must be positive and finite");
    if (opt->projection == 2)
        return set_error("trhip_taa_create: equirectangular cameras: the stage projects a miss's ray direction with the previous camera's view_proj, "
                         "which an equirectangular camera does not have (shader/taa.comp has no projected-direction function for it)");
    if (opt->projection != 0 && opt->projection != 1) return set_error("trhip_taa_create: unknown projection " + std::to_string(opt->projection));
    if (!dev) return set_error("trhip_taa_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_taa* t = new trhip_taa;
    t->dev = dev; t->hip_device = device_index(dev);
    t->w = width; t->h = height; t->layers = layers; t->opt = *opt;
    const size_t px = t->pixels();
    for (int i = 0; i < 2; ++i) t->alloc_zeroed(t->history[i], px * sizeof(f4));
    t->alloc_zeroed(t->decisions, px);
    return stage_finish_create("trhip_taa_create", t, out);
}

void trhip_taa_destroy(trhip_taa* t) { stage_destroy(t); }

int trhip_taa_reset_history(trhip_taa* t) {
    if (!t) return set_error("trhip_taa_reset_history: null stage");
    t->have_history = false;
    return 0;
}

int trhip_taa_run(trhip_taa* t, const trhip_taa_images* images, void* stream) {
    if (!t) return set_error("trhip_taa_run: null stage");
    if (!images) return set_error("trhip_taa_run: null images");
    if (!images->src || !images->dst || !images->screen_motion) return set_error("trhip_taa_run: src, dst and screen_motion are required");
    if (t->opt.edge_dilation && !images->pos) return set_error("trhip_taa_run: edge dilation reads pos");
    const size_t bytes = t->pixels() * sizeof(f4);
    const char* s = (const char*)images->src;
    const char* d = (const char*)images->dst;
    if (d != s && d < s + bytes && s < d + bytes) return set_error("trhip_taa_run: dst overlaps src without being src");
    DEVCHK(t->hip_device);
    DeviceScene* scene = device_scene(t->dev);
    if (!scene->cameras || (uint64_t)t->opt.base_camera_index + t->layers > scene->camera_count)
        return set_error("trhip_taa_run: the scene has " + std::to_string(scene->camera_count) + " cameras, the stage reads " + std::to_string(t->layers) +
                         " from " + std::to_string(t->opt.base_camera_index));
    TaaParams P{};
    P.w = (int)t->w; P.h = (int)t->h;
    P.gamma = t->opt.gamma; P.inv_gamma = 1.0f / t->opt.gamma; P.alpha = t->have_history ? t->opt.alpha : 1.0f;
    P.perspective = t->opt.projection == 0 ? 1 : 0;
    P.base_camera = t->opt.base_camera_index;
    P.cameras = scene->cameras; P.prev_cameras = scene->prev_cameras ? scene->prev_cameras : scene->cameras;
    const bool aliased = d == s;      // a tile reads the halo of src that its neighbours own: the result goes through the new history
    P.src = (const f4*)images->src; P.dst = aliased ? nullptr : (f4*)images->dst;
    P.motion = (const f2*)images->screen_motion; P.pos = (const f4*)images->pos; P.ids = (const int*)images->instance_id;
    const int c = t->cur, nx = c ^ 1;
    P.hist_in = t->history[c]; P.hist_out = t->history[nx]; P.decisions = t->decisions;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((t->w + TAA_TILE - 1) / TAA_TILE, (t->h + TAA_TILE - 1) / TAA_TILE, t->layers);
    const bool edge = t->opt.edge_dilation != 0, shimmer = t->opt.anti_shimmer != 0;
    HIPCHK(hipEventRecord(t->ev[0], st));
    if (edge && shimmer) hipLaunchKernelGGL((k_taa<true, true>), grid, dim3(KB), 0, st, P);
    else if (edge) hipLaunchKernelGGL((k_taa<true, false>), grid, dim3(KB), 0, st, P);
    else if (shimmer) hipLaunchKernelGGL((k_taa<false, true>), grid, dim3(KB), 0, st, P);
    else hipLaunchKernelGGL((k_taa<false, false>), grid, dim3(KB), 0, st, P);
    if (aliased) HIPCHK(hipMemcpyAsync(images->dst, t->history[nx], bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(t->ev[1], st));
    HIPCHK(hipGetLastError());
    t->cur = nx;
    t->have_history = true;
    t->frames += 1;
    return 0;
}

int trhip_taa_get_timings(trhip_taa* t, trhip_taa_timings* out) {
    const int r = stage_total_ms("trhip_taa_get_timings", t, out);
    if (t && out) snprintf(out->name, sizeof(out->name), "temporal antialiasing (%u viewports)", t->layers);
    return r;
}

int trhip_taa_download(trhip_taa* t, int which, void* host, size_t bytes) {
    return stage_download("trhip_taa_download", t, host, bytes, [&](const void*& src, size_t& size) {
        switch (which) {
            case TRHIP_TAA_HISTORY: src = t->history[t->cur]; size = t->pixels() * sizeof(f4); break;
            case TRHIP_TAA_DECISIONS: src = t->decisions; size = t->pixels(); break;
            default: return set_error("trhip_taa_download: unknown buffer");
        }
        return 0;
    });
}

}  // extern "C"
