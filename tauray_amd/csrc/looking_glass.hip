// Looking Glass output for gfx950: looking_glass_composition_stage (src/looking_glass_composition_stage.{hh,cc},
// shader/looking_glass_composition.comp restated: k_looking_glass) behind the entry points trhip_lkg_* of include/trhip.h.  One kernel per
// frame interleaves the N views of a light field, sub-pixel by sub-pixel, into the one image a lenticular panel shows.  Constants, layouts
// and the order of operations: looking_glass.h.  Everything is fp32 and evaluated without contraction in a fixed order, no atomics, no
// state between frames: two runs of the same inputs give the same bits.  Built with the flags of api.hip.
#include <cmath>
#include <cstring>
#include <string>

#include "looking_glass.h"
#include "stage_host.h"

namespace tr {
namespace {

struct LkgParams {
    int W, H;              // output
    int w, h;              // one view
    int views;
    f4 cal;
    const float* src;
    f4* dst;               // may be null
    uint* dst8;            // may be null; one packed r | g << 8 | b << 16 | a << 24 per pixel
    uint* indices;         // RECORD only
};

TR_DEV uint quantise(float c) {
    const float cc = c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f;
    return (uint)(cc * 255.0f + 0.5f);
}

// One thread per output pixel; threadIdx.x is the lane, so a wave stores 64 consecutive pixels of one row (1 KiB of dst in one instruction).
// Each of the 12 taps reads the one channel it needs: the three channels of a pixel come from up to three different views.
template <bool RECORD>
__global__ __launch_bounds__(LKG_WAVE * LKG_ROWS) void k_looking_glass(LkgParams P) {
    const int x = (int)(blockIdx.x * LKG_WAVE + threadIdx.x);
    const int y = (int)(blockIdx.y * LKG_ROWS + threadIdx.y);
    if (x >= P.W || y >= P.H) return;
    const float uvx = ((float)x + 0.5f) / (float)P.W;
    const float uvy = ((float)y + 0.5f) / (float)P.H;
    const float uvfy = 1.0f - uvy;

    const float px = uvx * (float)P.w - 0.5f, py = uvy * (float)P.h - 0.5f;
    const float fx = floorf(px), fy = floorf(py);
    const float wx = px - fx, wy = py - fy;
    const int x0 = clampi((int)fx, 0, P.w - 1), x1 = clampi((int)fx + 1, 0, P.w - 1);
    const int y0 = clampi((int)fy, 0, P.h - 1), y1 = clampi((int)fy + 1, 0, P.h - 1);
    const size_t o00 = ((size_t)y0 * P.w + x0) * 4, o10 = ((size_t)y0 * P.w + x1) * 4;
    const size_t o01 = ((size_t)y1 * P.w + x0) * 4, o11 = ((size_t)y1 * P.w + x1) * 4;
    const size_t view_stride = (size_t)P.w * P.h * 4;

    const float base = uvx * P.cal.x + uvfy * P.cal.y;
    int view[3];
    float t[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = (base + (float)c * P.cal.z) + P.cal.w;
        const float hh = d - floorf(d);
        const float hv = floorf(hh * (float)P.views);
        view[c] = hv >= 0.0f ? clampi((int)fmin2(hv, (float)LKG_MAX_VIEWS), 0, P.views - 1) : 0;      // a d that is not finite selects view 0
        const float* v = P.src + (size_t)view[c] * view_stride + c;
        t[c][0] = v[o00]; t[c][1] = v[o10]; t[c][2] = v[o01]; t[c][3] = v[o11];
    }
    float out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = t[c][0] * (1.0f - wx) + t[c][1] * wx;
        const float bottom = t[c][2] * (1.0f - wx) + t[c][3] * wx;
        out[c] = top * (1.0f - wy) + bottom * wy;
    }
    const size_t p = (size_t)y * P.W + x;
    if (P.dst) P.dst[p] = F4(out[0], out[1], out[2], 1.0f);
    if (P.dst8) P.dst8[p] = quantise(out[0]) | (quantise(out[1]) << 8) | (quantise(out[2]) << 16) | 0xFF000000u;
    if (RECORD) P.indices[p] = (uint)view[0] | ((uint)view[1] << 8) | ((uint)view[2] << 16);
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_lkg : StageHost<> {
    trhip_device* dev = nullptr;
    uint32_t view_w = 0, view_h = 0, out_w = 0, out_h = 0;
    trhip_lkg_options opt = {};
    f4 cal = {};
    uint* indices = nullptr;
    size_t pixels() const { return (size_t)out_w * out_h; }
};

extern "C" {

int trhip_lkg_create(trhip_device* dev, const trhip_lkg_options* opt, uint32_t view_w, uint32_t view_h, uint32_t out_w, uint32_t out_h, trhip_lkg** out) {
    if (!out) return set_error("trhip_lkg_create: null out");
    *out = nullptr;
    if (!opt) return set_error("trhip_lkg_create: null options");
    if (view_w == 0 || view_h == 0 || out_w == 0 || out_h == 0) return set_error("trhip_lkg_create: zero view or output size");
    if (view_w > LKG_MAX_EXTENT || view_h > LKG_MAX_EXTENT || out_w > LKG_MAX_EXTENT || out_h > LKG_MAX_EXTENT) return set_error("trhip_lkg_create: image too large");
    if (opt->viewport_count == 0 || opt->viewport_count > LKG_MAX_VIEWS)
        return set_error("trhip_lkg_create: viewport_count " + std::to_string(opt->viewport_count) + " is not in 1..255 (a recorded view index is one byte)");
    if (!std::isfinite(opt->pitch) || !std::isfinite(opt->tilt) || !std::isfinite(opt->center)) return set_error("trhip_lkg_create: pitch, tilt and center must be finite");
    if (!dev) return set_error("trhip_lkg_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_lkg* t = new trhip_lkg;
    t->dev = dev; t->hip_device = device_index(dev);
    t->view_w = view_w; t->view_h = view_h; t->out_w = out_w; t->out_h = out_h; t->opt = *opt;
    // looking_glass_composition_stage.cc:61-68, in float and in exactly this form
    t->cal = F4(opt->pitch, opt->tilt * opt->pitch, opt->pitch / (3.0f * (float)out_w), -opt->center);
    if (opt->invert) t->cal = F4(-t->cal.x, -t->cal.y, -t->cal.z, -t->cal.w);
    if (opt->record_view_indices) t->alloc_zeroed(t->indices, t->pixels() * 4);
    return stage_finish_create("trhip_lkg_create", t, out);
}

void trhip_lkg_destroy(trhip_lkg* t) { stage_destroy(t); }

int trhip_lkg_run(trhip_lkg* t, const void* src, void* dst, void* dst_rgba8, void* stream) {
    if (!t) return set_error("trhip_lkg_run: null stage");
    if (!src) return set_error("trhip_lkg_run: null src");
    if (!dst && !dst_rgba8) return set_error("trhip_lkg_run: dst and dst_rgba8 are both null: the frame would go nowhere");
    DEVCHK(t->hip_device);
    LkgParams P{};
    P.W = (int)t->out_w; P.H = (int)t->out_h; P.w = (int)t->view_w; P.h = (int)t->view_h;
    P.views = (int)t->opt.viewport_count;
    P.cal = t->cal;
    P.src = (const float*)src; P.dst = (f4*)dst; P.dst8 = (uint*)dst_rgba8; P.indices = t->indices;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((t->out_w + LKG_WAVE - 1) / LKG_WAVE, (t->out_h + LKG_ROWS - 1) / LKG_ROWS), block(LKG_WAVE, LKG_ROWS);
    HIPCHK(hipEventRecord(t->ev[0], st));
    if (t->indices) hipLaunchKernelGGL((k_looking_glass<true>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_looking_glass<false>), grid, block, 0, st, P);
    HIPCHK(hipEventRecord(t->ev[1], st));
    HIPCHK(hipGetLastError());
    t->frames += 1;
    return 0;
}

int trhip_lkg_get_timings(trhip_lkg* t, trhip_lkg_timings* out) {
    const int r = stage_total_ms("trhip_lkg_get_timings", t, out);
    if (t && out) snprintf(out->name, sizeof(out->name), "looking glass composition");
    return r;
}

int trhip_lkg_download(trhip_lkg* t, int which, void* host, size_t bytes) {
    return stage_download("trhip_lkg_download", t, host, bytes, [&](const void*& src, size_t& size) {
        if (which != TRHIP_LKG_VIEW_INDICES) return set_error("trhip_lkg_download: unknown buffer");
        if (!t->indices) return set_error("trhip_lkg_download: the stage was created without record_view_indices");
        src = t->indices; size = t->pixels() * 4;
        return 0;
    });
}

}  // extern "C"
