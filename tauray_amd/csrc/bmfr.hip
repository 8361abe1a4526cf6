// bmfr_stage for gfx950 (src/bmfr_stage.{hh,cc}; shader/bmfr_preprocess.comp, bmfr_fit.comp, bmfr_weighted_sum.comp,
// bmfr_accumulate_output.comp restated): k_bmfr_preprocess -> k_bmfr_fit -> k_bmfr_weighted_sum -> k_bmfr_accumulate_output, and the
// entry points trhip_bmfr_* of include/trhip.h.  Layouts: bmfr.h.  Everything is fp32 and evaluated without contraction in a fixed
// order: no atomics, two runs of the same inputs give the same bits.
#include <cmath>
#include <string>

#include "bmfr.h"
#include "stage_host.h"
#include "taps.h"
#include "rng.h"

namespace tr {
namespace {

struct BmfrParams {
    int w, h, layers, bw, bh, channels, nc;
    int shift_x, shift_y;            // -16 + offset[frame % 16]: image pixel = block-grid pixel + shift
    uint frame;
    int have_history;
    float noise;
    f4* color;
    const f4 *diffuse, *albedo, *pos;
    const f2 *normal, *motion;
    const int* instance_id;
    const f4* noisy_prev[2];  f4* noisy_cur[2];      // [0] diffuse (a = history length), [1] specular
    const f4* filt_prev[2];   f4* filt_cur[2];
    const f2* normal_prev;    f2* normal_cur;
    const f4* pos_prev;       f4* pos_cur;           // w = 1: no surface
    float *rows, *weights, *minmax;
    f4* weighted[2];
    uint8_t* accept;
};

TR_DEV float nan_to_zero(float v) { return isnan(v) ? 0.0f : v; }

TR_DEV int mirror_index(int i, int size) {
    if (i < 0) i = -i - 1;
    else if (i >= size) i = 2 * size - i - 1;
    return clampi(i, 0, size - 1);      // an image narrower than the margin
}

TR_DEV float scale_feature(float v, float lo, float hi) {
    const float range = hi - lo;
    return fabsf(range) > 1.0f ? (v - lo) / range : v - lo;
}

TR_DEV bool keep_tap(const BmfrParams& P, int x, int y, int z, f3 n, f3 p) {
    if (x < 0 || y < 0 || x >= P.w || y >= P.h) return false;
    const size_t s = ((size_t)z * P.h + y) * P.w + x;
    const f4 pp = P.pos_prev[s];
    if (pp.w != 0.0f) return false;
    const f3 d = p - F3(pp);
    const f3 np = octahedral_unpack(P.normal_prev[s]);
    const float cosn = dot(np, n);
    const float d2 = dot(d, d);
    float wgt = 1.0f;
    if (!(d2 < 0.001f)) {
        const f3 t = d / sqrtf(d2);
        wgt = clampf(1.0f - fabsf(dot(t, n)), 0.0f, 1.0f) * clampf(cosn, 0.0f, 1.0f);
    }
    return cosn > 0.9f && wgt > 0.5f;
}

TR_DEV f4 blend_taps(const f4* img, const BmfrParams& P, int tx, int ty, int z, uint bits, const float cw[4]) {
    f4 r = F4(0.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f4 t = F4(0.0f);
        if (bits & (1u << k)) t = img[((size_t)z * P.h + (ty + (k >> 1))) * P.w + (tx + (k & 1))];
        r = r + t * cw[k];
    }
    return r;
}

// (a) one thread per pixel of the block grid; a workgroup is a quarter (32 x 8) of a block, so every column store is 256 floats in a row.
__global__ __launch_bounds__(256) void k_bmfr_preprocess(BmfrParams P) {
    const int bx = blockIdx.x, by = blockIdx.y >> 2, z = blockIdx.z;
    const int xib = threadIdx.x & 31, yib = ((blockIdx.y & 3) << 3) + (threadIdx.x >> 5);
    const int ux = bx * 32 + xib + P.shift_x, uy = by * 32 + yib + P.shift_y;
    const int px = mirror_index(ux, P.w), py = mirror_index(uy, P.h);
    const bool own = ux == px && uy == py;           // not a mirrored copy: this thread writes the pixel's own outputs
    const size_t pix = ((size_t)z * P.h + py) * P.w + px;

    const f4 col = P.color[pix], dif = P.diffuse[pix], alb = P.albedo[pix], pp = P.pos[pix];
    const f3 n = octahedral_unpack(P.normal[pix]);
    const f3 p = F3(pp);
    const bool nosurf = any_nan(p) || (P.instance_id && P.instance_id[pix] < 0);
    f3 diffuse = F3(dif);
    f3 specular = max3(F3(0.0f), F3(col) - F3(alb) * F3(dif));
    float hist_len = 1.0f;

    uint bits = 0;
    if (P.have_history && !nosurf) {
        int tx, ty; float qx, qy;
        tap_position(P.motion[pix], P.w, P.h, tx, ty, qx, qy);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (keep_tap(P, tx + (k & 1), ty + (k >> 1), z, n, p)) bits |= 1u << k;
        float cw[4];
        const float sum_w = tap_weights(qx, qy, bits, cw);
        if (sum_w > 1e-5f) {
            const f4 dprev = blend_taps(P.noisy_prev[0], P, tx, ty, z, bits, cw);
            const f4 sprev = blend_taps(P.noisy_prev[1], P, tx, ty, z, bits, cw);
            if (sum_w > 0.001f && !(isnan(dprev.x) || isnan(dprev.y) || isnan(dprev.z) || isnan(dprev.w))) {
                hist_len = fmin2(dprev.w + 1.0f, 255.0f);
                const float alpha = clampf(1.0f / hist_len, 0.01f, 1.0f);
                diffuse = mix3(F3(dprev), diffuse, alpha);
                specular = mix3(F3(sprev), specular, alpha);
            }
        }
    }
    diffuse = F3(nan_to_zero(diffuse.x), nan_to_zero(diffuse.y), nan_to_zero(diffuse.z));
    specular = F3(nan_to_zero(specular.x), nan_to_zero(specular.y), nan_to_zero(specular.z));
    if (own) {
        P.noisy_cur[0][pix] = F4(diffuse, hist_len);
        P.noisy_cur[1][pix] = F4(specular, 1.0f);
        P.accept[pix] = (uint8_t)(bits | (nosurf ? 16u : 0u));
    }

    float row[16];
    row[0] = 1.0f;
    row[1] = n.x; row[2] = n.y; row[3] = n.z;
    row[4] = p.x; row[5] = p.y; row[6] = p.z;
    row[7] = p.x * p.x; row[8] = p.y * p.y; row[9] = p.z * p.z;
    row[10] = diffuse.x; row[11] = diffuse.y; row[12] = diffuse.z;
    row[13] = specular.x; row[14] = specular.y; row[15] = specular.z;
    const size_t blk = ((size_t)z * P.bh + by) * P.bw + bx;
    float* out = P.rows + blk * P.nc * BMFR_BLOCK_PIXELS + yib * 32 + xib;
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < P.nc) out[(size_t)c * BMFR_BLOCK_PIXELS] = nosurf ? 0.0f : nan_to_zero(row[c]);
}

TR_DEV float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
TR_DEV float wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin2(v, __shfl_xor(v, m));
    return v;
}
TR_DEV float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax2(v, __shfl_xor(v, m));
    return v;
}

// (b) one workgroup of 256 threads per block and layer.  Thread t holds rows t, t + 256, t + 512, t + 768 of the block's
// 1024 x NC matrix [features | channels] in registers.  Householder QR, one pivot column after the other; per pivot ONE batched
// reduction gives the squared norm of the pivot column below the diagonal and its dot products with every remaining column at once
// (the reflector v = x - alpha e_k needs nothing else: v.a_j = x.a_j - alpha a_kj, v.v = 2 (x.x - alpha x_k)): wave sums by __shfl_xor,
// the four waves through 256 bytes of LDS that alternate between pivots, so a pivot costs one barrier.  alpha takes the sign that
// avoids cancellation in v_k.  R (10 x NC) goes to LDS row by row; NC - 10 threads substitute back.  A zero pivot column leaves its
// reflection out and its weight 0.
// PREPARED = false (the stage): the rows are unscaled and without noise; features 4-9 are scaled to the block's min / max over the
// rows with a surface (kept for the weighted sum), and noise * 2 (u - 0.5) is added to features 1-9 of those rows,
// u = pcg4d(x, y, layer * 16 + feature, frame).x over the block-grid pixel (x, y).  PREPARED = true (trhip_bmfr_fit_blocks): the
// matrix is taken as it is.
template <int NC, bool PREPARED>
__global__ __launch_bounds__(256) void k_bmfr_fit(const float* __restrict__ rows, float* __restrict__ weights, float* __restrict__ minmax,
                                                  int bw, int bh, uint frame, float noise) {
    constexpr int NF = BMFR_FEATURES, C = NC - NF;
    __shared__ float s_part[2][4][16];
    __shared__ float s_piv[2][16];
    __shared__ float s_R[NF][16];
    __shared__ float s_mm[4][12];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const size_t blk = blockIdx.x;
    const float* M = rows + blk * NC * BMFR_BLOCK_PIXELS;

    float a[4][NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][c] = M[c * BMFR_BLOCK_PIXELS + i * 256 + t];

    if (!PREPARED) {
        float lo[6], hi[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            lo[f] = 3.402823466e+38f; hi[f] = -3.402823466e+38f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (a[i][0] != 0.0f) { lo[f] = fmin2(lo[f], a[i][4 + f]); hi[f] = fmax2(hi[f], a[i][4 + f]); }
            lo[f] = wave_min(lo[f]); hi[f] = wave_max(hi[f]);
            if (lane == 0) { s_mm[wave][2 * f] = lo[f]; s_mm[wave][2 * f + 1] = hi[f]; }
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            lo[f] = fmin2(fmin2(s_mm[0][2 * f], s_mm[1][2 * f]), fmin2(s_mm[2][2 * f], s_mm[3][2 * f]));
            hi[f] = fmax2(fmax2(s_mm[0][2 * f + 1], s_mm[1][2 * f + 1]), fmax2(s_mm[2][2 * f + 1], s_mm[3][2 * f + 1]));
            if (lo[f] > hi[f]) { lo[f] = 0.0f; hi[f] = 0.0f; }      // no row with a surface
            if (t == 0) { minmax[(blk * 6 + f) * 2] = lo[f]; minmax[(blk * 6 + f) * 2 + 1] = hi[f]; }
        }
        const uint per_layer = (uint)(bw * bh);
        const uint layer = (uint)blk / per_layer, in_layer = (uint)blk % per_layer;
        const uint gx0 = (in_layer % (uint)bw) * 32u, gy0 = (in_layer / (uint)bw) * 32u;
        const float amp = noise * 2.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (a[i][0] == 0.0f) continue;
            const uint r = (uint)(i * 256 + t);
#pragma unroll
            for (int f = 0; f < 6; ++f) a[i][4 + f] = scale_feature(a[i][4 + f], lo[f], hi[f]);
#pragma unroll
            for (int c = 1; c < NF; ++c) {
                u4 s = {gx0 + (r & 31u), gy0 + (r >> 5), layer * 16u + (uint)c, frame};
                const float u = (float)pcg4d(s).x * TR_INV_UINT32_MAX;
                a[i][c] = a[i][c] + amp * (u - 0.5f);
            }
        }
    }

#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const int buf = k & 1;
        const bool act0 = t >= k;                 // rows 0 .. k-1 (threads 0 .. k-1, slot 0) already hold rows of R
#pragma unroll
        for (int j = k; j < NC; ++j) {
            float s = act0 ? a[0][k] * a[0][j] : 0.0f;
#pragma unroll
            for (int i = 1; i < 4; ++i) s = s + a[i][k] * a[i][j];
            s = wave_sum(s);
            if (lane == 0) s_part[buf][wave][j] = s;
        }
        if (t == k) {
#pragma unroll
            for (int j = k; j < NC; ++j) s_piv[buf][j] = a[0][j];
        }
        __syncthreads();
        const float norm2 = (s_part[buf][0][k] + s_part[buf][1][k]) + (s_part[buf][2][k] + s_part[buf][3][k]);
        const float xk = s_piv[buf][k];
        const float norm = sqrtf(norm2);
        float alpha = xk > 0.0f ? -norm : norm;
        const float vv = 2.0f * (norm2 - alpha * xk);
        const bool reflect = norm2 > 0.0f && vv > 0.0f && vv < 3.402823466e+38f;
        if (!reflect) alpha = xk;                 // the column stays as it is (zero below the diagonal, or not finite)
        const float vk = xk - alpha;
        if (reflect) {
#pragma unroll
            for (int j = k + 1; j < NC; ++j) {
                const float d = (s_part[buf][0][j] + s_part[buf][1][j]) + (s_part[buf][2][j] + s_part[buf][3][j]);
                const float tau = 2.0f * (d - alpha * s_piv[buf][j]) / vv;
                if (act0) a[0][j] = a[0][j] - (t == k ? vk : a[0][k]) * tau;
#pragma unroll
                for (int i = 1; i < 4; ++i) a[i][j] = a[i][j] - a[i][k] * tau;
            }
        }
        if (t == k) {
            s_R[k][k] = alpha;
#pragma unroll
            for (int j = k + 1; j < NC; ++j) s_R[k][j] = a[0][j];
        }
    }
    __syncthreads();
    if (t < C) {
        float wv[NF];
#pragma unroll
        for (int i = NF - 1; i >= 0; --i) {
            float s = s_R[i][NF + t];
#pragma unroll
            for (int j = i + 1; j < NF; ++j) s = s - s_R[i][j] * wv[j];
            const float d = s_R[i][i];
            float x = d != 0.0f ? s / d : 0.0f;
            if (!(fabsf(x) < 3.402823466e+38f)) x = 0.0f;      // NaN or Inf: the feature drops out
            wv[i] = x;
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) weights[(blk * C + t) * NF + i] = wv[i];
    }
}

// (c) per pixel: the features again, without noise, scaled with the block's min / max, times the block's weights, clamped at 0
__global__ __launch_bounds__(256) void k_bmfr_weighted_sum(BmfrParams P) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)P.w * P.h * P.layers;
    if (i >= n) return;
    const int px = (int)(i % P.w), py = (int)((i / P.w) % P.h), z = (int)(i / ((size_t)P.w * P.h));
    const int bx = (px - P.shift_x) >> 5, by = (py - P.shift_y) >> 5;
    const size_t blk = ((size_t)z * P.bh + by) * P.bw + bx;
    const f4 pp = P.pos[i];
    const f3 p = F3(pp);
    const bool nosurf = any_nan(p) || (P.instance_id && P.instance_id[i] < 0);
    const f3 nrm = octahedral_unpack(P.normal[i]);
    float f[BMFR_FEATURES] = {1.0f, nrm.x, nrm.y, nrm.z, p.x, p.y, p.z, p.x * p.x, p.y * p.y, p.z * p.z};
    const float* mm = P.minmax + blk * 12;
#pragma unroll
    for (int k = 0; k < BMFR_FEATURES; ++k) {
        f[k] = nosurf ? 0.0f : nan_to_zero(f[k]);
        if (k >= 4 && !nosurf) f[k] = scale_feature(f[k], mm[(k - 4) * 2], mm[(k - 4) * 2 + 1]);
    }
    const float* wgt = P.weights + blk * P.channels * BMFR_FEATURES;
    for (int set = 0; set < P.channels / 3; ++set) {
        float c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < BMFR_FEATURES; ++k) s = s + wgt[(set * 3 + ch) * BMFR_FEATURES + k] * f[k];
            c[ch] = fmax2(s, 0.0f);
        }
        P.weighted[set][i] = F4(c[0], c[1], c[2], 1.0f);
    }
}

// (d) per pixel: the taps (a) kept, of the history of filtered values; alpha from the history length BEFORE the increment; the
// denoised colour; this frame's normal and position become the next frame's previous ones.
__global__ __launch_bounds__(256) void k_bmfr_accumulate_output(BmfrParams P) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)P.w * P.h * P.layers;
    if (i >= n) return;
    const int z = (int)(i / ((size_t)P.w * P.h));
    const uint accepts = P.accept[i];
    const uint bits = accepts & 15u;
    f4 dcur = P.weighted[0][i];
    f4 scur = P.channels == 6 ? P.weighted[1][i] : P.noisy_cur[1][i];
    if (bits) {
        int tx, ty; float qx, qy;
        tap_position(P.motion[i], P.w, P.h, tx, ty, qx, qy);
        float cw[4];
        const float sum_w = tap_weights(qx, qy, bits, cw);
        if (sum_w > 1e-5f) {
            const f4 dprev = blend_taps(P.filt_prev[0], P, tx, ty, z, bits, cw);
            if (sum_w > 0.001f && !(isnan(dprev.x) || isnan(dprev.y) || isnan(dprev.z) || isnan(dprev.w))) {
                const float alpha = clampf(1.0f / dprev.w, 0.01f, 1.0f);
                dcur = F4(mix3(F3(dprev), F3(dcur), alpha), fmin2(dprev.w + 1.0f, 255.0f));
                if (P.channels == 6) {
                    const f4 sprev = blend_taps(P.filt_prev[1], P, tx, ty, z, bits, cw);
                    scur = F4(mix3(F3(sprev), F3(scur), alpha), scur.w);
                }
            }
        }
    }
    dcur = F4(nan_to_zero(dcur.x), nan_to_zero(dcur.y), nan_to_zero(dcur.z), dcur.w);
    scur = F4(nan_to_zero(scur.x), nan_to_zero(scur.y), nan_to_zero(scur.z), scur.w);
    const bool nosurf = (accepts & 16u) != 0;
    if (!nosurf) {
        const f4 alb = P.albedo[i];
        P.color[i] = F4(alb.x * dcur.x + scur.x, alb.y * dcur.y + scur.y, alb.z * dcur.z + scur.z, 1.0f);
    }
    P.filt_cur[0][i] = dcur;
    if (P.channels == 6) P.filt_cur[1][i] = scur;
    P.normal_cur[i] = P.normal[i];
    const f4 pp = P.pos[i];
    P.pos_cur[i] = F4(pp.x, pp.y, pp.z, nosurf ? 1.0f : 0.0f);
}

template <bool PREPARED>
void launch_fit(int channels, uint blocks, const float* rows, float* weights, float* minmax, int bw, int bh, uint frame, float noise, hipStream_t st) {
    if (channels == 3) hipLaunchKernelGGL((k_bmfr_fit<13, PREPARED>), dim3(blocks), dim3(256), 0, st, rows, weights, minmax, bw, bh, frame, noise);
    else hipLaunchKernelGGL((k_bmfr_fit<16, PREPARED>), dim3(blocks), dim3(256), 0, st, rows, weights, minmax, bw, bh, frame, noise);
}

}  // namespace
}  // namespace tr

using namespace tr;

struct trhip_bmfr : StageHost<5> {      // an event before the frame and one behind each of the four passes
    int settings = 0, channels = 3;
    float noise = 1e-2f;
    uint32_t w = 0, h = 0, layers = 0, bw = 0, bh = 0;
    int cur = 0;                     // the histories a frame reads; it writes cur ^ 1
    bool have_history = false;
    f4* noisy[2][2] = {};
    f4* filt[2][2] = {};
    f2* normal[2] = {};
    f4* pos[2] = {};
    f4* weighted[2] = {};
    float *rows = nullptr, *weights = nullptr, *minmax = nullptr;
    uint8_t* accept = nullptr;
    size_t pixels() const { return (size_t)w * h * layers; }
    size_t blocks() const { return (size_t)bw * bh * layers; }
};

extern "C" {

int trhip_bmfr_create(trhip_device* dev, const trhip_bmfr_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_bmfr** out) {
    if (!out) return set_error("trhip_bmfr_create: null out");
    *out = nullptr;
    if (!opt) return set_error("trhip_bmfr_create: null options");
    if (opt->settings != TRHIP_BMFR_DIFFUSE_ONLY && opt->settings != TRHIP_BMFR_DIFFUSE_SPECULAR)
        return set_error("trhip_bmfr_create: settings must be TRHIP_BMFR_DIFFUSE_ONLY (0) or TRHIP_BMFR_DIFFUSE_SPECULAR (1)");
    if (!(opt->noise_amount >= 0.0f) || !(opt->noise_amount < 1.0f)) return set_error("trhip_bmfr_create: noise_amount must be in [0, 1) (0 = 1e-2)");
    if (width == 0 || height == 0 || layers == 0) return set_error("trhip_bmfr_create: zero width, height or layer count");
    if (width > 16384 || height > 16384 || layers > 4096) return set_error("trhip_bmfr_create: image too large");
    if (!dev) return set_error("trhip_bmfr_create: null trhip_device (no HIP device: there is no CPU fallback)");
    DEVCHK(device_index(dev));
    trhip_bmfr* b = new trhip_bmfr;
    b->hip_device = device_index(dev);
    b->settings = opt->settings;
    b->channels = opt->settings == TRHIP_BMFR_DIFFUSE_ONLY ? 3 : 6;
    b->noise = opt->noise_amount == 0.0f ? 1e-2f : opt->noise_amount;
    b->w = width; b->h = height; b->layers = layers;
    b->bw = (width + 31) / 32 + 1; b->bh = (height + 31) / 32 + 1;
    const size_t px = b->pixels(), nb = b->blocks();
    auto alloc = [&](auto*& p, size_t bytes) { b->alloc_zeroed(p, bytes); };
    for (int i = 0; i < 2; ++i) {
        alloc(b->noisy[i][0], px * sizeof(f4)); alloc(b->noisy[i][1], px * sizeof(f4));
        alloc(b->filt[i][0], px * sizeof(f4));
        if (b->channels == 6) alloc(b->filt[i][1], px * sizeof(f4));
        alloc(b->normal[i], px * sizeof(f2)); alloc(b->pos[i], px * sizeof(f4));
    }
    alloc(b->weighted[0], px * sizeof(f4));
    if (b->channels == 6) alloc(b->weighted[1], px * sizeof(f4));
    alloc(b->rows, nb * (BMFR_FEATURES + b->channels) * BMFR_BLOCK_PIXELS * sizeof(float));
    alloc(b->weights, nb * b->channels * BMFR_FEATURES * sizeof(float));
    alloc(b->minmax, nb * 12 * sizeof(float));
    alloc(b->accept, px);
    return stage_finish_create("trhip_bmfr_create", b, out);
}

void trhip_bmfr_destroy(trhip_bmfr* b) { stage_destroy(b); }

int trhip_bmfr_reset_history(trhip_bmfr* b) {
    if (!b) return set_error("trhip_bmfr_reset_history: null stage");
    b->have_history = false;
    return 0;
}

int trhip_bmfr_run(trhip_bmfr* b, const trhip_bmfr_features* f, uint32_t frame_counter, void* stream) {
    if (!b) return set_error("trhip_bmfr_run: null stage");
    if (!f) return set_error("trhip_bmfr_run: null features");
    if (!f->color || !f->diffuse || !f->albedo || !f->normal || !f->pos || !f->screen_motion)
        return set_error("trhip_bmfr_run: color, diffuse, albedo, normal, pos and screen_motion are required (only instance_id may be null)");
    DEVCHK(b->hip_device);
    hipStream_t st = (hipStream_t)stream;
    BmfrParams P{};
    P.w = (int)b->w; P.h = (int)b->h; P.layers = (int)b->layers; P.bw = (int)b->bw; P.bh = (int)b->bh;
    P.channels = b->channels; P.nc = BMFR_FEATURES + b->channels;
    int32_t ox, oy;
    bmfr_block_offset(frame_counter % BMFR_OFFSETS, ox, oy);
    P.shift_x = -16 + ox; P.shift_y = -16 + oy;
    P.frame = frame_counter; P.have_history = b->have_history ? 1 : 0; P.noise = b->noise;
    P.color = (f4*)f->color; P.diffuse = (const f4*)f->diffuse; P.albedo = (const f4*)f->albedo; P.pos = (const f4*)f->pos;
    P.normal = (const f2*)f->normal; P.motion = (const f2*)f->screen_motion; P.instance_id = (const int*)f->instance_id;
    const int c = b->cur, nx = c ^ 1;
    for (int k = 0; k < 2; ++k) {
        P.noisy_prev[k] = b->noisy[c][k]; P.noisy_cur[k] = b->noisy[nx][k];
        P.filt_prev[k] = b->filt[c][k]; P.filt_cur[k] = b->filt[nx][k];
        P.weighted[k] = b->weighted[k];
    }
    P.normal_prev = b->normal[c]; P.normal_cur = b->normal[nx];
    P.pos_prev = b->pos[c]; P.pos_cur = b->pos[nx];
    P.rows = b->rows; P.weights = b->weights; P.minmax = b->minmax; P.accept = b->accept;

    const uint pixel_groups = (uint)((b->pixels() + 255) / 256);
    HIPCHK(hipEventRecord(b->ev[0], st));
    hipLaunchKernelGGL(k_bmfr_preprocess, dim3(b->bw, b->bh * 4, b->layers), dim3(256), 0, st, P);
    HIPCHK(hipEventRecord(b->ev[1], st));
    launch_fit<false>(b->channels, (uint)b->blocks(), b->rows, b->weights, b->minmax, P.bw, P.bh, frame_counter, b->noise, st);
    HIPCHK(hipEventRecord(b->ev[2], st));
    hipLaunchKernelGGL(k_bmfr_weighted_sum, dim3(pixel_groups), dim3(256), 0, st, P);
    HIPCHK(hipEventRecord(b->ev[3], st));
    hipLaunchKernelGGL(k_bmfr_accumulate_output, dim3(pixel_groups), dim3(256), 0, st, P);
    HIPCHK(hipEventRecord(b->ev[4], st));
    HIPCHK(hipGetLastError());
    b->cur = nx;
    b->have_history = true;
    b->frames += 1;
    return 0;
}

int trhip_bmfr_get_timings(trhip_bmfr* b, trhip_bmfr_timings* out) {
    if (int r = stage_total_ms("trhip_bmfr_get_timings", b, out)) return r;
    if (b->frames == 0) return 0;
    float* dst[4] = {&out->preprocess_ms, &out->fit_ms, &out->weighted_sum_ms, &out->accumulate_output_ms};
    for (int i = 0; i < 4; ++i) HIPCHK(hipEventElapsedTime(dst[i], b->ev[i], b->ev[i + 1]));
    return 0;
}

int trhip_bmfr_fit_blocks(trhip_device* dev, uint32_t blocks, uint32_t channels, const float* matrix_dev, float* weights_dev, void* stream) {
    if (!dev) return set_error("trhip_bmfr_fit_blocks: null trhip_device");
    if (channels != 3 && channels != 6) return set_error("trhip_bmfr_fit_blocks: channels must be 3 or 6");
    if (blocks == 0) return 0;
    if (!matrix_dev || !weights_dev) return set_error("trhip_bmfr_fit_blocks: null matrix or weights");
    DEVCHK(device_index(dev));
    launch_fit<true>((int)channels, blocks, matrix_dev, weights_dev, nullptr, 1, 1, 0, 0.0f, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int trhip_bmfr_download(trhip_bmfr* b, int which, void* host, size_t bytes) {
    if (!b || !host) return set_error("trhip_bmfr_download: null argument");
    if (which == TRHIP_BMFR_BLOCK_OFFSETS) {
        int32_t table[BMFR_OFFSETS][2];
        for (uint32_t i = 0; i < BMFR_OFFSETS; ++i) bmfr_block_offset(i, table[i][0], table[i][1]);
        if (bytes != sizeof(table)) return set_error("trhip_bmfr_download: the block offsets are 16 x 2 int32");
        memcpy(host, table, sizeof(table));
        return 0;
    }
    return stage_download("trhip_bmfr_download", b, host, bytes, [&](const void*& src, size_t& size) {
        const size_t px = b->pixels(), nb = b->blocks();
        const int c = b->cur;      // what the last frame wrote
        switch (which) {
            case TRHIP_BMFR_NOISY_DIFFUSE: src = b->noisy[c][0]; size = px * sizeof(f4); break;
            case TRHIP_BMFR_NOISY_SPECULAR: src = b->noisy[c][1]; size = px * sizeof(f4); break;
            case TRHIP_BMFR_FILTERED_DIFFUSE: src = b->filt[c][0]; size = px * sizeof(f4); break;
            case TRHIP_BMFR_FILTERED_SPECULAR: src = b->filt[c][1]; size = px * sizeof(f4); break;
            case TRHIP_BMFR_FEATURE_ROWS: src = b->rows; size = nb * (BMFR_FEATURES + b->channels) * BMFR_BLOCK_PIXELS * sizeof(float); break;
            case TRHIP_BMFR_WEIGHTS: src = b->weights; size = nb * b->channels * BMFR_FEATURES * sizeof(float); break;
            case TRHIP_BMFR_MIN_MAX: src = b->minmax; size = nb * 12 * sizeof(float); break;
            case TRHIP_BMFR_ACCEPT_BITS: src = b->accept; size = px; break;
            case TRHIP_BMFR_PREVIOUS_NORMAL: src = b->normal[c]; size = px * sizeof(f2); break;
            case TRHIP_BMFR_PREVIOUS_POS: src = b->pos[c]; size = px * sizeof(f4); break;
            default: return set_error("trhip_bmfr_download: unknown buffer");
        }
        if (!src) return set_error("trhip_bmfr_download: the stage has no such buffer (the filtered specular history exists under DIFFUSE_SPECULAR)");
        return 0;
    });
}

}  // extern "C"
