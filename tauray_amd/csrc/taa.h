// taa_stage (src/taa_stage.{hh,cc}, shader/taa.comp restated): constants, the decision byte and the pinned order of operations of k_taa
// (taa.hip) behind the entry points trhip_taa_* (include/trhip.h).  tests/taa_model.py repeats this file in float32, as the reprojection
// model repeats taps.h.
//
// Layouts (all fp32; [layers][h][w]): src / dst / history RGBA32F, screen_motion RG32F (uv, y up), pos RGBA32F, instance id R32I,
// decisions one byte per pixel.
//
// Order of operations (every product and sum is rounded on its own: the build has contraction off; dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z
// from the left; mix(a, b, t) = a*(1 - t) + b*t):
//   functions  exp2, log2, log and exp below are float32 functions of a float32 argument, rounded once from double (the kernel evaluates them
//              at double: within half an ulp but for rare double-rounding cases; the device library's float versions are good to one or two ulps)
//   map(c)     per channel: c <= 0 ? 0 : exp2(gamma * log2(c)); under anti_shimmer then c > 1e-5 ? log(c) : -10
//   unmap(c)   under anti_shimmer first exp(c); then c <= 0 ? 0 : exp2(inv_gamma * log2(c)), inv_gamma = 1.0f / gamma
//   ranges     lo[a] = min over the window of dot(m, axis[a]) - 1e-5, hi[a] = max of dot(m, axis[a]) + 1e-5; window x outer, y inner; a
//              neighbour outside the image contributes the clamped-to-edge texel, which is in the window already
//   depth      dot(pos - cam.origin, forward), forward = -view_inverse[2].xyz; +inf for a pixel outside the image or without a surface;
//              the search starts from (+inf, offset 0) and takes a neighbour under a strict <, x outer, y inner.  The depth is this float32
//              value by definition (the reference compares the float32 content of a depth target): on a wall that faces the camera the
//              depths of a window differ by rounding only, so the model compares the same float32 values whatever it evaluates colours at
//   miss       (perspective only) t = proj_inverse * (u, v, 1, 1) with (u, v) = ((x + 0.5) / w, (h - (y + 0.5)) / h) * 2 - 1;
//              dir = normalize(view_inverse * (t.xyz, 0)); c = previous.view_proj * (dir, 0); motion = (c.xy / c.w) * 0.5 + 0.5
//              (a matrix times a vector is col0*x + col1*y + col2*z + col3*w from the left)
//   unjitter   motion = motion + (previous.pan.zw - current.pan.zw) * 0.5
//   uv         (motion.x, 1 - motion.y) - offset * pixel_size, pixel_size = 1.0f / size
//   outside    !(uv.x >= 0) || !(uv.y >= 0) || uv.x > 1 + 2 * pixel_size.x || uv.y > 1 + 2 * pixel_size.y   (a NaN is outside)
//   bicubic    pos = uv * size; c = floor(pos - 0.5); f = pos - (c + 0.5); f2 = f*f; f3 = f*f2
//              w0 = (-0.5*f3 + f2) - 0.5*f;  w1 = (1.5*f3 - 2.5*f2) + 1;  w2 = (-1.5*f3 + 2*f2) + 0.5*f;  w3 = 0.5*f3 - 0.5*f2
//              w12 = w1 + w2; q = w2 / w12 (per axis).  With T(i, j) the clamped-to-edge texel (c.x + i, c.y + j):
//              A = mix(T(0,-1), T(1,-1), q.x); B = mix(T(-1,0), T(-1,1), q.y); C = mix(mix(T(0,0), T(1,0), q.x), mix(T(0,1), T(1,1), q.x), q.y)
//              D = mix(T(2,0), T(2,1), q.y);   E = mix(T(0,2), T(1,2), q.x)
//              wa = w12.x*w0.y; wb = w0.x*w12.y; wc = w12.x*w12.y; wd = w3.x*w12.y; we = w12.x*w3.y
//              prev = max(((((A*wa + B*wb) + C*wc) + D*wd) + E*we) / ((((wa + wb) + wc) + wd) + we), 0)
//   clip       delta = map(prev) - m; per axis in table order: inv = 1 / dot(delta, axis); pp = dot(m, axis); t0 = (lo - pp) * inv;
//              t1 = (hi - pp) * inv; near = fmaxf(near, fminf(t0, t1)); far = fminf(far, fmaxf(t0, t1)), from near = -1e9, far = 1e9.
//              fminf / fmaxf return the other operand when one is NaN (0 * inf where the 1e-5 dilation is absorbed by a large colour):
//              an axis whose t0 / t1 is NaN does not constrain the result.  t = (near <= far && (near > 0 || far > 0)) ? (near > 0 ? near
//              : far) : -1; len = clamp(t, 0, 1); clipped = m + len * delta
//   blend      out.rgb = unmap(mix(clipped, m, alpha)); out.a = src.a; alpha = 1 while the stage has no history
#pragma once
#include <string>

#include "common.h"

namespace tr {

constexpr int TAA_TILE = 16;                     // a workgroup is a 16 x 16 tile of one layer ...
constexpr int TAA_HALO = TAA_TILE + 2;           // ... and stages the 18 x 18 pixels its windows touch
constexpr float TAA_KDOP_DILATION = 0.00001f;
constexpr int TAA_AXES = 11;
constexpr int TAA_DECISION_OUTSIDE = 1 << 4;     // reprojected outside the history: the frame's colour passes through
constexpr int TAA_DECISION_NO_SURFACE = 1 << 5;  // the pixel the motion was taken from has no surface

// the 22-DOP of shader/taa.comp:46-56
#define TAA_AXIS_TABLE \
    {1.000000f, 0.000000f, 0.000000f}, {-0.098489f, 0.184576f, -0.977871f}, {0.752374f, -0.312087f, 0.580116f}, {-0.098489f, -0.969577f, -0.224098f}, \
    {0.330653f, 0.717910f, -0.612596f}, {0.752374f, 0.656636f, -0.052553f}, {0.591354f, 0.440953f, 0.675174f}, {0.698983f, -0.670755f, -0.248014f}, \
    {0.176950f, -0.538181f, -0.824045f}, {-0.698983f, -0.042551f, 0.713871f}, {0.330652f, -0.849517f, 0.411084f}

}  // namespace tr
