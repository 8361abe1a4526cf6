// looking_glass_composition_stage (src/looking_glass_composition_stage.{hh,cc}, shader/looking_glass_composition.comp restated): constants and
// the pinned order of operations of k_looking_glass (looking_glass.hip) behind the entry points trhip_lkg_* (include/trhip.h).
// tests/looking_glass_model.py repeats this file in float32, as the TAA model repeats taa.h.
//
// Layouts: src RGBA32F [views][view_h][view_w] (display space), dst RGBA32F [out_h][out_w], dst_rgba8 uint8 [out_h][out_w][4], view indices
// uint8 [out_h][out_w][4] (the view of r, g, b; 0).
//
// Order of operations (plain fp32; every product, sum and quotient is rounded on its own: the build has contraction off and the correctly
// rounded divide; N = viewport_count, (W, H) = the output size, (w, h) = the size of one view):
//   calibration  on the host, in float: cal = (pitch, tilt * pitch, pitch / (3.0f * float(W)), -center); under invert every component is negated
//   uv           uv.x = (float(p.x) + 0.5f) / float(W); uv.y = (float(p.y) + 0.5f) / float(H); uvf = (uv.x, 1.0f - uv.y)
//   view         per channel c = 0, 1, 2:  d = ((uvf.x * cal.x + uvf.y * cal.y) + float(c) * cal.z) + cal.w;  hh = d - floorf(d);
//                view = clamp(int(floorf(hh * float(N))), 0, N - 1)     (hh rounds to 1 for a tiny negative d: the clamp takes it; a huge
//                finite pitch can make d infinite and hh NaN: the kernel selects view 0 then, without converting the NaN)
//   taps         at the unflipped uv (the shader flips y for the calibration and back for the fetch):
//                px = uv.x * float(w) - 0.5f; fx = floorf(px); wx = px - fx; x0 = clamp(int(fx), 0, w - 1); x1 = clamp(int(fx) + 1, 0, w - 1)
//                py, fy, wy, y0, y1 the same with uv.y and h.  T00 = (x0, y0), T10 = (x1, y0), T01 = (x0, y1), T11 = (x1, y1) of channel c of
//                view `view`
//   sum          top = T00 * (1.0f - wx) + T10 * wx;  bottom = T01 * (1.0f - wx) + T11 * wx;  out[c] = top * (1.0f - wy) + bottom * wy
//                (a tap with weight 0 still takes part: a NaN or an infinity in it reaches the sum)
//   alpha        out[3] = 1
//   rgba8        per channel: cc = c > 0 ? (c < 1 ? c : 1) : 0 (a NaN gives 0); uint8(cc * 255.0f + 0.5f) truncated; alpha 255
#pragma once
#include <string>

#include "common.h"

namespace tr {

constexpr int LKG_WAVE = 64;                     // a wave is 64 consecutive x of one output row ...
constexpr int LKG_ROWS = 4;                      // ... and a workgroup four such rows
constexpr uint32_t LKG_MAX_VIEWS = 255;          // a view index is one byte
constexpr uint32_t LKG_MAX_EXTENT = 16384;

}  // namespace tr
