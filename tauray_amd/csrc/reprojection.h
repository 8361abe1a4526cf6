// spatial_reprojection_stage / temporal_reprojection_stage (src/spatial_reprojection_stage.{hh,cc}, src/temporal_reprojection_stage.{hh,cc})
// and the first-hit G-buffer pass that feeds the spatial stage: constants and the decision record shared by the kernels of
// reprojection.hip and the entry points trhip_gbuffer_render, trhip_spatial_reprojection_*, trhip_temporal_reprojection_* (include/trhip.h).
//
// Layouts (all fp32; w x h pixels):
//   source images       colour RGBA32F, normal RG32F (octahedral), pos RGBA32F, instance id R32I: [sources][h][w], in the order of the list
//   destination images  normal, pos, instance id: [total - sources][h][w], the viewports that are not sources in ascending order
//   output colour       RGBA32F [total][h][w], natural viewport order
//   decision record     8 bytes per destination (spatial) or per pixel (temporal): u8 kind, u8 source slot, u8 keep bits (tl, tr, bl, br),
//                       u8 zero, i16 tap origin x, i16 tap origin y
#pragma once
#include <string>

#include "common.h"

struct trhip_device;

namespace tr {

uint* device_overflow_flag(trhip_device* dev);         // api.hip: the traversal-stack overflow flag of a handle

constexpr int REPROJ_NONE = 0;           // nothing accepted: default_value (spatial) / colour unchanged (temporal)
constexpr int REPROJ_REPROJECTED = 1;    // blended from the kept taps of `slot`
constexpr int REPROJ_SKY_COPY = 2;       // no surface: the same pixel of source `slot`, which has no surface there either
constexpr float REPROJ_NORMAL_COS = 0.99f;       // a tap is kept when dot(n_tap, n) > this ...
constexpr float REPROJ_DISTANCE_SQ = 0.01f;      // ... and |pos - pos_tap|^2 < this (0.1 world units)
constexpr float REPROJ_MIN_WEIGHT = 1e-5f;       // a try succeeds when the kept bilinear weight exceeds this
constexpr int REPROJ_MAX_SOURCES = 255;          // the record's slot is a byte
constexpr int REPROJ_TILE = 16;                  // a workgroup is a 16 x 16 tile of one layer

struct ReprojRecord { uint8_t kind, slot, bits, zero; int16_t ox, oy; };

}  // namespace tr
