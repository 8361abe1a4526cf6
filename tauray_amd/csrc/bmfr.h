// bmfr_stage (src/bmfr_stage.{hh,cc}, shader/bmfr_*.comp): blockwise multi-order feature regression between the path tracer and the
// tonemap stage.  Constants and buffer layouts shared by the kernels of bmfr.hip and the entry points trhip_bmfr_* (include/trhip.h).
//
// Layouts (all fp32; w x h pixels, L layers, bw = ceil(w/32)+1, bh = ceil(h/32)+1 blocks per layer, nb = bw*bh*L, C = 3 or 6 channels):
//   feature rows  [nb][10 + C][1024]  column-major per block, row = y_in_block*32 + x_in_block: the ten features unscaled and without
//                                     noise, then the accumulated noisy channels; a "no surface" row is all zero, so column 0 (the
//                                     constant feature) doubles as the row's surface flag
//   weights       [nb][C][10]         min / max [nb][6][2] (features 4-9)         accept bits u8 [L][h][w] (bits 0-3 taps, bit 4 no surface)
//   histories     RGBA32F [L][h][w], two of each (ping-pong: a frame reads index cur and writes cur ^ 1)
#pragma once
#include <string>

#include "common.h"

namespace tr {

constexpr int BMFR_BLOCK_EDGE = 32;
constexpr int BMFR_BLOCK_PIXELS = BMFR_BLOCK_EDGE * BMFR_BLOCK_EDGE;
constexpr int BMFR_FEATURES = 10;
constexpr int BMFR_OFFSETS = 16;

// The 16 block-grid offsets of this stage (not the reference's table): Halton points in bases 2 and 3, index i = 0..15, as even
// numbers of [-16, 16).  Integer arithmetic, so every host computes the same table.
inline void bmfr_block_offset(uint32_t i, int32_t& ox, int32_t& oy) {
    i &= 15u;
    uint32_t rev = ((i & 1u) << 3) | ((i & 2u) << 1) | ((i & 4u) >> 1) | ((i & 8u) >> 3);      // radical inverse base 2, 4 digits
    uint32_t num = (i % 3u) * 9u + ((i / 3u) % 3u) * 3u + ((i / 9u) % 3u);                     // radical inverse base 3, 3 digits, / 27
    ox = 2 * (int32_t)rev - 16;
    oy = 2 * (int32_t)(num * 16u / 27u) - 16;
}

}  // namespace tr
