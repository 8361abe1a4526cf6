// glTF morph targets (glTF 2.0 section 3.7.2.2; no counterpart in the reference, whose loader skips them, src/gltf.cc:623): the record of
// the active list and the pinned order of operations of k_morph (bvh_build.hip, next to k_skinning) behind trhip_scene_set_morph_targets /
// trhip_scene_morph (include/trhip.h).  tests/morph_model.py repeats this file in float32, as the TAA model repeats taa.h.
//
// Layouts (all fp32): base and destination are 48-byte vertices (common.h Vertex); the deltas are stored target-major in up to three planes,
// dpos / dnrm / dtan = float[target_count][vertex_count][3], so that the lanes of a wave read consecutive addresses of one target's plane;
// the active list is MorphActive[active_count], ascending in `index`.
//
// Order of operations for vertex i (every product and every sum is rounded on its own: the build has contraction off, no fma):
//   active    the targets k with w[k] != 0, ascending k, compacted by the host into (index, weight); every lane walks the same list, so the
//             trip count is uniform.  With an empty list the vertex is the base vertex, copied verbatim (no arithmetic, -0 stays -0)
//   position  acc = base.pos; for each active k in order: acc.c = acc.c + w[k] * dpos[k][i].c, per component c = x, y, z
//   normal    with a normal plane: acc = base.normal, the same accumulation over dnrm; d = (acc.x*acc.x + acc.y*acc.y) + acc.z*acc.z;
//             len = sqrt(d) (correctly rounded); normal = len > 0 ? (acc.x / len, acc.y / len, acc.z / len) (correctly rounded division)
//             : base.normal.  (len > 0 is false for a NaN: the base normal is kept.)  Without a normal plane the base normal is kept as it is
//   tangent   with a tangent plane: tangent.xyz as the normal over dtan from base.tangent.xyz (a zero-length result keeps base.tangent.xyz);
//             tangent.w is kept.  Without a tangent plane the base tangent is kept
//   uv        kept.  TEXCOORD_n and COLOR_n targets are not read (a vertex here has no colour, and no file this project meets morphs uvs)
//
// Order with skinning: glTF morphs first and skins second.  On an instance that has a skin slot the destination is the slot's `source`
// (the scene's vertices change at the next trhip_scene_skin); on any other instance it is the instance's vertex span in the scene, which
// is what k_skinning writes.
#pragma once
#include "common.h"

namespace tr {

struct MorphActive { uint index; float weight; };      // one active target: its plane index and w[index] != 0

}  // namespace tr
