// The first hit of a pixel of a listed viewport: the front half that k_feature (api.hip), k_gbuffer (reprojection.hip), k_dshgi_indirect
// (dshgi.hip), k_restir_di_canonical (restir_di.hip) and k_restir_gi_initial (restir_gi.hip) share, and the launch shape of the four that
// take a viewport list.  The five kernels call first_hit and first_hit_surface below and are built with the same flags (Makefile), so
// what one of them finds and shades at a pixel is what the others do: k_feature's images are the reference k_gbuffer, k_dshgi_indirect
// and k_restir_di_canonical are tested against bit for bit, and k_restir_gi_initial's surface record is tested against
// k_restir_di_canonical's.
//   device  tile_pixel, ViewportList, first_hit, first_hit_surface
//   host    whole_image_launch, tile_grid (they need LaunchCtx and dim3; the rest of a viewport frame's host side is in stage_host.h)
#pragma once
#include "reprojection.h"
#include "shading.h"
#include "trace.h"

namespace tr {

static_assert(REPROJ_TILE * REPROJ_TILE == TR_BLOCK, "a workgroup is one tile");

constexpr int VIEWPORT_CHUNK = 64;     // viewports of one launch: the list travels in the kernel arguments
struct ViewportList { uint v[VIEWPORT_CHUNK]; };

// Pixel of a thread: a workgroup is a 16 x 16 tile of layer blockIdx.z, a wave an 8 x 8 quarter of it (coherent primary rays, shared tap
// and texel lines).
TR_DEV void tile_pixel(int& x, int& y) {
    const uint t = threadIdx.x, wave = t >> 6, k = t & 63u;
    x = (int)(blockIdx.x * REPROJ_TILE + ((wave & 1u) << 3) + (k & 7u));
    y = (int)(blockIdx.y * REPROJ_TILE + ((wave >> 1) << 3) + (k >> 3));
}

// The camera ray through the centre of pixel (px, py) of `cam` and its closest hit (shader/rt_feature.rgen:21-45).  `stack`: the lane's
// column of the workgroup's LDS stack rows.  hit.instance_id < 0: a miss; overflow != 0: the traversal stack overflowed, the caller raises
// the device's flag.
template <bool TWO_LEVEL>
TR_DEV void first_hit(const SceneView& sv, const LaunchCtx& L, const CameraData& cam, int projection, int px, int py, float min_ray_dist, int* stack,
                      f3& ray_origin, f3& dir, HitRecord& hit, int& overflow) {
    f3 origin;
    get_screen_camera_ray(L, px, py, cam, projection, false, F2(0), F2(0.5f), origin, dir);
    ray_origin = projection == 2 ? origin : F3(cam.origin);   // rt_feature.rgen:35 traces from cam.origin
    TraceStats st = {};
    overflow = 0;
    trace_closest4<1, false, TWO_LEVEL>(sv, ray_origin, dir, min_ray_dist, __builtin_huge_valf(), 0u, stack, hit, st, overflow);
}

// The surface and material at a hit of first_hit (rt_feature.rchit:16-27).
TR_DEV void first_hit_surface(const SceneView& sv, const HitRecord& hit, f3 dir, f3 ray_origin, SurfacePoint& v, SampledMaterial& mat) {
    shade_surface(sv, hit.instance_id, hit.primitive_id, hit.u, hit.v, dir, ray_origin, false, 0, false, v, mat);
}

// A duplicate distribution of the whole image: what trhip_feature_render launches for it.
inline LaunchCtx whole_image_launch(uint w, uint h) {
    LaunchCtx L{};
    L.size_x = w; L.size_y = h; L.strategy = 0; L.index = 0; L.count = 1; L.primary = 1; L.launch_w = w; L.launch_h = h;
    return L;
}

inline dim3 tile_grid(uint w, uint h, uint layers) { return dim3((w + REPROJ_TILE - 1) / REPROJ_TILE, (h + REPROJ_TILE - 1) / REPROJ_TILE, layers); }

}  // namespace tr
