"""Host-side mirror of the reference's renderer/stage surface for the path-tracer hot path,
driving the HIP kernels through the C ABI (include/trhip.h).

Reference classes mirrored (same names, argument meaning and error behaviour; errors surface as
TrhipError where the reference throws std::runtime_error):

* ``Context``            - tr::context / tr::device pair for ONE device (src/context.hh, src/device.hh)
* ``SceneStage``         - scene_stage uploads + acceleration structure (src/scene_stage.cc)
* ``PathTracerStage``    - path_tracer_stage / rt_camera_stage / rt_stage (src/path_tracer_stage.{hh,cc})
* ``FeatureStage``       - feature_stage (src/feature_stage.{hh,cc})
* ``StitchStage``        - stitch_stage (src/stitch_stage.{hh,cc})
* ``TonemapStage``       - tonemap_stage (src/tonemap_stage.{hh,cc})
* ``ShPathTracerStage`` / ``ShRenderer`` - sh_path_tracer_stage + sh_compact_stage, sh_renderer (src/sh_path_tracer_stage.{hh,cc},
                           src/sh_renderer.{hh,cc}): the probe grids of a scene baked as spherical harmonics
* ``DshgiStage`` / ``DshgiRenderer`` - dshgi_renderer (src/dshgi_renderer.{hh,cc}, shader/forward.frag): direct light plus the indirect
                           light looked up in the baked grids
* ``RtRenderer``         - rt_renderer<path_tracer_stage> (src/rt_renderer.{hh,cc}); one process per GPU,
                           partial frames gathered with torch.distributed (RCCL) instead of host-bounce copies
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import (AccelInfoC, AccelLayoutC, CountersC, DistributionC, LightAccelInfoC, LightCountersC, PtOptionsC, TerminalCountersC, SceneDescC, TimingsC,
                   TonemapInfoC, TrhipError, check)
from .distribution import (DISTRIBUTION_DUPLICATE, DISTRIBUTION_SCANLINE, DISTRIBUTION_SHUFFLED_STRIPS, DistributionParams,
                           get_device_distribution_params, get_distribution_target_size)
from .scene import SceneDesc, ShGrid, build_alias_table

# film_filter, multiple_importance_sampling_mode, bounce_sampling_mode, tri_light_sampling_mode (src/rt_common.hh)
FILM_POINT, FILM_BOX, FILM_BLACKMAN_HARRIS = 0, 1, 2
MIS_DISABLED, MIS_BALANCE_HEURISTIC, MIS_POWER_HEURISTIC = 0, 1, 2
BOUNCE_HEMISPHERE, BOUNCE_COSINE_HEMISPHERE, BOUNCE_MATERIAL = 0, 1, 2
TRI_LIGHT_AREA, TRI_LIGHT_SOLID_ANGLE, TRI_LIGHT_HYBRID = 0, 1, 2
SAMPLER_UNIFORM_RANDOM, SAMPLER_SOBOL_OWEN, SAMPLER_SOBOL_Z_ORDER_2D, SAMPLER_SOBOL_Z_ORDER_3D = 0, 1, 2, 3
TONEMAP_LINEAR, TONEMAP_GAMMA_CORRECTION, TONEMAP_FILMIC, TONEMAP_REINHARD, TONEMAP_REINHARD_LUMINANCE = 0, 1, 2, 3, 4
FEATURE_ALBEDO, FEATURE_WORLD_NORMAL, FEATURE_VIEW_NORMAL, FEATURE_WORLD_POS, FEATURE_VIEW_POS, FEATURE_DISTANCE = 0, 1, 2, 3, 4, 5
FEATURE_INSTANCE_ID = 9


def make_options(**kw) -> PtOptionsC:
    """path_tracer_stage::options at the reference's CLI defaults (src/options.hh)."""
    o = PtOptionsC(max_bounces=8, min_ray_dist=1e-4, rng_seed=0, sampler=SAMPLER_UNIFORM_RANDOM, samples_per_pixel=1,
                   samples_per_pass=1, projection=0, film=FILM_POINT, film_radius=0.5, mis_mode=MIS_POWER_HEURISTIC,
                   russian_roulette_delta=0.0, indirect_clamping=0.0, regularization_gamma=0.0, depth_of_field=0,
                   nee_point=1.0, nee_directional=1.0, nee_envmap=1.0, nee_triangles=1.0, bounce_mode=BOUNCE_MATERIAL,
                   tri_light_mode=TRI_LIGHT_SOLID_ANGLE, hide_lights=0, use_white_albedo_on_first_bounce=0,
                   transparent_background=0, pre_transformed_vertices=0)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(f"unknown path tracer option {k!r}")
        setattr(o, k, v)
    return o


def options_for_scene(scene: SceneDesc, **kw) -> PtOptionsC:
    """create_renderer's per-scene set-up (src/tauray.cc:355-421): NEE weights are zeroed for light
    classes the scene does not have, projection follows the scene camera."""
    o = make_options(**kw)
    if len(scene.point_lights) == 0:
        o.nee_point = 0.0
    if len(scene.directional_lights) == 0:
        o.nee_directional = 0.0
    if scene.envmap is None:
        o.nee_envmap = 0.0
    if not scene.has_tri_lights():
        o.nee_triangles = 0.0
    if scene.cameras and "projection" not in kw:
        o.projection = scene.cameras[0].projection
    return o


def copy_options(o: PtOptionsC, **changes) -> PtOptionsC:
    c = PtOptionsC()
    C.memmove(C.byref(c), C.byref(o), C.sizeof(PtOptionsC))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


class DeviceBuffer:
    """gpu_buffer-like owner of one device allocation."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        check(_lib.lib().trhip_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def data_ptr(self):
        return self.ptr

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(_lib.lib().trhip_upload(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes, None))
        return self

    def download(self, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(_lib.lib().trhip_download(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes, None))
        return out

    def zero(self):
        check(_lib.lib().trhip_memset(self.ctx.h, self.ptr, 0, self.nbytes, None))
        return self

    def free(self):
        if self.ptr:
            _lib.lib().trhip_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


class Context:
    """One HIP device (the reference's context enumerates all Vulkan devices in one process; here each
    process owns one GPU and peers are reached through torch.distributed)."""

    def __init__(self, hip_device: int = 0):
        h = C.c_void_p()
        check(_lib.lib().trhip_device_create(hip_device, C.byref(h)))
        self.h = h.value
        self.hip_device = hip_device

    def alloc(self, nbytes) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def sync(self, stream=None):
        check(_lib.lib().trhip_sync(self.h, stream))

    def create_stream(self) -> int:
        st = C.c_void_p()
        check(_lib.lib().trhip_stream_create(self.h, C.byref(st)))
        return st.value

    def destroy_stream(self, stream):
        check(_lib.lib().trhip_stream_destroy(self.h, stream))

    def stream_pipe_class(self, stream=None) -> int:
        """The hardware pipe (a small integer) the queue of `stream` sits on (None = the default stream); launches that fill the chip
        overlap only between streams of different pipes (csrc/stream_pool.hip)."""
        c = C.c_int32(-1)
        check(_lib.lib().trhip_stream_pipe_class(self.h, stream, C.byref(c)))
        return c.value

    def info(self) -> dict:
        """trhip_device_get_info: which device this is (arch, PCI bus id, UUID) and how many hardware pipes the process reaches on it
        (include/trhip.h, "process requirements": 4 on MI355X with GPU_MAX_HW_QUEUES >= 8)."""
        class Info(C.Structure):
            _fields_ = [("struct_size", C.c_uint32), ("hip_device", C.c_int32), ("name", C.c_char * 64), ("pci_bus_id", C.c_char * 24),
                        ("uuid", C.c_uint8 * 16), ("compute_units", C.c_int32), ("pipe_classes", C.c_int32), ("pool_streams", C.c_int32),
                        ("hw_queues_env", C.c_int32)]
        i = Info()
        check(_lib.lib().trhip_device_get_info(self.h, C.byref(i)))
        return {"hip_device": i.hip_device, "name": i.name.decode("ascii", "replace"), "pci_bus_id": i.pci_bus_id.decode("ascii", "replace"),
                "uuid": bytes(i.uuid).hex(), "compute_units": i.compute_units, "pipe_classes": i.pipe_classes, "pool_streams": i.pool_streams,
                "hw_queues_env": i.hw_queues_env}

    def stream_wait(self, stream, on):
        """Work enqueued on `stream` from now on waits for what is on `on` now (None = the default stream)."""
        check(_lib.lib().trhip_stream_wait(self.h, stream, on))

    def calibrate_valu(self) -> float:
        """Peak vector-instruction issue rate of the device as it runs now, in 10^9 wave-level instructions per second."""
        g = C.c_float()
        check(_lib.lib().trhip_calibrate_valu(self.h, C.byref(g)))
        return float(g.value)

    def calibrate_l1(self) -> float:
        """Peak rate of cache-line accesses of the vector L1 caches of the device, in 10^9 accesses per second."""
        g = C.c_float()
        check(_lib.lib().trhip_calibrate_l1(self.h, C.byref(g)))
        return float(g.value)

    def close(self):
        if self.h:
            _lib.lib().trhip_device_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SceneStage:
    """scene_stage: uploads the flattened scene and builds the acceleration structure on the device."""

    def __init__(self, ctx: Context, scene: Optional[SceneDesc] = None, fast_trace_rebuilds: bool = False, as_strategy: int = 0,
                 dynamic=None, deformation_motion: bool = False):
        """`as_strategy`: trhip_scene_set_accel_strategy (0 all-merged, the default; 1 per-mesh; 2 static-merged-dynamic-per-mesh).
        `dynamic`: per-instance marks (trhip_scene_set_dynamic_instances) of the scenes this stage is given, or None (all static).
        `deformation_motion`: set_deformation_motion for the scenes this stage is given, and what animate() and pose() do by default."""
        self.ctx = ctx
        self.scene = None
        self.accel = None
        # the first build of a scene is a static build (tree optimisation on); rebuilds after a change are fast builds unless asked
        self.fast_trace_rebuilds = fast_trace_rebuilds
        self.as_strategy = int(as_strategy)
        self.dynamic = None if dynamic is None else np.ascontiguousarray(np.asarray(dynamic).astype(np.uint8))
        self.deformation_motion = bool(deformation_motion)
        if scene is not None:
            self.set_scene(scene)

    def set_scene(self, scene: SceneDesc):
        L = _lib.lib()
        keep = []

        def k(a):
            a = np.ascontiguousarray(a)
            keep.append(a)
            return a

        def p(a):
            return a.ctypes.data if a.size else None

        infos, texels = scene.texture_table()
        inst, spans, verts, idx = k(scene.instances), k(scene.spans), k(scene.vertices), k(scene.indices)
        pls, dls, infos, texels = k(scene.point_lights), k(scene.directional_lights), k(infos), k(texels)
        cams, non_opaque = k(scene.camera_data()), k(scene.potentially_transparent().astype(np.uint8))
        d = SceneDescC()
        d.instances, d.spans, d.instance_count = p(inst), p(spans), len(inst)
        d.vertices, d.vertex_count = p(verts), len(verts)
        d.indices, d.index_count = p(idx), len(idx)
        d.point_lights, d.point_light_count = p(pls), len(pls)
        d.directional_lights, d.directional_light_count = p(dls), len(dls)
        d.texture_infos, d.texture_count, d.texels = p(infos), len(infos), p(texels)
        if scene.envmap is not None:
            env = k(np.asarray(scene.envmap, dtype=np.float32))
            at = k(build_alias_table(env))
            d.envmap, d.envmap_width, d.envmap_height, d.alias_table = p(env), env.shape[1], env.shape[0], p(at)
        d.environment_factor = (C.c_float * 4)(*[float(x) for x in scene.environment_factor])
        d.cameras, d.camera_count = p(cams), len(cams)
        d.non_opaque = p(non_opaque)
        d.gather_emissive_triangles = 1 if getattr(scene, "tri_light_count", 0) > 0 else 0
        check(L.trhip_scene_upload(self.ctx.h, C.byref(d)))
        # the device handle keeps the switch over uploads; set behind the upload, so that a plane is never filled for the scene that leaves
        check(L.trhip_scene_set_deformation_motion(self.ctx.h, 1 if self.deformation_motion else 0))
        self.scene = scene
        self.camera_data = cams.copy()           # what the device renders with (update_cameras follows)
        self.previous_camera_data = None         # camera_pair.previous as last set (None: the cameras themselves)
        # skinned meshes: the uploaded vertices are the bind pose; pose them with the file's rest pose before the build
        # (the reference runs skinning.comp on the first scene update, src/scene_stage.cc:1543-1567)
        # morph targets come ahead of skinning (glTF 2.0 section 3.7.2.2): the skins are set first, so that a morphed and skinned mesh
        # morphs its bind pose, the file's default weights are applied, and the rest pose skins the result
        for sk in getattr(scene, "skinned", []):
            self.set_skin(sk.instance, sk.skins)
        for mm in getattr(scene, "morphed", []):
            self.set_morph_targets(mm.instance, mm.position_deltas, mm.normal_deltas, mm.tangent_deltas)
            self.morph(mm.instance, scene.morph_weights(mm), refit=None)
        for sk in getattr(scene, "skinned", []):
            self.skin(sk.instance, scene.joint_transforms(sk), refit=None)
        if self.deformation_motion:      # the plane was filled with the uploaded bind pose: a still scene has previous = current
            self.latch_positions()
        info = AccelInfoC()
        check(L.trhip_scene_set_accel_strategy(self.ctx.h, self.as_strategy))
        if self.dynamic is not None:
            if len(self.dynamic) != len(inst):
                raise ValueError(f"SceneStage: {len(self.dynamic)} dynamic marks for {len(inst)} instances")
            check(L.trhip_scene_set_dynamic_instances(self.ctx.h, self.dynamic.ctypes.data, len(self.dynamic)))
        check(L.trhip_scene_set_build_mode(self.ctx.h, 0))
        check(L.trhip_scene_build_accel(self.ctx.h, C.byref(info)))
        self.accel = dict(triangle_count=info.triangle_count, node_count=info.node_count,
                          tri_light_count=info.tri_light_count, build_ms=info.build_ms,
                          bounds_min=tuple(info.bounds_min), bounds_max=tuple(info.bounds_max),
                          node_bytes=info.node_bytes, leaf_count=info.leaf_count)
        return self.accel

    def layout(self) -> dict:
        """trhip_scene_get_accel_layout: strategy, BLAS count, TLAS leaves, BLASes the last build / refit touched, node and record bytes
        of both levels, device ms of the last BLAS work and TLAS build."""
        out = AccelLayoutC()
        check(_lib.lib().trhip_scene_get_accel_layout(self.ctx.h, C.byref(out)))
        return {name: getattr(out, name) for name, _ in AccelLayoutC._fields_}

    def set_light_accel(self, mode: int):
        """trhip_scene_set_light_accel: how closest-hit rays find sphere lights - _lib.LIGHT_ACCEL_AUTO (the default), LIGHT_ACCEL_LOOP or
        LIGHT_ACCEL_TREE.  Kept over scenes; builds or drops the light tree now.  Hits do not depend on the mode."""
        check(_lib.lib().trhip_scene_set_light_accel(self.ctx.h, int(mode)))

    def light_accel(self) -> dict:
        """trhip_scene_get_light_accel: requested mode and mode in effect, lights with a radius, lights / nodes / bytes of the tree, the
        AUTO threshold and the ms of the last tree build or refit (last_was_refit: 1 refit, 0 build, -1 none)."""
        out = LightAccelInfoC()
        check(_lib.lib().trhip_scene_get_light_accel(self.ctx.h, C.byref(out)))
        return {name: getattr(out, name) for name, _ in LightAccelInfoC._fields_}

    def update_lights(self, point_lights: np.ndarray, directional_lights: Optional[np.ndarray] = None):
        """trhip_scene_update_lights: new light records, same counts; the light tree is refit (or rebuilt) before this returns."""
        pl = np.ascontiguousarray(point_lights)
        dl = np.ascontiguousarray(self.scene.directional_lights if directional_lights is None else directional_lights)
        check(_lib.lib().trhip_scene_update_lights(self.ctx.h, pl.ctypes.data if len(pl) else None, len(pl), dl.ctypes.data if len(dl) else None, len(dl)))

    def pose(self, node_globals: dict, refit: bool = True, deformation_motion: Optional[bool] = None):
        """New global transforms of the joint nodes (an animation step of the caller's): every skinned mesh is skinned again
        and the acceleration structure updated.  `deformation_motion`: latch the positions first (latch_positions); None = as the
        switch stands."""
        if self.deformation_motion if deformation_motion is None else deformation_motion:
            self.latch_positions()
        for sk in self.scene.skinned:
            self.skin(sk.instance, self.scene.joint_transforms(sk, node_globals), refit=None)
        return self._accel_after_change(refit)

    def animate(self, animator, dt_ticks: int, refit: bool = True, deformation_motion: Optional[bool] = None):
        """One frame of a playing animation (update(scene, dt) of src/scene.cc:226-235 followed by scene_stage::update):
        `animator` (tauray_amd.animation.SceneAnimator over this stage's scene) advances by dt microseconds; the new instance
        records, cameras (with last frame's as camera_pair.previous) and joint matrices go to the device, and the acceleration
        structure is updated once - refitted, or rebuilt with `refit=False`.  With `deformation_motion` the positions of the deforming
        meshes are latched first (latch_positions; None = as the switch, set_deformation_motion, stands): latch, morph, skin, one refit."""
        instances, cameras, node_globals = animator.update(dt_ticks)
        inst = np.ascontiguousarray(instances)
        check(_lib.lib().trhip_scene_update_instances(self.ctx.h, inst.ctypes.data, len(inst)))
        if self.deformation_motion if deformation_motion is None else deformation_motion:
            self.latch_positions()
        for mm in self.scene.morphed:       # morph, then skin, then one refit
            self.morph(mm.instance, self.scene.morph_weights(mm), refit=None)
        for sk in self.scene.skinned:
            self.skin(sk.instance, self.scene.joint_transforms(sk, node_globals), refit=None)
        self.update_cameras(cameras)
        self.set_previous_cameras(animator.previous_cameras)
        pl, dl = np.ascontiguousarray(self.scene.point_lights), np.ascontiguousarray(self.scene.directional_lights)
        if len(pl) or len(dl):          # lights on moving nodes
            check(_lib.lib().trhip_scene_update_lights(self.ctx.h, pl.ctypes.data if len(pl) else None, len(pl), dl.ctypes.data if len(dl) else None, len(dl)))
        return self._accel_after_change(refit)

    def update_cameras(self, cameras):
        data = np.concatenate([c.pack() for c in cameras])
        check(_lib.lib().trhip_scene_update_cameras(self.ctx.h, data.ctypes.data, len(data)))
        self.camera_data = data

    def set_previous_cameras(self, cameras):
        """camera_pair.previous per viewport (motion features, screen-motion target)."""
        self.set_previous_camera_data(np.concatenate([c.pack() for c in cameras]))

    def set_previous_camera_data(self, data: np.ndarray):
        """The same from packed camera_data records (what `camera_data` held when an earlier frame was rendered)."""
        data = np.ascontiguousarray(data)
        check(_lib.lib().trhip_scene_set_previous_cameras(self.ctx.h, data.ctypes.data, len(data)))
        self.previous_camera_data = data.copy()

    def update_instances(self, instances: np.ndarray, refit: bool = False):
        """Dynamic scenes: new instance records (transforms / materials) for the same meshes, then a full rebuild of the
        acceleration structure on the device (what scene_stage::update + the TLAS rebuild do per frame) or, with
        `refit`, an update that keeps the tree and recomputes its boxes."""
        inst = np.ascontiguousarray(instances)
        check(_lib.lib().trhip_scene_update_instances(self.ctx.h, inst.ctypes.data, len(inst)))
        return self._accel_after_change(refit)

    def _accel_after_change(self, refit: bool):
        info = AccelInfoC()
        if refit:
            check(_lib.lib().trhip_scene_refit_accel(self.ctx.h, C.byref(info)))
        else:
            # a scene that is rebuilt after its first build is dynamic: ePreferFastBuild (src/acceleration_structure.cc:129-131)
            check(_lib.lib().trhip_scene_set_build_mode(self.ctx.h, 0 if self.fast_trace_rebuilds else 1))
            check(_lib.lib().trhip_scene_build_accel(self.ctx.h, C.byref(info)))
        self.accel.update(node_count=info.node_count, build_ms=info.build_ms, tri_light_count=info.tri_light_count,
                          bounds_min=tuple(info.bounds_min), bounds_max=tuple(info.bounds_max), leaf_count=info.leaf_count)
        return self.accel

    def set_skin(self, instance: int, skins: np.ndarray, source: Optional[np.ndarray] = None):
        """Marks the mesh of `instance` as skinned (mesh::get_animation_source + skin buffer, src/mesh.hh:32-73): `skins` is
        one SKIN record per vertex, `source` the bind-pose vertices (default: the uploaded ones)."""
        from .scene import SKIN
        skins = np.ascontiguousarray(skins, dtype=SKIN)
        src_ptr = None
        if source is not None:
            source = np.ascontiguousarray(source)
            if len(source) != len(skins):
                raise ValueError("set_skin: source and skins differ in length")
            src_ptr = source.ctypes.data
        check(_lib.lib().trhip_scene_set_skin(self.ctx.h, instance, src_ptr, skins.ctypes.data if len(skins) else None, len(skins)))

    def skin(self, instance: int, joint_transforms: np.ndarray, refit: Optional[bool] = True):
        """scene_stage::record_skinning (src/scene_stage.cc:1543-1612): shader/skinning.comp over the instance's mesh with
        the given joint matrices ((n, 4, 4), row-major as numpy writes a matrix; uploaded column-major), then the
        acceleration-structure update (`refit`), a rebuild (`refit=False`) or nothing (`refit=None`: caller batches)."""
        j = np.ascontiguousarray(np.asarray(joint_transforms, dtype=np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        check(_lib.lib().trhip_scene_skin(self.ctx.h, instance, j.ctypes.data, len(j)))
        return None if refit is None else self._accel_after_change(refit)

    def set_morph_targets(self, instance: int, position_deltas: np.ndarray, normal_deltas: Optional[np.ndarray] = None,
                          tangent_deltas: Optional[np.ndarray] = None):
        """trhip_scene_set_morph_targets: the mesh of `instance` gets the targets of the (T, V, 3) float32 delta planes (normals and tangents
        optional); their base is the instance's vertices as they stand, or the bind pose of its skin (set the skin first)."""
        planes = [None if p is None else np.ascontiguousarray(p, dtype=np.float32) for p in (position_deltas, normal_deltas, tangent_deltas)]
        if planes[0] is None or planes[0].ndim != 3 or planes[0].shape[2] != 3:
            raise ValueError("set_morph_targets: position deltas are (targets, vertices, 3)")
        for p in planes[1:]:
            if p is not None and p.shape != planes[0].shape:
                raise ValueError("set_morph_targets: the planes differ in shape")
        t, v, _ = planes[0].shape
        ptr = [None if p is None else p.ctypes.data for p in planes]
        check(_lib.lib().trhip_scene_set_morph_targets(self.ctx.h, instance, t, ptr[0], ptr[1], ptr[2], v))

    def morph(self, instance: int, weights: np.ndarray, refit: Optional[bool] = True):
        """trhip_scene_morph: base + sum of weights[k] * delta[k] (tauray_amd/csrc/morph.h) into the instance's vertices, or into its
        skin's bind pose; then the acceleration-structure update (`refit`), a rebuild (`refit=False`) or nothing (`refit=None`)."""
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        check(_lib.lib().trhip_scene_morph(self.ctx.h, instance, w.ctypes.data if len(w) else None, len(w)))
        return None if refit is None else self._accel_after_change(refit)

    def set_deformation_motion(self, on: bool):
        """trhip_scene_set_deformation_motion: with it on, the previous world position of a hit on a skinned or morphed mesh (feature
        outputs 6 to 8, the screen_motion target, the temporal reuse of ReSTIR DI) interpolates the positions latch_positions last kept,
        not the current ones.  Kept over scenes; off by default."""
        check(_lib.lib().trhip_scene_set_deformation_motion(self.ctx.h, 1 if on else 0))
        self.deformation_motion = bool(on)

    def latch_positions(self):
        """trhip_scene_latch_positions: keeps the positions of every skinned or morphed mesh as they stand, as the previous positions of the
        frame to come.  Once per frame, before morph() and skin(); nothing happens while the switch is off."""
        check(_lib.lib().trhip_scene_latch_positions(self.ctx.h))

    def previous_positions(self, instance: int) -> np.ndarray:
        """trhip_scene_get_previous_positions: the (vertices, 3) float32 previous model-space positions of the instance's mesh."""
        n = int(self.scene.spans[instance]["vertex_count"])
        out = np.zeros((n, 3), dtype=np.float32)
        check(_lib.lib().trhip_scene_get_previous_positions(self.ctx.h, instance, out.ctypes.data, n))
        return out

    def vertices(self, instance: int) -> np.ndarray:
        from .scene import VERTEX
        n = int(self.scene.spans[instance]["vertex_count"])
        out = np.zeros(n, dtype=VERTEX)
        if n:
            check(_lib.lib().trhip_scene_get_vertices(self.ctx.h, instance, out.ctypes.data, n))
        return out

    def tri_lights(self) -> np.ndarray:
        from .scene import TRI_LIGHT
        n = self.accel["tri_light_count"]
        out = np.zeros(n, dtype=TRI_LIGHT)
        if n:
            check(_lib.lib().trhip_scene_get_tri_lights(self.ctx.h, out.ctypes.data, n))
        return out

    def trace_closest(self, rays: np.ndarray, seeds: Optional[np.ndarray] = None, include_lights=False) -> np.ndarray:
        """traceRayEXT closest-hit query on explicit rays (parity hook)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        hit_dtype = np.dtype([("instance_id", "<i4"), ("primitive_id", "<i4"), ("bary_u", "<f4"), ("bary_v", "<f4"), ("t", "<f4")])
        if n == 0:
            return np.zeros(0, dtype=hit_dtype)
        d_rays = self.ctx.alloc(rays.nbytes).upload(rays)
        d_seeds = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
            d_seeds = self.ctx.alloc(seeds.nbytes).upload(seeds)
        d_hits = self.ctx.alloc(n * 20)
        check(_lib.lib().trhip_trace_closest(self.ctx.h, n, d_rays.ptr, d_seeds.ptr if d_seeds else None,
                                             1 if include_lights else 0, d_hits.ptr, None))
        return d_hits.download((n,), hit_dtype)

    def trace_terminal(self, rays: np.ndarray, seeds: Optional[np.ndarray] = None, fallback: Optional[np.ndarray] = None) -> np.ndarray:
        """trhip_trace_terminal: the terminal query on explicit rays.  Hits as trace_closest without lights, except that a blocked ray
        reports instance_id _lib.HIT_BLOCKED; fallback: nonzero = trace that ray as an ordinary closest hit."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        hit_dtype = np.dtype([("instance_id", "<i4"), ("primitive_id", "<i4"), ("bary_u", "<f4"), ("bary_v", "<f4"), ("t", "<f4")])
        if n == 0:
            return np.zeros(0, dtype=hit_dtype)
        d_rays = self.ctx.alloc(rays.nbytes).upload(rays)
        d_seeds = d_fb = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
            d_seeds = self.ctx.alloc(seeds.nbytes).upload(seeds)
        if fallback is not None:
            fallback = np.ascontiguousarray(fallback, dtype=np.uint32)
            d_fb = self.ctx.alloc(fallback.nbytes).upload(fallback)
        d_hits = self.ctx.alloc(n * 20)
        check(_lib.lib().trhip_trace_terminal(self.ctx.h, n, d_rays.ptr, d_seeds.ptr if d_seeds else None, d_fb.ptr if d_fb else None,
                                              d_hits.ptr, None))
        return d_hits.download((n,), hit_dtype)

    def trace_shadow(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        if n == 0:
            return np.zeros(0, dtype=np.float32)
        d_rays = self.ctx.alloc(rays.nbytes).upload(rays)
        d_vis = self.ctx.alloc(n * 4)
        check(_lib.lib().trhip_trace_shadow(self.ctx.h, n, d_rays.ptr, d_vis.ptr, None))
        return d_vis.download((n,), np.float32)


def _dist_c(p: DistributionParams) -> DistributionC:
    return DistributionC(int(p.size[0]), int(p.size[1]), int(p.strategy), int(p.index), int(p.count), 1 if p.primary else 0)


class PathTracerStage:
    """path_tracer_stage(device&, scene_stage&, const gbuffer_target&, const options&)."""

    _create = "trhip_pt_create"

    def __init__(self, ctx: Context, scene_stage: SceneStage, options: PtOptionsC, distribution: Optional[DistributionParams] = None):
        self.ctx, self.ss, self.opt = ctx, scene_stage, options
        h = C.c_void_p()
        check(getattr(_lib.lib(), self._create)(ctx.h, C.byref(options), C.byref(h)))
        self.h = h.value
        self.distribution = None
        if distribution is not None:
            self.reset_distribution_params(distribution)

    def reset_distribution_params(self, distribution: DistributionParams):
        d = _dist_c(distribution)
        check(_lib.lib().trhip_pt_set_distribution(self.h, C.byref(d)))
        self.distribution = distribution

    def set_shard(self, viewport_base=0, viewport_stride=1, sample_base=0, sample_stride=1):
        """View / sample sharding (trhip_pt_set_shard): local layer l = viewport base + l * stride, local sample s = sample
        base + s * stride of the pixel's sequence."""
        check(_lib.lib().trhip_pt_set_shard(self.h, viewport_base, viewport_stride, sample_base, sample_stride))

    def set_frame_counter(self, frame_counter: int):
        check(_lib.lib().trhip_pt_set_frame_counter(self.h, frame_counter))

    def set_frame_batch(self, frames: int):
        """trhip_pt_set_frame_batch: `frames` consecutive frames per run(), as frame-major layer groups of the target."""
        check(_lib.lib().trhip_pt_set_frame_batch(self.h, int(frames)))

    def set_shading_arithmetic(self, ieee: bool):
        """k_shade at IEEE fp32 with the C library's sin / cos / pow (True), or at the accuracy Vulkan asks of the reference's GLSL
        for the command-line option set (False, the default unless TRHIP_SHADE_FAST=0): include/trhip.h."""
        check(_lib.lib().trhip_pt_set_shading_arithmetic(self.h, int(bool(ieee))))

    def set_specialization(self, enable: bool):
        """A shading program compiled for this stage's option set the first time it renders (True, the default unless TRHIP_SPECIALIZE=0)
        or always the general kernels (False): include/trhip.h trhip_pt_set_specialization."""
        check(_lib.lib().trhip_pt_set_specialization(self.h, int(bool(enable))))

    def set_lanes(self, lanes: int):
        check(_lib.lib().trhip_pt_set_lanes(self.h, lanes))

    def set_fused_tonemap(self, display, info):
        """The stage's last pass writes tonemap(colour) into `display` as it writes the colour target (None: off); trhip_pt_set_fused_tonemap."""
        check(_lib.lib().trhip_pt_set_fused_tonemap(self.h, None if display is None else _ptr(display), None if info is None else C.byref(info)))

    def lane_pipes(self):
        """(lanes, [hardware pipe class of each lane's stream]) of the last render; trhip_pt_get_lane_pipes."""
        if not hasattr(_lib.lib(), "trhip_pt_get_lane_pipes"):
            return 0, []
        n = C.c_int32(0)
        cls = (C.c_int32 * 4)()
        check(_lib.lib().trhip_pt_get_lane_pipes(self.h, C.byref(n), cls))
        return n.value, [cls[i] for i in range(n.value)]

    def set_frame_slots(self, slots: int):
        """Hint: how many stages render next to this one (a renderer's frames in flight); trhip_pt_set_frame_slots."""
        if hasattr(_lib.lib(), "trhip_pt_set_frame_slots"):      # an older build named by TRHIP_LIB (A/B runs) has no such hint
            check(_lib.lib().trhip_pt_set_frame_slots(self.h, slots))

    def reset_accumulated_samples(self):
        check(_lib.lib().trhip_pt_reset_accumulation(self.h, 0))

    def reset_sample_counter(self):
        check(_lib.lib().trhip_pt_reset_accumulation(self.h, 1))

    def run(self, color_target, viewports=1, stream=None):
        """stage::run: enqueue one frame (all passes) into `color_target` (device RGBA32F)."""
        tw, th = get_distribution_target_size(self.distribution)
        check(_lib.lib().trhip_pt_render(self.h, _ptr(color_target), tw, th, viewports, stream))

    # gbuffer_target entries path_tracer.rgen can write (src/gbuffer.hh; shader/path_tracer.glsl:535-576):
    # name -> (channels, numpy dtype)
    TARGETS = {"color": (4, np.float32), "diffuse": (4, np.float32), "reflection": (4, np.float32), "albedo": (4, np.float32),
               "material": (4, np.float32), "normal": (2, np.float32), "pos": (4, np.float32), "instance_id": (1, np.int32),
               "screen_motion": (2, np.float32)}

    def run_targets(self, targets: dict, viewports=1, stream=None):
        """stage::run with a gbuffer: `targets` maps any subset of TARGETS to device images."""
        unknown = set(targets) - set(self.TARGETS)
        if unknown:
            raise ValueError(f"unknown gbuffer targets: {sorted(unknown)}")
        t = _lib.PtTargetsC()
        for name, buf in targets.items():
            setattr(t, name, _ptr(buf))
        tw, th = get_distribution_target_size(self.distribution)
        check(_lib.lib().trhip_pt_render_targets(self.h, C.byref(t), tw, th, viewports, stream))

    def set_profiling(self, count_work=False, detailed_timing=False):
        check(_lib.lib().trhip_pt_set_profiling(self.h, int(count_work), int(detailed_timing)))

    def counters(self) -> dict:
        c = CountersC()
        check(_lib.lib().trhip_pt_get_counters(self.h, C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in CountersC._fields_}

    def reset_counters(self):
        check(_lib.lib().trhip_pt_reset_counters(self.h))

    def light_counters(self) -> dict:
        """trhip_pt_get_light_counters: sphere tests, light-tree node visits and walks that fell back to the loop (stack full), of the
        closest-hit rays (counted under count_work)."""
        c = LightCountersC()
        check(_lib.lib().trhip_pt_get_light_counters(self.h, C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in LightCountersC._fields_}

    def max_stack_depth(self) -> int:
        """trhip_pt_get_max_stack_depth: the deepest per-ray traversal stack since the counters were cleared (counted under count_work)."""
        d = C.c_uint32(0)
        check(_lib.lib().trhip_pt_get_max_stack_depth(self.h, C.byref(d)))
        return int(d.value)

    def set_terminal_query(self, mode: int):
        """trhip_pt_set_terminal_query: _lib.TERMINAL_QUERY_AUTO (the default: the last bounce is a first-hit emitter query where the
        scene allows it) or TERMINAL_QUERY_OFF.  Frames and ray counts do not depend on the mode."""
        check(_lib.lib().trhip_pt_set_terminal_query(self.h, mode))

    def terminal_counters(self) -> dict:
        """trhip_pt_get_terminal_counters: blocked_rays / fallback_rays of the terminal query (counted under count_work), in_effect,
        emitter_triangles, threshold."""
        c = TerminalCountersC()
        check(_lib.lib().trhip_pt_get_terminal_counters(self.h, C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in TerminalCountersC._fields_ if n != "pad"}

    def set_primary_start(self, mode: int):
        """trhip_pt_set_primary_start: _lib.PRIMARY_START_AUTO (the default: no ray generation launch, the closest-hit launch of bounce 0
        computes the camera rays, where the stage allows it) or PRIMARY_START_OFF.  Frames and ray counts do not depend on the mode."""
        check(_lib.lib().trhip_pt_set_primary_start(self.h, mode))

    def primary_start(self) -> dict:
        """trhip_pt_get_primary_start: mode (what was set, -1 none), in_effect (what the next frame does), last_frame (what the last frame
        rendered did, -1 none yet)."""
        p = _lib.PrimaryStartInfoC()
        check(_lib.lib().trhip_pt_get_primary_start(self.h, C.byref(p)))
        return {"mode": int(p.mode), "in_effect": bool(p.in_effect), "last_frame": int(p.last_frame)}

    def timings(self) -> dict:
        t = TimingsC()
        check(_lib.lib().trhip_pt_get_timings(self.h, C.byref(t)))
        return {n: float(getattr(t, n)) for n, _ in TimingsC._fields_}

    def program(self) -> dict:
        """Which shading program renders this stage, resolved now (trhip_pt_get_program): kind ("general" | "cli" | "compiled"), ieee,
        identity (what the ranks of a job compare), key (the pinned option fields as text)."""
        from ._lib import ProgramInfoC
        p = ProgramInfoC()
        if not hasattr(_lib.lib(), "trhip_pt_get_program"):      # an older build named by TRHIP_LIB (A/B runs)
            return {"kind": "general", "ieee": False, "identity": 0, "key": "unknown: the library predates trhip_pt_get_program"}
        check(_lib.lib().trhip_pt_get_program(self.h, C.byref(p)))
        return {"kind": ("general", "cli", "compiled")[p.kind], "ieee": bool(p.ieee), "identity": int(p.identity), "key": p.key.decode()}

    def phase_counters(self) -> dict:
        """Wave-level phase statistics of the counting trace kernels (trhip_pt_get_phase_counters)."""
        from ._lib import PhaseCountersC
        p = PhaseCountersC()
        check(_lib.lib().trhip_pt_get_phase_counters(self.h, C.byref(p)))
        out = {n: int(getattr(p, n)) for n, _ in PhaseCountersC._fields_ if n != "lane_node_phase_hist"}
        out["lane_node_phase_hist"] = [int(x) for x in p.lane_node_phase_hist]
        return out

    def close(self):
        if self.h:
            _lib.lib().trhip_pt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DirectStage(PathTracerStage):
    """direct_stage(device&, scene_stage&, const gbuffer_target&, const options&): first hit + samples_per_pass light samples
    (src/direct_stage.{hh,cc}); same surface as PathTracerStage."""
    _create = "trhip_direct_create"


class FeatureStage:
    """feature_stage: primary-hit AOVs from the same traversal."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, feature: int, distribution: DistributionParams, projection=0,
                 min_ray_dist=1e-4, default_value=(np.nan,) * 4):
        self.ctx, self.ss, self.feature, self.distribution = ctx, scene_stage, feature, distribution
        self.projection, self.min_ray_dist, self.default_value = projection, min_ray_dist, default_value

    def run(self, color_target, viewport=0, stream=None):
        tw, th = get_distribution_target_size(self.distribution)
        d = _dist_c(self.distribution)
        dv = (C.c_float * 4)(*self.default_value)
        check(_lib.lib().trhip_feature_render(self.ctx.h, self.feature, C.byref(d), self.projection, viewport, self.min_ray_dist, dv,
                                              _ptr(color_target), tw, th, stream))


class StitchStage:
    """stitch_stage: scatter non-primary partial images into the primary image."""

    def __init__(self, ctx: Context, size, blend_ratio=1.0):
        self.ctx, self.size, self.blend_ratio = ctx, tuple(size), blend_ratio

    def set_blend_ratio(self, r):
        self.blend_ratio = r

    def run_one(self, partial_dist: DistributionParams, partial, primary, viewports=1, stream=None):
        pw, ph = get_distribution_target_size(partial_dist)
        d = _dist_c(partial_dist)
        check(_lib.lib().trhip_stitch(self.ctx.h, C.byref(d), _ptr(partial), pw, ph, _ptr(primary), viewports, self.blend_ratio, stream))


    def run_all(self, partial_dists, partials, primary, viewports=1, stream=None):
        """Every partial image in one launch (trhip_stitch_batch)."""
        n = len(partial_dists)
        if n == 0:
            return
        key = tuple((id(p), d.index, d.count, d.strategy) for d, p in zip(partial_dists, partials))
        if getattr(self, "_batch_key", None) != key:      # argument arrays are rebuilt only when the partials change
            ds = (DistributionC * n)(*[_dist_c(d) for d in partial_dists])
            ptrs = (C.c_void_p * n)(*[_ptr(p) for p in partials])
            sizes = [get_distribution_target_size(d) for d in partial_dists]
            pws = (C.c_uint32 * n)(*[w for w, _ in sizes])
            phs = (C.c_uint32 * n)(*[h for _, h in sizes])
            self._batch_key, self._batch_args = key, (ds, ptrs, pws, phs)
        ds, ptrs, pws, phs = self._batch_args
        check(_lib.lib().trhip_stitch_batch(self.ctx.h, n, ds, ptrs, pws, phs, _ptr(primary), viewports, self.blend_ratio, stream))


class TonemapStage:
    """tonemap_stage (filmic default, exposure 1, gamma 2.2; alpha grid only when not headless)."""

    def __init__(self, ctx: Context, op=TONEMAP_FILMIC, exposure=1.0, gamma=2.2, alpha_grid_background=False):
        self.ctx = ctx
        self.info = TonemapInfoC(op, exposure, gamma, 16 if alpha_grid_background else 0)

    def run(self, src, dst, width, height, layers=1, stream=None):
        check(_lib.lib().trhip_tonemap(self.ctx.h, _ptr(src), _ptr(dst), width, height, layers, C.byref(self.info), stream))


def _device_images(struct, images: dict, allowed, who, noun):
    """A ctypes struct of device pointers filled from a dict; `noun` is the stage's own word for an entry of it."""
    unknown = set(images) - set(allowed)
    if unknown:
        raise ValueError(f"{who}: not {noun}: {sorted(unknown)}")
    f = struct()
    for name, buf in images.items():
        setattr(f, name, None if buf is None else _ptr(buf))
    return f


class _PostStage:
    """What the post-processing stages share: the handle of a trhip_<PREFIX>_* object, its end, its timer and its downloads."""

    PREFIX = TIMINGS = h = None

    def _fn(self, name):
        return getattr(_lib.lib(), f"trhip_{self.PREFIX}_{name}")

    def _create(self, *args):
        h = C.c_void_p()
        check(self._fn("create")(*args, C.byref(h)))
        self.h = h.value

    def _images(self, struct, images: dict, allowed, noun="an image the stage reads"):
        return _device_images(struct, images, allowed, type(self).__name__, noun)

    def timings(self) -> dict:
        """The stage's timer as the C struct names it: device ms of the last frame, the frames run, the reference's timer name if it has one."""
        t = self.TIMINGS()
        check(self._fn("get_timings")(self.h, C.byref(t)))
        values = ((n, getattr(t, n)) for n, _ in t._fields_)
        return {n: v.decode() if isinstance(v, bytes) else v for n, v in values}

    def _download(self, code, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(self._fn("download")(self.h, code, out.ctypes.data, out.nbytes))
        return out

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BmfrStage(_PostStage):
    """bmfr_stage(device&, gbuffer_target& current_features, gbuffer_target& prev_features, const options&) (src/bmfr_stage.{hh,cc}):
    the BMFR denoiser between the path tracer and the tonemap stage.  The stage keeps last frame's normal / pos and its histories
    itself (trhip_bmfr_*, include/trhip.h); `settings`: _lib.BMFR_DIFFUSE_ONLY (--denoiser=bmfr) or BMFR_DIFFUSE_SPECULAR."""

    PREFIX, TIMINGS = "bmfr", _lib.BmfrTimingsC
    FEATURES = ("color", "diffuse", "albedo", "normal", "pos", "screen_motion", "instance_id")
    # trhip_bmfr_download: name -> (code, numpy dtype, shape(stage))
    BUFFERS = {
        "noisy_diffuse": (_lib.BMFR_NOISY_DIFFUSE, np.float32, lambda s: (s.layers, s.size[1], s.size[0], 4)),
        "noisy_specular": (_lib.BMFR_NOISY_SPECULAR, np.float32, lambda s: (s.layers, s.size[1], s.size[0], 4)),
        "filtered_diffuse": (_lib.BMFR_FILTERED_DIFFUSE, np.float32, lambda s: (s.layers, s.size[1], s.size[0], 4)),
        "filtered_specular": (_lib.BMFR_FILTERED_SPECULAR, np.float32, lambda s: (s.layers, s.size[1], s.size[0], 4)),
        "feature_rows": (_lib.BMFR_FEATURE_ROWS, np.float32, lambda s: (s.blocks, 10 + s.channels, 1024)),
        "weights": (_lib.BMFR_WEIGHTS, np.float32, lambda s: (s.blocks, s.channels, 10)),
        "min_max": (_lib.BMFR_MIN_MAX, np.float32, lambda s: (s.blocks, 6, 2)),
        "accept_bits": (_lib.BMFR_ACCEPT_BITS, np.uint8, lambda s: (s.layers, s.size[1], s.size[0])),
        "block_offsets": (_lib.BMFR_BLOCK_OFFSETS, np.int32, lambda s: (16, 2)),
        "previous_normal": (_lib.BMFR_PREVIOUS_NORMAL, np.float32, lambda s: (s.layers, s.size[1], s.size[0], 2)),
        "previous_pos": (_lib.BMFR_PREVIOUS_POS, np.float32, lambda s: (s.layers, s.size[1], s.size[0], 4)),
    }

    def __init__(self, ctx: Context, size, layers=1, settings=_lib.BMFR_DIFFUSE_ONLY, noise_amount=0.0):
        self.ctx, self.size, self.layers, self.settings = ctx, (int(size[0]), int(size[1])), int(layers), int(settings)
        self.channels = 3 if self.settings == _lib.BMFR_DIFFUSE_ONLY else 6
        self.block_grid = ((self.size[0] + 31) // 32 + 1, (self.size[1] + 31) // 32 + 1)
        self.blocks = self.block_grid[0] * self.block_grid[1] * self.layers
        opt = _lib.BmfrOptionsC(self.settings, float(noise_amount))
        self._create(getattr(ctx, "h", None), C.byref(opt), self.size[0], self.size[1], self.layers)

    def run(self, targets: dict, frame_counter: int, stream=None):
        """stage::run: denoises targets["color"] in place from the other gbuffer entries (device images of the stage's size)."""
        f = self._images(_lib.BmfrFeaturesC, targets, self.FEATURES, "a feature the stage reads")
        check(_lib.lib().trhip_bmfr_run(self.h, C.byref(f), int(frame_counter) & 0xFFFFFFFF, stream))

    def reset_history(self):
        check(_lib.lib().trhip_bmfr_reset_history(self.h))

    def download(self, name: str) -> np.ndarray:
        """A buffer of the stage as the last frame left it (trhip_bmfr_download; test hook)."""
        code, dtype, shape = self.BUFFERS[name]
        return self._download(code, shape(self), dtype)


def fit_blocks(ctx: Context, matrices: np.ndarray) -> np.ndarray:
    """trhip_bmfr_fit_blocks: the BMFR least-squares fit alone.  matrices [blocks][10 + channels][1024] (features scaled and with
    noise, then 3 or 6 channels) -> weights [blocks][channels][10]."""
    m = np.ascontiguousarray(matrices, dtype=np.float32)
    if m.ndim != 3 or m.shape[2] != 1024 or m.shape[1] not in (13, 16):
        raise ValueError("fit_blocks: matrices must be [blocks][13 or 16][1024]")
    blocks, channels = m.shape[0], m.shape[1] - 10
    if blocks == 0:
        return np.zeros((0, channels, 10), np.float32)
    d_m = ctx.alloc(m.nbytes).upload(m)
    d_w = ctx.alloc(blocks * channels * 40)
    check(_lib.lib().trhip_bmfr_fit_blocks(ctx.h, blocks, channels, d_m.ptr, d_w.ptr, None))
    return d_w.download((blocks, channels, 10), np.float32)


class _LayerView:
    """Layers [first, ...) of a device image (what a stage that renders a run of the viewport list writes)."""

    def __init__(self, image, byte_offset):
        self.image, self.byte_offset = image, int(byte_offset)

    def data_ptr(self):
        return _ptr(self.image) + self.byte_offset


def viewport_runs(viewports):
    """A viewport list as arithmetic runs [(base, stride, count), ...] in list order - what trhip_pt_set_shard expresses: 0,4,8 is one
    run, 18..26 is one run, 0,1,5 is (0, 1, 2), (5, 1, 1)."""
    runs, i, v = [], 0, [int(x) for x in viewports]
    while i < len(v):
        count, stride = 1, 1
        if i + 1 < len(v) and v[i + 1] > v[i]:
            stride = v[i + 1] - v[i]
            while i + count < len(v) and v[i + count] - v[i + count - 1] == stride:
                count += 1
        runs.append((v[i], stride, count))
        i += count
    return runs


def check_viewport_list(viewports, total, what="spatial_reprojection"):
    """The active viewports of a sparse light field: a non-empty list of distinct viewports of the grid that leaves some to reproject."""
    v = [int(x) for x in viewports]
    if not v:
        raise ValueError(f"{what}: the viewport list is empty")
    bad = [x for x in v if x < 0 or x >= total]
    if bad:
        raise ValueError(f"{what}: viewport {bad[0]} is out of range (the scene has {total} viewports)")
    if len(set(v)) != len(v):
        raise ValueError(f"{what}: a viewport is listed twice")
    if len(v) >= total:
        raise ValueError(f"{what}: the list names every viewport: there is nothing to reproject")
    return v


class GbufferStage:
    """The first-hit G-buffer of viewports that are not path traced (trhip_gbuffer_render): normal, pos and instance id of one ray through
    every pixel centre, for a list of viewports in one launch, as compact layers in list order."""

    TARGETS = ("normal", "pos", "instance_id")

    def __init__(self, ctx: Context, scene_stage: SceneStage, size, projection=0, min_ray_dist=1e-4):
        self.ctx, self.ss, self.size = ctx, scene_stage, (int(size[0]), int(size[1]))
        self.projection, self.min_ray_dist = int(projection), float(min_ray_dist)

    def alloc_targets(self, layers) -> dict:
        w, h = self.size
        return {n: self.ctx.alloc(max(layers, 1) * w * h * PathTracerStage.TARGETS[n][0] * 4).zero() for n in self.TARGETS}

    def run(self, viewports, targets: dict, stream=None):
        t = _device_images(_lib.GbufferTargetsC, targets, self.TARGETS, "GbufferStage", "a target the pass writes")
        v = (C.c_uint32 * max(len(viewports), 1))(*[int(x) for x in viewports])
        check(_lib.lib().trhip_gbuffer_render(self.ctx.h, self.projection, v, len(viewports), self.min_ray_dist, C.byref(t), self.size[0], self.size[1], stream))


class SpatialReprojectionStage(_PostStage):
    """spatial_reprojection_stage (src/spatial_reprojection_stage.{hh,cc}): fills the viewports that were not path traced from the ones
    that were, through the G-buffer (trhip_spatial_reprojection_*, include/trhip.h).  `source_viewports`: the path-traced viewports, in the
    order of the source images' layers; the output holds every viewport in natural order."""

    PREFIX, TIMINGS = "spatial_reprojection", _lib.ReprojectionTimingsC
    SOURCES = ("color", "normal", "pos", "instance_id")
    DESTINATIONS = ("normal", "pos", "instance_id")

    def __init__(self, ctx: Context, size, total_viewports, source_viewports, default_value=(np.nan,) * 4):
        self.ctx, self.size, self.total = ctx, (int(size[0]), int(size[1])), int(total_viewports)
        self.sources = [int(v) for v in source_viewports]
        self.destinations = [v for v in range(self.total) if v not in set(self.sources)]
        src = (C.c_uint32 * max(len(self.sources), 1))(*[v & 0xFFFFFFFF for v in self.sources])
        dv = (C.c_float * 4)(*default_value)
        self._create(getattr(ctx, "h", None), self.size[0], self.size[1], max(self.total, 0), src, len(self.sources), dv)

    def run(self, sources: dict, destinations: dict, color_out, stream=None):
        s = self._images(_lib.ReprojectionImagesC, sources, self.SOURCES)
        d = self._images(_lib.ReprojectionImagesC, destinations, self.DESTINATIONS)
        check(_lib.lib().trhip_spatial_reprojection_run(self.h, C.byref(s), C.byref(d), _ptr(color_out), stream))

    def decisions(self) -> np.ndarray:
        """The decision record of the last frame, [destinations][h][w] (fields kind, slot, bits, ox, oy; test hook)."""
        return self._download(_lib.REPROJECTION_DECISIONS, (len(self.destinations), self.size[1], self.size[0]), np.dtype(_lib.REPROJECTION_RECORD))


class TemporalReprojectionStage(_PostStage):
    """temporal_reprojection_stage (src/temporal_reprojection_stage.{hh,cc}): blends last frame's colour, found through screen_motion, into
    the path-traced layers: color = mix(color, reprojected, ratio) (trhip_temporal_reprojection_*, include/trhip.h).  The stage keeps last
    frame's colour, normal and pos itself."""

    PREFIX, TIMINGS = "temporal_reprojection", _lib.ReprojectionTimingsC
    IMAGES = ("color", "normal", "pos", "screen_motion", "instance_id")
    BUFFERS = {"previous_color": (_lib.REPROJECTION_PREVIOUS_COLOR, 4), "previous_normal": (_lib.REPROJECTION_PREVIOUS_NORMAL, 2),
               "previous_pos": (_lib.REPROJECTION_PREVIOUS_POS, 4)}

    def __init__(self, ctx: Context, size, layers=1, ratio=0.75):
        self.ctx, self.size, self.layers, self.ratio = ctx, (int(size[0]), int(size[1])), int(layers), float(ratio)
        self._create(getattr(ctx, "h", None), self.size[0], self.size[1], max(self.layers, 0), self.ratio)

    def run(self, images: dict, stream=None):
        """stage::run: blends into images["color"] in place."""
        f = self._images(_lib.ReprojectionImagesC, images, self.IMAGES)
        check(_lib.lib().trhip_temporal_reprojection_run(self.h, C.byref(f), stream))

    def reset_history(self):
        check(_lib.lib().trhip_temporal_reprojection_reset_history(self.h))

    def decisions(self) -> np.ndarray:
        return self._download(_lib.REPROJECTION_DECISIONS, (self.layers, self.size[1], self.size[0]), np.dtype(_lib.REPROJECTION_RECORD))

    def download(self, name: str) -> np.ndarray:
        """The history the last frame left (test hook)."""
        code, ch = self.BUFFERS[name]
        return self._download(code, (self.layers, self.size[1], self.size[0], ch))


class TaaStage(_PostStage):
    """taa_stage (src/taa_stage.{hh,cc}): temporal antialiasing behind the tonemap stage (trhip_taa_*, include/trhip.h).  The stage keeps
    its two history images itself and reads the scene's cameras and previous cameras (with their jitter in pan.zw) on the device.
    `options`: alpha (weight of the new frame, 1 / sequence length), gamma (the tonemap stage's), edge_dilation, anti_shimmer,
    base_camera_index, projection."""

    PREFIX, TIMINGS = "taa", _lib.TaaTimingsC
    IMAGES = ("src", "dst", "screen_motion", "pos", "instance_id")
    DEFAULTS = dict(alpha=0.125, gamma=2.2, edge_dilation=True, anti_shimmer=False, base_camera_index=0, projection=0)

    def __init__(self, ctx: Context, size, layers=1, options: Optional[dict] = None):
        unknown = set(options or {}) - set(self.DEFAULTS)
        if unknown:
            raise ValueError(f"TaaStage: not an option of the stage: {sorted(unknown)}")
        self.options = dict(self.DEFAULTS, **(options or {}))
        self.ctx, self.size, self.layers = ctx, (int(size[0]), int(size[1])), int(layers)
        o = self.options
        opt = _lib.TaaOptionsC(float(o["alpha"]), float(o["gamma"]), int(bool(o["edge_dilation"])), int(bool(o["anti_shimmer"])),
                               int(o["base_camera_index"]), int(o["projection"]))
        self._create(getattr(ctx, "h", None), C.byref(opt), max(self.size[0], 0), max(self.size[1], 0), max(self.layers, 0))

    def run(self, images: dict, stream=None):
        """stage::run: images["dst"] = this frame's images["src"] blended into the stage's history (dst may be src)."""
        f = self._images(_lib.TaaImagesC, images, self.IMAGES)
        check(_lib.lib().trhip_taa_run(self.h, C.byref(f), stream))

    def reset_history(self):
        check(_lib.lib().trhip_taa_reset_history(self.h))

    def download(self, name: str) -> np.ndarray:
        """"history": RGBA32F, what the next frame will read; "decisions": the decision byte per pixel (test hooks)."""
        if name == "history":
            return self._download(_lib.TAA_HISTORY, (self.layers, self.size[1], self.size[0], 4))
        if name == "decisions":
            return self._download(_lib.TAA_DECISIONS, (self.layers, self.size[1], self.size[0]), np.uint8)
        raise KeyError(name)


class LookingGlassStage(_PostStage):
    """looking_glass_composition_stage (src/looking_glass_composition_stage.{hh,cc}): interleaves the views of a light field, sub-pixel by
    sub-pixel, into the one image a lenticular panel shows (trhip_lkg_*, include/trhip.h).  `view_size`: the size of one view; `out_size`: the
    panel's.  `options`: viewport_count (1..255), pitch / tilt / center (the reference's corrected_pitch, tilt, center:
    looking_glass.LookingGlassCalibration.stage_options), invert, record_view_indices.  The stage has no history."""

    PREFIX, TIMINGS = "lkg", _lib.LkgTimingsC
    DEFAULTS = dict(viewport_count=48, pitch=0.0, tilt=0.0, center=0.0, invert=False, record_view_indices=False)

    def __init__(self, ctx: Context, view_size, out_size, options: Optional[dict] = None):
        unknown = set(options or {}) - set(self.DEFAULTS)
        if unknown:
            raise ValueError(f"LookingGlassStage: not an option of the stage: {sorted(unknown)}")
        self.options = dict(self.DEFAULTS, **(options or {}))
        self.ctx = ctx
        self.view_size, self.out_size = (int(view_size[0]), int(view_size[1])), (int(out_size[0]), int(out_size[1]))
        o = self.options
        opt = _lib.LkgOptionsC(max(int(o["viewport_count"]), 0), float(o["pitch"]), float(o["tilt"]), float(o["center"]), int(bool(o["invert"])),
                               int(bool(o["record_view_indices"])))
        self._create(getattr(ctx, "h", None), C.byref(opt), max(self.view_size[0], 0), max(self.view_size[1], 0), max(self.out_size[0], 0), max(self.out_size[1], 0))

    def run(self, src, dst=None, dst_rgba8=None, stream=None):
        """stage::run: `src` RGBA32F [views][h][w] in display space; `dst` RGBA32F [out_h][out_w] and / or `dst_rgba8` uint8 [out_h][out_w][4]."""
        check(_lib.lib().trhip_lkg_run(self.h, None if src is None else _ptr(src), None if dst is None else _ptr(dst),
                                       None if dst_rgba8 is None else _ptr(dst_rgba8), stream))

    def view_indices(self) -> np.ndarray:
        """uint8 [out_h][out_w][4]: the view the last frame took r, g and b from; 0 (record_view_indices only)."""
        return self._download(_lib.LKG_VIEW_INDICES, (self.out_size[1], self.out_size[0], 4), np.uint8)


def sh_coef_count(order: int) -> int:
    """sh_grid::get_coef_count (src/sh_grid.cc)."""
    return (int(order) + 1) ** 2


def sh_options(**kw) -> dict:
    """sh_path_tracer_stage::options at the reference's defaults (src/sh_path_tracer_stage.hh:14-31; rt_stage::options for the rest)."""
    o = dict(max_bounces=8, min_ray_dist=1e-4, rng_seed=0, sampler=SAMPLER_UNIFORM_RANDOM, samples_per_probe=1, film=FILM_BLACKMAN_HARRIS,
             film_radius=1.0, mis_mode=MIS_POWER_HEURISTIC, russian_roulette_delta=0.0, temporal_ratio=0.02, indirect_clamping=100.0,
             regularization_gamma=1.0, nee_point=1.0, nee_directional=1.0, nee_envmap=1.0, nee_triangles=1.0, bounce_mode=BOUNCE_MATERIAL,
             tri_light_mode=TRI_LIGHT_SOLID_ANGLE, sh_order=2)
    unknown = set(kw) - set(o)
    if unknown:
        raise AttributeError(f"not an option of the SH path tracer stage: {sorted(unknown)}")
    o.update(kw)
    return o


def _sh_grid_data_dict(g) -> dict:
    return dict(transform=np.array(g.transform, dtype=np.float32).reshape(4, 4).T, normal_transform=np.array(g.normal_transform, dtype=np.float32).reshape(4, 4).T,
                grid_size=tuple(g.grid_size), mix_ratio=float(g.mix_ratio), cell_scale=np.array(g.cell_scale, dtype=np.float32),
                rotation_x=float(g.rotation_x), rotation_y=float(g.rotation_y))


def sh_grid_parameters(grid: ShGrid, samples_per_probe: int, frame_counter: int, history_length: int, temporal_ratio: float) -> dict:
    """grid_data_buffer of render number `history_length` of `grid` at `frame_counter` (src/sh_path_tracer_stage.cc:115-137): transform and
    normal_transform as mathematical 4x4, cell_scale, the rotations of the direction lattice, mix_ratio.  Needs no device."""
    t = np.ascontiguousarray(np.asarray(grid.transform, dtype=np.float64).T, dtype=np.float32).reshape(16)
    sc = np.asarray(grid.scaling, dtype=np.float32).reshape(3)
    res = (C.c_uint32 * 3)(*[int(r) for r in grid.resolution])
    g = _lib.ShGridDataC()
    check(_lib.lib().trhip_sh_pack_grid_data(t.ctypes.data_as(C.POINTER(C.c_float)), sc.ctypes.data_as(C.POINTER(C.c_float)), res, int(samples_per_probe),
                                             int(frame_counter) & 0xFFFFFFFF, int(history_length), float(temporal_ratio), C.byref(g)))
    return _sh_grid_data_dict(g)


class ShPathTracerStage(_PostStage):
    """sh_path_tracer_stage(device&, scene_stage&, texture& output_grid, layout, const options&) followed by sh_compact_stage
    (src/sh_path_tracer_stage.{hh,cc}, src/sh_compact_stage.cc): bakes one sh_grid (trhip_sh_*, include/trhip.h).  `grid`: a scene.ShGrid;
    `options`: sh_options().  The stage owns both volumes: RGBA32F [rz][ry * C][rx] and its RGBA16F copy."""

    PREFIX, TIMINGS = "sh", _lib.ShTimingsC

    def __init__(self, ctx: Context, scene_stage: Optional[SceneStage], grid: ShGrid, options: Optional[dict] = None):
        self.options = sh_options(**(options or {}))
        self.ctx, self.scene_stage, self.grid = ctx, scene_stage, grid
        o = self.options
        self.order, self.samples = int(o["sh_order"]), int(o["samples_per_probe"])
        self.resolution = tuple(int(r) for r in grid.resolution)
        path = make_options(**{k: o[k] for k in ("max_bounces", "min_ray_dist", "rng_seed", "sampler", "film", "film_radius", "mis_mode",
                                                 "russian_roulette_delta", "indirect_clamping", "regularization_gamma", "nee_point",
                                                 "nee_directional", "nee_envmap", "nee_triangles", "bounce_mode", "tri_light_mode")})
        opt = _lib.ShOptionsC(self.order, (C.c_uint32 * 3)(*[max(r, 0) for r in self.resolution]), max(self.samples, 0), float(o["temporal_ratio"]))
        self._create(getattr(ctx, "h", None), C.byref(path), C.byref(opt))
        self.set_transform(grid.transform, grid.scaling)

    def set_transform(self, transform, scaling):
        """The grid's transformable: `transform` a mathematical 4x4 (get_global_transform), `scaling` its get_scaling()."""
        t = np.ascontiguousarray(np.asarray(transform, dtype=np.float64).T, dtype=np.float32).reshape(16)      # column-major, as glm
        sc = np.asarray(scaling, dtype=np.float32).reshape(3)
        check(_lib.lib().trhip_sh_set_transform(self.h, t.ctypes.data_as(C.POINTER(C.c_float)), sc.ctypes.data_as(C.POINTER(C.c_float))))

    def set_frame_counter(self, frame_counter: int):
        check(_lib.lib().trhip_sh_set_frame_counter(self.h, frame_counter))

    def reset_history(self):
        check(_lib.lib().trhip_sh_reset_history(self.h))

    def set_lanes(self, lanes: int):
        check(_lib.lib().trhip_sh_set_lanes(self.h, lanes))

    def set_batch_probes(self, probes: int):
        check(_lib.lib().trhip_sh_set_batch_probes(self.h, probes))

    def set_shading_arithmetic(self, ieee: bool):
        check(_lib.lib().trhip_sh_set_shading_arithmetic(self.h, 1 if ieee else 0))

    def grid_data(self) -> dict:
        """grid_data_buffer as the next run would pack it: transform and normal_transform as mathematical 4x4, cell_scale, the rotations,
        mix_ratio."""
        g = _lib.ShGridDataC()
        check(_lib.lib().trhip_sh_get_grid_data(self.h, C.byref(g)))
        return _sh_grid_data_dict(g)

    def run(self, stream=None):
        """stage::run: one render of the whole grid, blended into the stage's history."""
        check(_lib.lib().trhip_sh_render(self.h, stream))

    @property
    def shape(self):
        rx, ry, rz = self.resolution
        return (rz, ry * sh_coef_count(self.order), rx, 4)

    def download(self, name: str = "grid") -> np.ndarray:
        """"grid": RGBA32F [rz][ry * C][rx][4]; "half": the RGBA16F copy."""
        if name == "grid":
            return self._download(_lib.SH_GRID, self.shape)
        if name == "half":
            return self._download(_lib.SH_GRID_HALF, self.shape, np.float16)
        raise KeyError(name)

    def device_grids(self):
        """The device addresses of the two volumes, for a consumer."""
        a, b = C.c_void_p(), C.c_void_p()
        check(_lib.lib().trhip_sh_get_grids(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def counters(self) -> dict:
        c = CountersC()
        check(_lib.lib().trhip_sh_get_counters(self.h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in c._fields_}

    def primary_start(self) -> dict:
        """trhip_sh_get_primary_start: as PathTracerStage.primary_start; a probe stage always starts its paths with its own ray generation."""
        p = _lib.PrimaryStartInfoC()
        check(_lib.lib().trhip_sh_get_primary_start(self.h, C.byref(p)))
        return {"mode": int(p.mode), "in_effect": bool(p.in_effect), "last_frame": int(p.last_frame)}

    def set_profiling(self, count_work=False, detailed_timing=False):
        check(_lib.lib().trhip_sh_set_profiling(self.h, int(count_work), int(detailed_timing)))

    def reset_counters(self):
        check(_lib.lib().trhip_sh_reset_counters(self.h))


class ShRenderer:
    """sh_renderer (src/sh_renderer.{hh,cc}): one ShPathTracerStage per sh_grid of the scene."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, grids, options: Optional[dict] = None):
        if not grids:
            raise ValueError("ShRenderer: the scene has no light-probe grid (TR_data.light_probe of type GRID)")
        self.stages = [ShPathTracerStage(ctx, scene_stage, g, options) for g in grids]

    def render(self, stream=None):
        for st in self.stages:
            st.run(stream)

    def download(self, name: str = "grid"):
        return [st.download(name) for st in self.stages]

    def close(self):
        for st in self.stages:
            st.close()


def dshgi_pick_grid(grids, position) -> int:
    """get_sh_grid, then get_largest_sh_grid (src/scene.cc:163-211) for `position`: the index into `grids` (scene.ShGrid), -1 without any.
    Needs no device (trhip_dshgi_pick_grid)."""
    n = len(grids)
    if n == 0:
        return -1
    t = np.ascontiguousarray([np.asarray(g.transform, dtype=np.float64).T for g in grids], dtype=np.float32).reshape(n * 16)
    sc = np.ascontiguousarray([g.scaling for g in grids], dtype=np.float32).reshape(n * 3)
    res = np.ascontiguousarray([g.resolution for g in grids], dtype=np.uint32).reshape(n * 3)
    rad = np.ascontiguousarray([g.radius for g in grids], dtype=np.float32)
    pos = np.ascontiguousarray(position, dtype=np.float32).reshape(3)
    fp, index = C.POINTER(C.c_float), C.c_int32(-1)
    check(_lib.lib().trhip_dshgi_pick_grid(t.ctypes.data_as(fp), sc.ctypes.data_as(fp), res.ctypes.data_as(C.POINTER(C.c_uint32)), rad.ctypes.data_as(fp), n,
                                           pos.ctypes.data_as(fp), C.byref(index)))
    return index.value


def dshgi_instance_grids(grids, instances: np.ndarray) -> np.ndarray:
    """sh_grid_index of every instance (src/scene_stage.cc:1075-1083): the grid picked for model[3], the instance's origin."""
    return np.array([dshgi_pick_grid(grids, inst["model"][3][:3]) for inst in instances], dtype=np.int32)


def brdf_integration_table(ctx: "Context", size=256, samples=1024, stream=None) -> "DeviceBuffer":
    """The BRDF-integration table generated on the device (trhip_brdf_integration_generate): RG32F [size][size]."""
    buf = ctx.alloc(size * size * 8)
    check(_lib.lib().trhip_brdf_integration_generate(ctx.h, size, samples, buf.data_ptr(), stream))
    return buf


def load_brdf_integration(path: str) -> np.ndarray:
    """The table of an EXR file as texture() sees it (data/brdf_integration.exr: channels R and G, row 0 first): (h, w, 2) float32."""
    from .exr import load_exr
    img = load_exr(path)
    if img.shape[2] < 2:
        raise ValueError(f"{path}: {img.shape[2]} channel; a BRDF-integration table has R (scale) and G (bias)")
    return np.ascontiguousarray(img[..., :2], dtype=np.float32)


class DshgiStage(_PostStage):
    """The indirect light of dshgi_renderer (src/dshgi_renderer.{hh,cc}, shader/forward.frag): first hit, SH grid lookup, brdf_indirect,
    added to the direct stage's colour (trhip_dshgi_*, include/trhip.h).  `size`: (w, h); `layers`: the viewports of a frame."""

    PREFIX, TIMINGS = "dshgi", _lib.DshgiTimingsC

    def __init__(self, ctx: Context, scene_stage: Optional[SceneStage], size, layers=1, order=2, use_probe_visibility=False, record_surface=False,
                 projection=0, min_ray_dist=1e-4):
        self.ctx, self.scene_stage, self.size, self.layers = ctx, scene_stage, tuple(size), int(layers)
        self.order, self.projection, self.min_ray_dist = int(order), int(projection), float(min_ray_dist)
        opt = _lib.DshgiOptionsC(self.order, int(bool(use_probe_visibility)), int(bool(record_surface)))
        self._create(getattr(ctx, "h", None), C.byref(opt), max(int(self.size[0]), 0), max(int(self.size[1]), 0), max(self.layers, 0))

    def set_grids(self, grids, images):
        """`grids`: scene.ShGrid; `images`: the RGBA16F volume of each on the device (ShPathTracerStage.device_grids()[1] or an upload)."""
        n = len(grids)
        arr = (_lib.DshgiGridC * max(n, 1))()
        for g, img, a in zip(grids, images, arr):
            a.grid_half_dev = _ptr(img)
            a.resolution = (C.c_uint32 * 3)(*[int(r) for r in g.resolution])
            a.transform = (C.c_float * 16)(*np.asarray(g.transform, dtype=np.float64).T.astype(np.float32).reshape(16).tolist())
            a.scaling = (C.c_float * 3)(*[float(s) for s in g.scaling])
        check(_lib.lib().trhip_dshgi_set_grids(self.h, arr, n))

    def set_instance_grids(self, instance_grids):
        a = np.ascontiguousarray(instance_grids, dtype=np.int32)
        check(_lib.lib().trhip_dshgi_set_instance_grids(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size))

    def set_brdf_integration(self, table, w, h):
        """`table`: RG32F [h][w] on the device; the stage keeps a copy."""
        check(_lib.lib().trhip_dshgi_set_brdf_integration(self.h, _ptr(table), w, h))

    def run(self, viewports, direct, out, stream=None):
        """One frame: out = direct + indirect for the listed viewports; `direct` None writes the indirect term alone, `out` may be `direct`."""
        v = np.ascontiguousarray(viewports, dtype=np.uint32)
        check(_lib.lib().trhip_dshgi_render(self.h, self.projection, v.ctypes.data_as(C.POINTER(C.c_uint32)), v.size, self.min_ray_dist,
                                            None if direct is None else _ptr(direct), _ptr(out), stream))

    def download(self, name: str = "indirect") -> np.ndarray:
        """"indirect": RGBA32F [layers][h][w][4]; "surface": the record per pixel (record_surface), a structured array [layers][h][w]."""
        shape = (self.layers, self.size[1], self.size[0])
        if name == "indirect":
            return self._download(_lib.DSHGI_INDIRECT, shape + (4,))
        if name == "surface":
            return self._download(_lib.DSHGI_SURFACE, shape, np.dtype(_lib.DSHGI_SURFACE_DTYPE))
        raise KeyError(name)


class _ViewportFrameRenderer:
    """What the single-device renderers of whole viewports share (DshgiRenderer, RestirDiRenderer, RestirGiRenderer): `size`, `viewports` (one per camera), the
    `color` and `display` images of every viewport, the tonemap stage and the tail of a frame that runs it - all on one stream."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, scene: SceneDesc, size, tonemap: Optional[TonemapStage],
                 deformation_motion: Optional[bool] = None):
        """`deformation_motion`: None leaves the scene stage's switch (SceneStage.set_deformation_motion) as it stands, else sets it - on
        the caller's scene stage, for every stage that shares it: the switch belongs to the scene, not to this renderer (the C++
        viewport-frame renderers have no such argument and take the switch from the scene stage they are given)."""
        self.ctx, self.ss, self.size = ctx, scene_stage, tuple(size)
        if deformation_motion is not None:
            scene_stage.set_deformation_motion(deformation_motion)
        self.viewports = max(len(scene.cameras), 1)
        self.tonemap = tonemap or TonemapStage(ctx)
        pixels = self.size[0] * self.size[1] * self.viewports
        self.color, self.display = ctx.alloc(pixels * 16).zero(), ctx.alloc(pixels * 16).zero()

    def _finish(self, stream, tonemap):
        if tonemap:
            self.tonemap.run(self.color, self.display, self.size[0], self.size[1], self.viewports, stream)

    def download(self, which="color") -> np.ndarray:
        self.ctx.sync()
        buf = self.color if which == "color" else self.display
        return buf.download((self.viewports, self.size[1], self.size[0], 4))

    def close(self):
        for b in (self.color, self.display):
            b.free()


class DshgiRenderer(_ViewportFrameRenderer):
    """dshgi_renderer (src/dshgi_renderer.{hh,cc}): per frame the scene's probe grids are baked (ShRenderer), the direct stage renders every
    viewport, the indirect light of the grids is added (DshgiStage), the frame is tonemapped - all on one stream.  The first bake has
    history 1, so the grids are complete before they are read.  `options`: the direct stage's PtOptionsC; `sh`: sh_options() of the bake;
    `brdf_integration`: None (the generated 256 x 256 table of 1024 samples), a file name or an (h, w, 2) array.
    Direct light is what the reference's raster pass lights with - point and directional lights: the direct stage samples neither the
    emissive triangles nor the environment map (their weights are set to 0; it still shows them where a pixel sees them), because the probes
    see both and the indirect term carries their light."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, scene: SceneDesc, size, options: PtOptionsC, sh: Optional[dict] = None,
                 use_probe_visibility=False, brdf_integration=None, tonemap: Optional[TonemapStage] = None, record_surface=False,
                 deformation_motion: Optional[bool] = None):
        if not scene.sh_grids:
            raise ValueError("DshgiRenderer: the scene has no light-probe grid (TR_data.light_probe of type GRID)")
        super().__init__(ctx, scene_stage, scene, size, tonemap, deformation_motion)
        self.grids = list(scene.sh_grids)
        self.sh = ShRenderer(ctx, scene_stage, self.grids, sh)
        order = self.sh.stages[0].order
        self.direct = DirectStage(ctx, scene_stage, copy_options(options, nee_triangles=0.0, nee_envmap=0.0),
                                  DistributionParams(self.size, DISTRIBUTION_DUPLICATE, 0, 1, True))
        self.indirect = DshgiStage(ctx, scene_stage, self.size, self.viewports, order, use_probe_visibility, record_surface, options.projection,
                                   options.min_ray_dist)
        self.indirect.set_grids(self.grids, [st.device_grids()[1] for st in self.sh.stages])
        if brdf_integration is None:
            w = h = 256
            table = brdf_integration_table(ctx, w, 1024)
            ctx.sync()
        else:
            host = load_brdf_integration(brdf_integration) if isinstance(brdf_integration, str) else np.ascontiguousarray(brdf_integration, dtype=np.float32)
            h, w = host.shape[:2]
            table = ctx.alloc(host.nbytes).upload(host)
        self.indirect.set_brdf_integration(table, w, h)
        table.free()
        self.set_scene(scene)

    def set_scene(self, scene: SceneDesc):
        """The instances have moved (the scene stage holds them already): every instance picks its grid again."""
        self.instance_grids = dshgi_instance_grids(self.grids, scene.instances)
        self.indirect.set_instance_grids(self.instance_grids)

    def render(self, stream=None, tonemap=True):
        self.sh.render(stream)
        self.direct.reset_accumulated_samples()
        self.direct.run(self.color, self.viewports, stream)
        self.indirect.run(np.arange(self.viewports), self.color, self.color, stream)
        self._finish(stream, tonemap)

    def timings(self) -> dict:
        return {"bake": [st.timings() for st in self.sh.stages], "direct": self.direct.timings(), "indirect": self.indirect.timings()}

    def close(self):
        self.sh.close()
        self.direct.close()
        self.indirect.close()
        super().close()


def restir_di_options(**kw) -> dict:
    """trhip_restir_di_options at the command line's defaults (--restir=4,2,32,16,on), and `visibility` (--restir-visibility=per-target):
    "per-target", "shared" or "sampled", which the stage applies through trhip_restir_di_set_visibility, and `light_selection`
    (--restir-light-selection=uniform): "uniform" or "power" with `uniform_fraction` in (0, 1], applied through
    trhip_restir_di_set_light_selection, and `bsdf_candidates` (--restir-bsdf-candidates=0): 0..8 candidates a pixel drawn from the
    surface's BSDF behind the `candidates` light candidates, at most 32 together, applied through trhip_restir_di_set_bsdf_candidates,
    and `sphere_lights` (--restir-sphere-lights=point): "point" or "area" - a point light with a radius lit as a point or as the sphere it
    is -, applied through trhip_restir_di_set_sphere_lights."""
    o = dict(candidates=4, spatial_samples=2, search_radius=32.0, max_confidence=16.0, temporal_reuse=True, min_ray_dist=1e-4, rng_seed=0,
             record=False, visibility="per-target", light_selection="uniform", uniform_fraction=0.1, bsdf_candidates=0, sphere_lights="point")
    unknown = set(kw) - set(o)
    if unknown:
        raise AttributeError(f"unknown ReSTIR DI option {sorted(unknown)}")
    o.update(kw)
    _restir_visibility_mode(o["visibility"])
    _restir_light_selection_mode(o["light_selection"], o["uniform_fraction"])
    _restir_bsdf_candidates(o["bsdf_candidates"], o["candidates"])
    _restir_sphere_lights_mode(o["sphere_lights"])
    return o


def _restir_visibility_mode(name) -> int:
    if name not in _lib.RESTIR_VISIBILITY:
        raise ValueError(f"unknown ReSTIR DI visibility mode {name!r} ({', '.join(_lib.RESTIR_VISIBILITY)})")
    return _lib.RESTIR_VISIBILITY[name]


def _restir_light_selection_mode(name, uniform_fraction) -> int:
    if name not in _lib.RESTIR_LIGHT_SELECTION:
        raise ValueError(f"unknown ReSTIR DI light selection {name!r} ({', '.join(_lib.RESTIR_LIGHT_SELECTION)})")
    if not 0.0 < float(uniform_fraction) <= 1.0:      # a NaN fails both comparisons
        raise ValueError(f"ReSTIR DI uniform_fraction {uniform_fraction!r} is outside (0, 1]")
    return _lib.RESTIR_LIGHT_SELECTION[name]


def _restir_sphere_lights_mode(name) -> int:
    if name not in _lib.RESTIR_SPHERE_LIGHTS:
        raise ValueError(f"unknown ReSTIR DI sphere lights mode {name!r} ({', '.join(_lib.RESTIR_SPHERE_LIGHTS)})")
    return _lib.RESTIR_SPHERE_LIGHTS[name]


def _restir_bsdf_candidates(n, candidates) -> int:
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 8:
        raise ValueError(f"ReSTIR DI bsdf_candidates {n!r} is outside 0..8")
    if int(n) > 0 and int(candidates) + int(n) > 32:      # without BSDF candidates, `candidates` alone is create's to refuse
        raise ValueError(f"ReSTIR DI candidates {candidates!r} + bsdf_candidates {n!r} is above 32")
    return int(n)


class _RestirStage(_PostStage):
    """What RestirDiStage and RestirGiStage share: `size`: (w, h); `layers`: the viewports of a frame; `options`: the stage's option dict.
    _RECORDS: name -> (download code, dtype); _AXES: a record with one more axis -> the option that is its length."""

    _RECORDS, _AXES = {}, {}

    def _create_stage(self, ctx, scene_stage, size, layers, projection, opt):
        """`opt`: the stage's trhip_restir_*_options."""
        self.ctx, self.scene_stage, self.size, self.layers, self.projection = ctx, scene_stage, tuple(size), int(layers), int(projection)
        self._create(getattr(ctx, "h", None), C.byref(opt), max(int(self.size[0]), 0), max(int(self.size[1]), 0), max(self.layers, 0))

    def _render(self, viewports, *images_and_stream):
        v = np.ascontiguousarray(viewports, dtype=np.uint32)
        check(self._fn("render")(self.h, self.projection, v.ctypes.data_as(C.POINTER(C.c_uint32)), v.size, *images_and_stream))

    def reset(self):
        """Forgets the history: the next frame is the first frame of a new stage."""
        check(self._fn("reset")(self.h))

    def download(self, name: str) -> np.ndarray:
        """A structured array [layers][h][w] (a name of _AXES: one more axis) of "surface", "canonical", "history" and, with record, the
        decision records of _RECORDS."""
        code, dtype = self._RECORDS[name]
        shape = (self.layers, self.size[1], self.size[0])
        if name in self._AXES:
            shape += (int(self.options[self._AXES[name]]),)
        return self._download(code, shape, np.dtype(dtype))


class RestirDiStage(_RestirStage):
    """ReSTIR DI (trhip_restir_di_*, include/trhip.h; written after shader/restir_di.glsl and its two ray generation shaders): per frame
    the canonical kernel (first hit, RIS over light candidates, temporal merge) and the spatial kernel (neighbour merge, shading).
    `options`: restir_di_options(); with record, download() has "candidates", "temporal", "spatial", "final", "sampled"; with the power
    light selection, "light_weights" (float [n_point + n_tri]) and "light_table" (the alias entries in the same order); with record and
    bsdf_candidates > 0, "candidates" has candidates + bsdf_candidates records a pixel and "bsdf_candidates" one record next to each."""

    PREFIX, TIMINGS = "restir_di", _lib.RestirDiTimingsC
    _RECORDS = {"surface": (_lib.RESTIR_DI_SURFACE, _lib.RESTIR_DI_SURFACE_DTYPE), "canonical": (_lib.RESTIR_DI_CANONICAL, _lib.RESTIR_DI_RESERVOIR_DTYPE),
                "history": (_lib.RESTIR_DI_HISTORY, _lib.RESTIR_DI_RESERVOIR_DTYPE), "candidates": (_lib.RESTIR_DI_CANDIDATES, _lib.RESTIR_DI_CANDIDATE_DTYPE),
                "temporal": (_lib.RESTIR_DI_TEMPORAL, _lib.RESTIR_DI_TEMPORAL_DTYPE), "spatial": (_lib.RESTIR_DI_SPATIAL, _lib.RESTIR_DI_SPATIAL_DTYPE),
                "final": (_lib.RESTIR_DI_FINAL, _lib.RESTIR_DI_FINAL_DTYPE), "sampled": (_lib.RESTIR_DI_SAMPLED, _lib.RESTIR_DI_SAMPLED_DTYPE)}
    _AXES = {"candidates": "candidates", "spatial": "spatial_samples"}

    def __init__(self, ctx: Optional[Context], scene_stage: Optional[SceneStage], size, layers=1, options: Optional[dict] = None, projection=0):
        o = self.options = restir_di_options(**(options or {}))
        opt = _lib.RestirDiOptionsC(max(int(o["candidates"]), 0), max(int(o["spatial_samples"]), 0), float(o["search_radius"]), float(o["max_confidence"]),
                                    int(o["temporal_reuse"]), float(o["min_ray_dist"]), int(o["rng_seed"]) & 0xFFFFFFFF, int(o["record"]))
        if int(o["candidates"]) < 0 or int(o["spatial_samples"]) < 0:
            raise TrhipError("RestirDiStage: candidates and spatial_samples are counts")
        visibility, o["visibility"] = o["visibility"], "per-target"
        selection, o["light_selection"] = o["light_selection"], "uniform"
        bsdf_candidates, o["bsdf_candidates"] = o["bsdf_candidates"], 0
        sphere_lights, o["sphere_lights"] = o["sphere_lights"], "point"
        self._create_stage(ctx, scene_stage, size, layers, projection, opt)
        try:
            if sphere_lights != "point":
                self.set_sphere_lights(sphere_lights)
            if bsdf_candidates != 0:
                self.set_bsdf_candidates(bsdf_candidates)
            if visibility != "per-target":
                self.set_visibility(visibility)
            if selection != "uniform":
                self.set_light_selection(selection, o["uniform_fraction"])
        except TrhipError:
            self.close()
            raise

    def set_visibility(self, visibility: str):
        """The visibility mode, "per-target", "shared" or "sampled" (trhip_restir_di_set_visibility); another mode than the history's
        is refused while there is history."""
        check(self._fn("set_visibility")(self.h, _restir_visibility_mode(visibility)))
        self.options["visibility"] = visibility

    def set_light_selection(self, light_selection: str, uniform_fraction: float = 0.1):
        """How a point or triangle light candidate is drawn, "uniform" or "power" (trhip_restir_di_set_light_selection): in proportion to
        the lights' power with the share `uniform_fraction` of the pdf uniform.  "power" builds the table from the scene's lights as
        they are and waits for the device; a change is refused while there is history."""
        check(self._fn("set_light_selection")(self.h, _restir_light_selection_mode(light_selection, uniform_fraction), float(uniform_fraction)))
        self.options["light_selection"], self.options["uniform_fraction"] = light_selection, float(uniform_fraction)

    def set_bsdf_candidates(self, n: int):
        """The candidates a pixel draws from its surface's BSDF behind the light candidates, 0..8 and at most 32 together
        (trhip_restir_di_set_bsdf_candidates): a closest-hit ray each, weighted with the light candidates by the balance heuristic.
        A change is refused while there is history."""
        check(self._fn("set_bsdf_candidates")(self.h, _restir_bsdf_candidates(n, self.options["candidates"])))
        self.options["bsdf_candidates"] = int(n)

    def set_sphere_lights(self, sphere_lights: str):
        """How a point light with a radius is lit, "point" or "area" (trhip_restir_di_set_sphere_lights): as a point, or by samples on
        the sphere, which gives its shadows a penumbra.  Another mode than the history's is refused while there is history."""
        check(self._fn("set_sphere_lights")(self.h, _restir_sphere_lights_mode(sphere_lights)))
        self.options["sphere_lights"] = sphere_lights

    def refresh_light_selection(self) -> bool:
        """Rebuilds the power selection's table after the scene's lights or instances changed (trhip_restir_di_refresh_light_selection);
        allowed while there is history.  True when the table was rebuilt, False when the lights' weights were those it holds (or the
        stage is uniform).  Waits for the device."""
        rebuilt = C.c_uint32(0)
        check(self._fn("refresh_light_selection")(self.h, C.byref(rebuilt)))
        return bool(rebuilt.value)

    def download(self, name: str) -> np.ndarray:
        if name in ("light_weights", "light_table"):
            weights = name == "light_weights"
            code, dtype = (_lib.RESTIR_DI_LIGHT_WEIGHTS, np.float32) if weights else (_lib.RESTIR_DI_LIGHT_TABLE, _lib.RESTIR_DI_LIGHT_TABLE_DTYPE)
            n = len(self.scene_stage.scene.point_lights) + int(self.scene_stage.accel["tri_light_count"])
            # one entry more than the table has: an empty table still has an address to copy to
            return self._download_prefix(code, n, np.dtype(dtype))
        if name in ("candidates", "bsdf_candidates"):      # one record per candidate of either technique
            code, dtype = (_lib.RESTIR_DI_CANDIDATES, _lib.RESTIR_DI_CANDIDATE_DTYPE) if name == "candidates" else (
                _lib.RESTIR_DI_BSDF_CANDIDATES, _lib.RESTIR_DI_BSDF_CANDIDATE_DTYPE)
            per_pixel = int(self.options["candidates"]) + int(self.options["bsdf_candidates"])
            return self._download(code, (self.layers, self.size[1], self.size[0], per_pixel), np.dtype(dtype))
        return super().download(name)

    def _download_prefix(self, code, n, dtype) -> np.ndarray:
        out = np.empty(n + 1, dtype=dtype)
        check(self._fn("download")(self.h, code, out.ctypes.data, n * dtype.itemsize))
        return out[:n]

    def run(self, viewports, out, stream=None):
        """One frame: `out` RGBA32F [len(viewports)][h][w] = contribution * uc_weight + emission of the listed viewports.  History is kept
        per position in the list: with temporal reuse the list stays the same from frame to frame until `reset`."""
        self._render(viewports, _ptr(out), stream)


class RestirDiRenderer(_ViewportFrameRenderer):
    """--renderer=restir-di: the ReSTIR DI stage renders every viewport, the frame is tonemapped - on one stream."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, scene: SceneDesc, size, options: Optional[dict] = None, projection=None,
                 tonemap: Optional[TonemapStage] = None, deformation_motion: Optional[bool] = None):
        super().__init__(ctx, scene_stage, scene, size, tonemap, deformation_motion)
        if projection is None:
            projection = scene.cameras[0].projection if scene.cameras else 0
        self.stage = RestirDiStage(ctx, scene_stage, self.size, self.viewports, options, projection)
        self._animated = bool(scene.animations)

    def render(self, stream=None, tonemap=True):
        if self._animated:      # the lights may have moved with their nodes: a no-op for the uniform selection
            self.stage.refresh_light_selection()
        self.stage.run(np.arange(self.viewports), self.color, stream)
        self._finish(stream, tonemap)

    def reset(self):
        self.stage.reset()

    def timings(self) -> dict:
        return self.stage.timings()

    def close(self):
        self.stage.close()
        super().close()


def restir_gi_options(**kw) -> dict:
    """trhip_restir_gi_options at the command line's defaults (--restir-gi=2,32,16,on), and `bounces` (--restir-gi-bounces=1), which
    the stage applies through trhip_restir_gi_set_bounces."""
    o = dict(spatial_samples=2, search_radius=32.0, max_confidence=16.0, temporal_reuse=True, min_ray_dist=1e-4, rng_seed=0, record=False, bounces=1)
    unknown = set(kw) - set(o)
    if unknown:
        raise AttributeError(f"unknown ReSTIR GI option {sorted(unknown)}")
    o.update(kw)
    return o


class RestirGiStage(_RestirStage):
    """ReSTIR GI (trhip_restir_gi_*, include/trhip.h; csrc/restir_gi.h pins the rule): indirect light by reservoir resampling - per
    frame the initial kernel (first hit, one cosine-hemisphere ray, a light sample at its hit and, with bounces > 1, the path continued
    from there), the temporal kernel (the history merge, no rays) and the spatial kernel (neighbour merge, shading).  `options`:
    restir_gi_options(); with record, download() has "initial", "secondary", "light", "temporal", "spatial", "final" and, with
    bounces > 1, "path" and "path_surface" ([layers][h][w][bounces - 1])."""

    PREFIX, TIMINGS = "restir_gi", _lib.RestirGiTimingsC
    _RECORDS = {"surface": (_lib.RESTIR_GI_SURFACE, _lib.RESTIR_DI_SURFACE_DTYPE), "canonical": (_lib.RESTIR_GI_CANONICAL, _lib.RESTIR_GI_RESERVOIR_DTYPE),
                "history": (_lib.RESTIR_GI_HISTORY, _lib.RESTIR_GI_RESERVOIR_DTYPE), "initial": (_lib.RESTIR_GI_INITIAL, _lib.RESTIR_GI_INITIAL_DTYPE),
                "secondary": (_lib.RESTIR_GI_SECONDARY, _lib.RESTIR_DI_SURFACE_DTYPE), "light": (_lib.RESTIR_GI_LIGHT, _lib.RESTIR_DI_CANDIDATE_DTYPE),
                "temporal": (_lib.RESTIR_GI_TEMPORAL, _lib.RESTIR_DI_TEMPORAL_DTYPE), "spatial": (_lib.RESTIR_GI_SPATIAL, _lib.RESTIR_DI_SPATIAL_DTYPE),
                "final": (_lib.RESTIR_GI_FINAL, _lib.RESTIR_DI_FINAL_DTYPE), "path": (_lib.RESTIR_GI_PATH, _lib.RESTIR_GI_PATH_DTYPE),
                "path_surface": (_lib.RESTIR_GI_PATH_SURFACE, _lib.RESTIR_DI_SURFACE_DTYPE)}
    _AXES = {"spatial": "spatial_samples"}

    def __init__(self, ctx: Optional[Context], scene_stage: Optional[SceneStage], size, layers=1, options: Optional[dict] = None, projection=0):
        o = self.options = restir_gi_options(**(options or {}))
        opt = _lib.RestirGiOptionsC(max(int(o["spatial_samples"]), 0), float(o["search_radius"]), float(o["max_confidence"]), int(o["temporal_reuse"]),
                                    float(o["min_ray_dist"]), int(o["rng_seed"]) & 0xFFFFFFFF, int(o["record"]))
        if int(o["spatial_samples"]) < 0:
            raise TrhipError("RestirGiStage: spatial_samples is a count")
        bounces, o["bounces"] = int(o["bounces"]), 1
        self._create_stage(ctx, scene_stage, size, layers, projection, opt)
        if bounces != 1:
            try:
                self.set_bounces(bounces)
            except TrhipError:
                self.close()
                raise

    def set_bounces(self, bounces: int):
        """The vertices of a sample's path behind the pixel, 1..8 (trhip_restir_gi_set_bounces); refused while there is history."""
        if not 0 <= int(bounces) <= 0xFFFFFFFF:
            raise TrhipError("RestirGiStage: bounces is a count")
        check(self._fn("set_bounces")(self.h, int(bounces)))
        self.options["bounces"] = int(bounces)

    def download(self, name: str) -> np.ndarray:
        if name in ("path", "path_surface"):
            code, dtype = self._RECORDS[name]
            return self._download(code, (self.layers, self.size[1], self.size[0], int(self.options["bounces"]) - 1), np.dtype(dtype))
        return super().download(name)

    def run(self, viewports, in_color, out, stream=None):
        """One frame: `out` RGBA32F [len(viewports)][h][w] = `in_color` + the indirect light of the listed viewports; `in_color` None
        counts as (0, 0, 0, 1), `out` may be `in_color`.  History is kept per position in the list: with temporal reuse the list stays
        the same from frame to frame until `reset`."""
        self._render(viewports, None if in_color is None else _ptr(in_color), _ptr(out), stream)


class RestirGiRenderer(_ViewportFrameRenderer):
    """--renderer=restir-gi: the ReSTIR DI stage renders the direct light of every viewport, the ReSTIR GI stage adds indirect light to it
    (`bounces` of its options: how far a sample's path goes on), the frame is tonemapped - on one stream.  `di_options`:
    restir_di_options(); `options`: restir_gi_options()."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, scene: SceneDesc, size, options: Optional[dict] = None, di_options: Optional[dict] = None,
                 projection=None, tonemap: Optional[TonemapStage] = None, deformation_motion: Optional[bool] = None):
        super().__init__(ctx, scene_stage, scene, size, tonemap, deformation_motion)
        if projection is None:
            projection = scene.cameras[0].projection if scene.cameras else 0
        self.direct = RestirDiStage(ctx, scene_stage, self.size, self.viewports, di_options, projection)
        self.stage = RestirGiStage(ctx, scene_stage, self.size, self.viewports, options, projection)
        self._animated = bool(scene.animations)

    def render(self, stream=None, tonemap=True):
        v = np.arange(self.viewports)
        if self._animated:      # as RestirDiRenderer
            self.direct.refresh_light_selection()
        self.direct.run(v, self.color, stream)
        self.stage.run(v, self.color, self.color, stream)
        self._finish(stream, tonemap)

    def reset(self):
        self.direct.reset()
        self.stage.reset()

    def timings(self) -> dict:
        return {"direct": self.direct.timings(), "indirect": self.stage.timings()}

    def close(self):
        self.direct.close()
        self.stage.close()
        super().close()


@dataclass(frozen=True)
class PostProcessingPlan:
    """What plan_post_processing decides about the chain behind the path tracer; needs no device."""
    stages: tuple           # the chain in order, out of POST_STAGES
    targets: tuple          # set_gbuffer_spec: the G-buffer entries the path tracer writes besides colour
    frame_order: bool       # a stage's history (or the G-buffer the slots share) is one chain over all frame slots: the chain runs in frame order on the default stream
    fused_tonemap: bool     # nothing sits between the path tracer and the tonemap stage: the path tracer may write the display image itself
    output_layers: int      # layers of the display image
    viewports: int          # the viewports of the scene (a Looking Glass rig brings its own count)
    viewport_list: Optional[tuple]      # a sparse light field: the viewports that are path traced, as compact layers in this order
    denoiser: Optional[str]
    temporal_ratio: float
    taa_length: int


POST_STAGES = ("bmfr", "temporal", "gbuffer+spatial", "tonemap", "taa", "looking_glass")


def plan_post_processing(*, denoiser=None, spatial_reprojection=None, temporal_reprojection=0.0, taa=0, looking_glass=None, device_count=1,
                         shard="pixels", viewports=1, viewports_per_device=None, accumulate=False, frames_per_launch=1, projection=0,
                         path_tracer=True) -> PostProcessingPlan:
    """The policy of the post-processing chain (the reference's post_processing_renderer, src/post_processing_renderer.cc:53-106) as one pure
    function of the chain's options and the facts of the renderer they depend on: which stages run and in which order, what the path tracer
    has to write for them, whether the chain is bound to frame order and whether the tonemap may still be fused - or a ValueError that says
    which combination is not built.  `viewports_per_device`: the viewports of this device's share (a view shard), default all."""
    world_size = device_count
    if looking_glass is not None:
        if world_size > 1:
            raise ValueError(f"looking_glass with a {shard} distribution of count {world_size} > 1: the composition stage reads every view of the light "
                             "field on one device, the views would have to be gathered first, which is not built; use one device")
        if viewports not in (1, looking_glass.viewports):
            raise ValueError(f"looking_glass: the rig has {looking_glass.viewports} views, not viewports={viewports}")
        if frames_per_launch > 1:
            raise ValueError("looking_glass: a composed frame is one frame: frames_per_launch must be 1")
        if projection != 0:
            raise ValueError("looking_glass: the rig's cameras are perspective cameras (options.projection must be 0)")
        viewports = viewports_per_device = looking_glass.viewports
    if denoiser not in (None, "none", "bmfr"):
        raise ValueError(f"denoiser {denoiser!r}: only \"bmfr\" is built" + (" (svgf is not built)" if denoiser == "svgf" else ""))
    denoiser = None if denoiser == "none" else denoiser
    if denoiser is not None:
        if world_size > 1 and shard != "views":
            raise ValueError(f"denoiser with a {shard} distribution of count {world_size} > 1: the feature targets (diffuse, albedo, normal, pos, "
                             "instance id, screen motion) would have to be gathered and stitched like colour, which is not built; "
                             "use one device or shard=\"views\"")
        if accumulate or frames_per_launch > 1:
            raise ValueError("a denoised frame is a fresh frame: accumulate must be False and frames_per_launch 1")
        if not path_tracer:
            raise ValueError("the denoiser reads the path tracer's demodulated diffuse target: stage_cls must be PathTracerStage")
    temporal_reprojection = float(temporal_reprojection or 0.0)
    if not (0.0 <= temporal_reprojection < 1.0):
        raise ValueError(f"temporal_reprojection {temporal_reprojection!r}: the ratio must be in [0, 1) (0 = off)")
    if spatial_reprojection is not None:
        spatial_reprojection = check_viewport_list(spatial_reprojection, viewports)
    spatial, temporal = spatial_reprojection is not None, temporal_reprojection > 0.0
    if spatial or temporal:
        which = "spatial_reprojection" if spatial else "temporal_reprojection"
        if world_size > 1:
            raise ValueError(f"{which} with a {shard} distribution of count {world_size} > 1: the stages read the G-buffer of whole viewports on one "
                             "device, gathering it from several is not built; use one device")
        if denoiser is not None:
            raise ValueError(f"{which} together with denoiser={denoiser!r}: a chain of reprojection and a denoiser is not built")
        if frames_per_launch > 1:
            raise ValueError(f"{which}: a reprojected frame is one frame: frames_per_launch must be 1")
        if temporal and accumulate:
            raise ValueError("temporal_reprojection blends the previous frame into a fresh frame: accumulate must be False")
    taa = int(taa or 0)
    if taa < 0:
        raise ValueError(f"taa {taa!r}: the length of the jitter sequence must be positive (0 = off)")
    per_device = viewports if viewports_per_device is None else viewports_per_device
    if taa:
        if world_size > 1 and shard != "views":
            raise ValueError(f"taa with a {shard} distribution of count {world_size} > 1: the stage reads screen motion, pos and instance id of whole "
                             "viewports on one device, gathering them from several is not built; use one device or shard=\"views\"")
        if world_size > 1 and shard == "views" and per_device > 1:
            raise ValueError("taa with shard=\"views\": more than one viewport per device is not built (the stage reads consecutive cameras)")
        if accumulate:
            raise ValueError("taa blends a fresh, jittered frame into its history: accumulate must be False")
        if frames_per_launch > 1:
            raise ValueError("taa: an antialiased frame is one frame (the jitter steps between frames): frames_per_launch must be 1")
        if spatial or temporal:
            raise ValueError("taa together with spatial_reprojection / temporal_reprojection: a chain of reprojection and taa is not built")
        if projection == 2:
            raise ValueError("taa with equirectangular cameras: the stage projects a miss's ray direction with the previous camera's view_proj, "
                             "which an equirectangular camera does not have")
        if not path_tracer:
            raise ValueError("taa reads the path tracer's screen_motion target: stage_cls must be PathTracerStage")
    on = dict(zip(POST_STAGES, (denoiser == "bmfr", temporal, spatial, True, bool(taa), looking_glass is not None)))
    if on["bmfr"]:
        targets = tuple(n for n in BmfrStage.FEATURES if n != "color")
    elif taa:
        targets = ("screen_motion", "pos", "instance_id")
    elif spatial or temporal:
        targets = ("normal", "pos", "instance_id") + (("screen_motion",) if temporal else ())
    else:
        targets = ()
    return PostProcessingPlan(stages=tuple(n for n in POST_STAGES if on[n]), targets=targets,
                              frame_order=on["bmfr"] or temporal or spatial or bool(taa),
                              fused_tonemap=world_size == 1 and path_tracer and not any(on[n] for n in POST_STAGES if n != "tonemap"),
                              output_layers=viewports if spatial else per_device * frames_per_launch, viewports=viewports,
                              viewport_list=tuple(spatial_reprojection) if spatial else None, denoiser=denoiser,
                              temporal_ratio=temporal_reprojection, taa_length=taa)


class PostProcessingRenderer:
    """post_processing_renderer (src/post_processing_renderer.{hh,cc}): the owner of the chain behind the path tracer.  It builds the stages of
    a PostProcessingPlan and the images that belong to the chain rather than to a frame slot's path tracing (the TAA input, the destination
    G-buffer, the composed images), keeps the previous-camera record and the jitter step, and runs the chain for a slot on a stream.  The
    renderer in front of it asks four things: alloc_targets (per slot), frame_order, plan.fused_tonemap, run.  The owner holds no reference to
    that renderer: both are released by reference count, in the order their owner drops them.

    `layers`: the layers the path tracer renders on this device (0: an empty view shard, no stage is built)."""

    def __init__(self, ctx: Context, scene_stage: SceneStage, plan: PostProcessingPlan, size, layers, options: PtOptionsC, torch=None,
                 tonemap: Optional[dict] = None, denoiser_settings=_lib.BMFR_DIFFUSE_ONLY, taa_edge_dilation=True, taa_anti_shimmer=False,
                 looking_glass=None, base_camera=0):
        self.ctx, self.ss, self.plan, self.size, self.layers, self.torch = ctx, scene_stage, plan, (int(size[0]), int(size[1])), layers, torch
        self.tonemap = TonemapStage(ctx, **(tonemap or {}))
        self.bmfr = self.temporal = self.spatial = self.gbuffer = self.destination_targets = self.taa = self.taa_input = self.lkg = None
        self._last_cameras = None        # the cameras the last frame was rendered with (a history chain's camera_pair.previous)
        if layers <= 0:
            return
        if "bmfr" in plan.stages:
            self.bmfr = BmfrStage(ctx, self.size, layers, denoiser_settings)
        if "temporal" in plan.stages:
            self.temporal = TemporalReprojectionStage(ctx, self.size, layers, plan.temporal_ratio)
        if "gbuffer+spatial" in plan.stages:
            self.spatial = SpatialReprojectionStage(ctx, self.size, plan.viewports, plan.viewport_list)
            self.gbuffer = GbufferStage(ctx, scene_stage, self.size, options.projection, options.min_ray_dist)
            self.destination_targets = self.gbuffer.alloc_targets(len(self.spatial.destinations))
        if "taa" in plan.stages:
            self._jitter(scene_stage.scene)
            # a view shard's stage reads its first camera (`base_camera`); TaaStage strides by one
            self.taa = TaaStage(ctx, self.size, layers, dict(alpha=1.0 / plan.taa_length, gamma=self.tonemap.info.gamma, edge_dilation=taa_edge_dilation,
                                                             anti_shimmer=taa_anti_shimmer, base_camera_index=base_camera, projection=options.projection))
            self.taa_input = self.alloc_display(layers)      # the tonemap stage's output; the stage writes the display image
        if "looking_glass" in plan.stages:
            self.lkg = LookingGlassStage(ctx, self.size, looking_glass.calibration.size,
                                         looking_glass.calibration.stage_options(plan.output_layers, looking_glass.record_view_indices))

    def _jitter(self, scene):
        """Every camera of the scene gets the TAA jitter sequence; the first frame's camera_pair.previous: the cameras before their first step."""
        from .scene import get_camera_jitter_sequence
        seq = get_camera_jitter_sequence(self.plan.taa_length, self.size)
        for cam in scene.cameras:
            cam.set_jitter(seq)
        self.ss.update_cameras(scene.cameras)
        self._last_cameras = self.ss.camera_data.copy()

    @property
    def frame_order(self) -> bool:
        return self.plan.frame_order and self.layers > 0

    def alloc_display(self, layers):
        """A display-space image of `layers` layers (a torch tensor when the renderer exchanges frames through torch, `torch` = the module)."""
        w, h = self.size
        if self.torch is not None:
            return self.torch.empty((layers, h, w, 4), dtype=self.torch.float32, device=f"cuda:{self.ctx.hip_device}")
        return self.ctx.alloc(layers * w * h * 16)

    def alloc_targets(self, tw, th):
        """The G-buffer entries of one frame slot next to its colour target (None: the path tracer writes colour only)."""
        if not self.plan.targets or self.layers <= 0:
            return None
        return {n: self.ctx.alloc(self.layers * tw * th * PathTracerStage.TARGETS[n][0] * 4).zero() for n in self.plan.targets}

    def set_scene(self, scene):
        """A new scene is on the device: the histories start over."""
        for stage in (self.bmfr, self.temporal):
            if stage is not None:
                stage.reset_history()
                self._last_cameras = None
        if self.taa is not None:
            self._jitter(scene)
            self.taa.reset_history()

    def begin_frame(self, wait=None):
        """In front of a frame's path tracing: the jitter steps, and the device's previous cameras become the cameras of the frame before this
        one.  `wait`: called before the device's cameras change while frames are in flight (they read the cameras they were enqueued with)."""
        if self.taa is not None:
            # scene::update (src/scene.cc:228): every camera steps its jitter before it is packed
            if wait is not None:
                wait()
            cams = self.ss.scene.cameras
            for cam in cams:
                cam.step_jitter()
            self.ss.update_cameras(cams)
        if self.bmfr is not None or self.temporal is not None or self.taa is not None:
            cameras = self.ss.camera_data
            prev = cameras if self._last_cameras is None else self._last_cameras
            on_device = self.ss.previous_camera_data
            if on_device is None or prev.tobytes() != on_device.tobytes():
                if wait is not None:
                    wait()
                self.ss.set_previous_camera_data(prev)
            self._last_cameras = cameras.copy()

    def run(self, slot, stream=None, tonemap=True):
        """The chain on one frame slot's images (src/post_processing_renderer.cc:53-106), in the order of POST_STAGES."""
        w, h = self.size
        if self.layers <= 0:
            return
        if self.bmfr is not None:
            self.bmfr.run(dict(slot.features, color=slot.color), slot.frame, stream)
        if self.temporal is not None:
            self.temporal.run(dict(slot.features, color=slot.color), stream)
        if self.spatial is not None:
            self.gbuffer.run(self.spatial.destinations, self.destination_targets, stream)
            self.spatial.run({n: (slot.color if n == "color" else slot.features[n]) for n in SpatialReprojectionStage.SOURCES},
                             self.destination_targets, slot.full, stream)
        if not tonemap:
            return
        if slot.display is None:
            slot.display = self.alloc_display(self.plan.output_layers)
        self.tonemap.run(slot.full if self.spatial is not None else slot.color, slot.display if self.taa is None else self.taa_input, w, h,
                         self.plan.output_layers, stream)
        if self.taa is not None:
            self.taa.run(dict(src=self.taa_input, dst=slot.display, screen_motion=slot.features["screen_motion"], pos=slot.features["pos"],
                              instance_id=slot.features["instance_id"]), stream)
        if self.lkg is not None:
            if slot.composed is None:
                ow, oh = self.lkg.out_size
                slot.composed, slot.composed8 = self.ctx.alloc(ow * oh * 16), self.ctx.alloc(ow * oh * 4)
            self.lkg.run(slot.display, slot.composed, slot.composed8, stream)

    def close(self):
        if self.taa is not None and self.ss.scene is not None:
            for cam in self.ss.scene.cameras:      # the caller's cameras get their jitter from this renderer: it goes with it
                cam.set_jitter([])
        for stage in (self.bmfr, self.temporal, self.spatial, self.taa, self.lkg):
            if stage is not None:
                stage.close()


class _FrameSlot:
    """What one frame in flight owns: its stage (path buffers, counters), its images and the stream it is ordered on."""

    def __init__(self):
        self.pt = None
        self.runs = None         # a viewport list: [(stage, first layer, layers)], one stage per arithmetic run of the list (self.pt is the first)
        self.full = None         # spatial reprojection: the colour of every viewport in natural order (self.color holds the sources)
        self.features = None     # denoiser: the gbuffer targets next to the colour target
        self.color = None
        self.display = None
        self.composed = self.composed8 = None      # a Looking Glass output: the panel's image in fp32 and in 8 bits
        self.stream = None
        self.frame = 0           # frame counter of the slot's last frame
        self.fused_info = None


class RtRenderer:
    """rt_renderer<path_tracer_stage> for one rank of an N-GPU job.

    Each rank renders its share (`get_device_distribution_params`) into its own target; the display
    rank (0) owns the full-size image.  `render()` = scene update -> ray tracer -> transfer -> stitch ->
    tonemap (src/rt_renderer.cc:84-133).  Transfers use torch.distributed (backend "nccl" = RCCL over
    xGMI): non-display ranks `send` their partial, the display rank `recv`s it straight into device
    memory and runs the stitch kernel - replacing the GPU->pinned host->GPU copies of
    src/device_transfer.cc:21-347.

    `frames_in_flight` (MAX_FRAMES_IN_FLIGHT = 2 in the reference, src/context.hh:26): that many frame slots, each with its
    own stage, images and stream; frame i goes to slot i mod F and starts while the previous frames are still running, so
    the tails of one frame's kernels are filled by the next frame.  The exchange between ranks, the stitch and the tonemap
    of a multi-GPU frame stay on the default stream (= torch's current stream, where RCCL orders itself); only the path
    tracing runs ahead on the slot streams.
    """

    def __init__(self, ctx: Context, scene: SceneDesc, options: PtOptionsC, size, strategy=DISTRIBUTION_SCANLINE,
                 rank=0, world_size=1, viewports=1, tonemap: Optional[dict] = None, accumulate=False, use_torch=None,
                 shard="pixels", frames_in_flight=1, stage_cls=None, exchange=None, frames_per_launch=1, as_strategy=0, dynamic=None,
                 deformation_motion=False,
                 denoiser=None, denoiser_settings=_lib.BMFR_DIFFUSE_ONLY, spatial_reprojection=None, temporal_reprojection=0.0,
                 taa=0, taa_edge_dilation=True, taa_anti_shimmer=False, looking_glass=None):
        """`shard`: what the ranks divide among themselves - "pixels" (the reference's distribution strategies, partial frames
        stitched on rank 0), "views" (viewport v on rank v mod N; nothing is exchanged before output) or "samples" (every
        rank renders samples_per_pixel / N samples of every pixel; one reduce to rank 0).  SURVEY.md section 8(e).
        `exchange`: what carries the partial frames of a pixel-sharded job to rank 0 - None = torch.distributed (RCCL), or a
        transfer.LocalExchange shared by the ranks of one process (device-to-device copies on the default stream).
        `frames_per_launch`: B > 1 makes every render() call B consecutive frames (trhip_pt_set_frame_batch): the images grow B
        layer groups, frame-major, and everything after the path tracing - exchange, stitch, tonemap - handles the B frames in
        one go.  For frames that do not accumulate; what the ranks of a pixel-sharded job use, whose launches are small.
        `as_strategy`, `dynamic`: the acceleration-structure strategy and dynamic marks of the scene stage (SceneStage; the C++
        rt_renderer::options::scene).  `deformation_motion`: the scene stage's switch (SceneStage.set_deformation_motion): its animate()
        and pose() then latch the positions of skinned and morphed meshes, and screen motion follows their deformation.
        `denoiser`: None, or "bmfr" (the reference's --denoiser=bmfr, src/post_processing_renderer.cc:53-106): the path tracer renders the
        gbuffer entries the BMFR stage reads next to the colour target, every frame is a fresh frame of samples_per_pixel samples (the
        sample counter keeps counting), and post_process runs the stage before the tonemap stage (which is then a stage of its own: the
        fused tonemap is off).  The stage gets last frame's cameras as camera_pair.previous.  With frames in flight its history stays
        one chain: it runs in frame order on the default stream.  `denoiser_settings`: _lib.BMFR_DIFFUSE_ONLY or BMFR_DIFFUSE_SPECULAR.
        `spatial_reprojection`: None, or the list of active viewports of a sparse light field (the reference's --spatial-reprojection=i,j,...):
        only these are path traced, as compact layers in list order with their own cameras and RNG streams; the others get a first-hit
        G-buffer pass and are filled by SpatialReprojectionStage.  color / display then hold every viewport in natural order, the fused
        tonemap is off, and with `accumulate` the sources are the accumulators and the full image is rewritten every frame.
        `temporal_reprojection`: 0, or the ratio of TemporalReprojectionStage (--temporal-reprojection=r), which runs on the path-traced layers
        in front of the spatial stage; its history is one chain in frame order, like the denoiser's.
        `taa`: 0, or the length N of the camera jitter sequence of temporal antialiasing (the reference's --taa=N): every camera of the scene
        gets the Halton sequence of get_camera_jitter_sequence(N, size) and steps it once per frame before it is packed
        (scene::update), the path tracer renders screen_motion, pos and instance_id next to the colour target, and TaaStage (alpha =
        1 / N, gamma = the tonemap stage's; `taa_edge_dilation`, `taa_anti_shimmer`: the reference's defaults) runs after the tonemap
        stage, in frame order on the default stream like the denoiser's history chain; the fused tonemap is off.  Every frame is a
        fresh frame.  With denoiser="bmfr" or without.
        `looking_glass`: None, or a looking_glass.LookingGlassOutput (the reference's --display=looking-glass with --lkg-calibration and
        --lkg-params): the scene's cameras are replaced by the rig of looking_glass::setup_cameras under the scene's first camera, `size` is
        the size of one view, and LookingGlassStage runs at the end of post_process, behind tonemap and TAA: download("composed") is the
        panel's image in fp32, download("composed8") in the reference's 8 bits.  The caller's scene stays rigged after close() (scene.cameras
        are the rig, scene.camera_rig its local transforms).  One device; the fused tonemap is off.  With
        spatial_reprojection / temporal_reprojection, denoiser="bmfr", taa or an animated scene."""
        if shard not in ("pixels", "views", "samples"):
            raise ValueError("shard must be pixels, views or samples")
        path_tracer = stage_cls is None or stage_cls is PathTracerStage
        mine = max(viewports - rank + world_size - 1, 0) // world_size if (world_size > 1 and shard == "views") else viewports
        plan = plan_post_processing(denoiser=denoiser, spatial_reprojection=spatial_reprojection, temporal_reprojection=temporal_reprojection, taa=taa,
                                    looking_glass=looking_glass, device_count=world_size, shard=shard, viewports=viewports, viewports_per_device=mine,
                                    accumulate=accumulate, frames_per_launch=frames_per_launch, projection=getattr(options, "projection", 0), path_tracer=path_tracer)
        self.plan, viewports = plan, plan.viewports
        if frames_in_flight < 1:
            raise ValueError("frames_in_flight must be >= 1")
        if frames_in_flight > 1 and accumulate:
            raise ValueError("accumulating frames depend on each other: frames_in_flight must be 1")
        if frames_per_launch < 1 or (frames_per_launch > 1 and (accumulate or shard != "pixels")):
            raise ValueError("frames_per_launch > 1 batches independent frames of a pixel-sharded (or single-device) renderer")
        if shard == "samples" and accumulate and world_size > 1:
            # the reduce sums the ranks' running means into rank 0's target in place: a second accumulated frame would blend
            # new samples into an already reduced mean
            raise ValueError("sample sharding reduces into the colour target: it cannot accumulate across frames")
        self.ctx, self.opt, self.size = ctx, options, (int(size[0]), int(size[1]))
        self.rank, self.world_size = rank, world_size
        self.exchange = exchange
        if exchange is not None:
            if shard != "pixels":
                raise ValueError("an in-process exchange carries pixel shards only")
            exchange.attach(rank, ctx)
            use_torch = False if use_torch is None else use_torch
        self.shard = shard if world_size > 1 else "pixels"
        self.total_viewports = viewports
        if self.shard == "views":
            from .transfer import shard_viewports
            viewports = len(shard_viewports(viewports, rank, world_size))
        if plan.viewport_list is not None:
            viewports = len(plan.viewport_list)             # the path tracer's layers: the active viewports, compact, in list order
        self.frames_per_launch = frames_per_launch
        self.frame_viewports = viewports                    # layers of one frame
        viewports = viewports * frames_per_launch           # layers of one launch: every buffer, transfer, stitch and tonemap below
        self.viewports = viewports
        self.strategy = DISTRIBUTION_DUPLICATE if (world_size == 1 or self.shard != "pixels") else strategy   # src/tauray.cc:519-521
        self.accumulate = accumulate
        self.looking_glass = looking_glass
        if looking_glass is not None:       # looking_glass::setup_cameras, before the scene goes to the device
            from .looking_glass import looking_glass_cameras
            looking_glass_cameras(scene, looking_glass.viewports, looking_glass.midplane, looking_glass.depth, looking_glass.relative_dist,
                                  looking_glass.calibration)
        self.scene_update = SceneStage(ctx, scene, as_strategy=as_strategy, dynamic=dynamic, deformation_motion=deformation_motion)
        if self.shard == "pixels":
            workloads = [1.0 / world_size] * world_size
            self.dists = self._device_dists(workloads)
        else:       # every rank owns full-size images
            self.dists = [DistributionParams(self.size, DISTRIBUTION_DUPLICATE, 0, 1, True)] * world_size
        self.dist = self.dists[rank]
        if self.shard == "samples":
            if options.samples_per_pixel % world_size or (options.samples_per_pixel // world_size) % options.samples_per_pass:
                raise ValueError("sample sharding needs samples_per_pixel divisible by the device count (and the share by samples_per_pass)")
            options = copy_options(options, samples_per_pixel=options.samples_per_pixel // world_size)
            self.opt = options
        tw, th = get_distribution_target_size(self.dist)
        self.target_size = (tw, th)
        self.use_torch = (world_size > 1) if use_torch is None else use_torch
        self._torch = None
        if self.use_torch:
            import torch
            self._torch = torch
        self.frames_in_flight = frames_in_flight
        self.output_viewports = plan.output_layers      # layers of color / display
        self.post = PostProcessingRenderer(ctx, self.scene_update, plan, self.size, viewports, options, self._torch, tonemap, denoiser_settings,
                                           taa_edge_dilation, taa_anti_shimmer, looking_glass, base_camera=rank if self.shard == "views" else 0)
        self.tonemap = self.post.tonemap
        # rt_renderer on one device has nothing between path_tracer_stage and tonemap_stage: the stage writes the display image itself
        # (trhip_pt_set_fused_tonemap: the same bits without the second pass over the frame); TRHIP_FUSED_TONEMAP=0 keeps the stage
        self.fused_tonemap = (plan.fused_tonemap and viewports > 0 and hasattr(_lib.lib(), "trhip_pt_set_fused_tonemap")
                              and os.environ.get("TRHIP_FUSED_TONEMAP", "1") != "0")
        self.slots = []
        for k in range(frames_in_flight):
            slot = _FrameSlot()
            slot.pt = (stage_cls or PathTracerStage)(ctx, self.scene_update, options, self.dist)   # rt_renderer<Pipeline>: path_tracer_stage or direct_stage
            if plan.viewport_list is not None:
                # the list as arithmetic runs, one stage per run (usually one): layer l shows viewport list[l], its camera and its RNG stream
                slot.runs, first = [], 0
                for base, stride, count in viewport_runs(plan.viewport_list):
                    stage = slot.pt if not slot.runs else (stage_cls or PathTracerStage)(ctx, self.scene_update, options, self.dist)
                    stage.set_shard(viewport_base=base, viewport_stride=stride)
                    slot.runs.append((stage, first, count))
                    first += count
            if self.shard == "views":
                slot.pt.set_shard(viewport_base=rank, viewport_stride=world_size)
            elif self.shard == "samples":
                slot.pt.set_shard(sample_base=rank, sample_stride=world_size)
            if frames_per_launch > 1:
                slot.pt.set_frame_batch(frames_per_launch)
            if frames_in_flight > 1:
                slot.pt.set_frame_slots(frames_in_flight)    # the frames in flight fill the chip between them: the stage picks one lane (two with two slots)
                slot.stream = ctx.create_stream()
            slot.color = self._alloc_color(viewports, tw, th)
            slot.features = self.post.alloc_targets(tw, th)
            if plan.viewport_list is not None:
                slot.full = self._alloc_color(self.output_viewports, tw, th)
            if self.fused_tonemap:
                slot.display = self._alloc_display(viewports)
                slot.fused_info = None       # what the stage was last told (bytes of the tonemap info), None = off
            self.slots.append(slot)
        self.current = self.slots[0]
        self.stitch = StitchStage(ctx, self.size) if (world_size > 1 and self.shard == "pixels") else None
        self.all_views = None
        self.recv_buffers = {}
        self.accumulated_frames = 0
        self.frame_index = 0

    def __getattr__(self, name):
        """What the owner of the chain holds - its stages and the chain's images - reads on the renderer under the same name, as it did
        when the renderer held them itself (r.taa is r.post.taa)."""
        post = self.__dict__.get("post")
        if post is not None and not name.startswith("_") and name in vars(post):
            return getattr(post, name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    # the stage / images of the most recent frame (the only ones there are with frames_in_flight = 1)
    @property
    def ray_tracer(self) -> PathTracerStage:
        return self.current.pt

    @property
    def color(self):
        return self.current.full if self.plan.viewport_list is not None else self.current.color

    def _stages(self, slot):
        """The path tracer stages of a slot: one, or one per arithmetic run of the viewport list."""
        return [slot.pt] if slot.runs is None else [stage for stage, _, _ in slot.runs]

    @property
    def display(self):
        return self.current.display

    def _alloc_color(self, viewports, tw, th):
        if self.use_torch:
            return self._torch.zeros((viewports, th, tw, 4), dtype=self._torch.float32, device=f"cuda:{self.ctx.hip_device}")
        return self.ctx.alloc(max(viewports * tw * th, 1) * 16).zero()

    def _alloc_display(self, viewports):
        return self.post.alloc_display(viewports)

    def _device_dists(self, ratios) -> List[DistributionParams]:
        out, cumulative = [], 0.0
        for i in range(self.world_size):
            ratio = min(max(ratios[i], 0.0), 1.0 - cumulative)
            out.append(get_device_distribution_params(self.size, self.strategy, cumulative, ratio, i, self.world_size, i == 0))
            cumulative += ratio
        return out

    def set_scene(self, scene: SceneDesc):
        self.sync()
        if self.looking_glass is not None:
            from .looking_glass import looking_glass_cameras
            lg = self.looking_glass
            looking_glass_cameras(scene, lg.viewports, lg.midplane, lg.depth, lg.relative_dist, lg.calibration)
        self.scene_update.set_scene(scene)
        self.post.set_scene(scene)

    def program(self) -> dict:
        """The shading program of this rank's stage (PathTracerStage.program)."""
        return self.slots[0].pt.program()

    def check_same_program(self, allgather=None):
        """All ranks of a job render with the same shading program, or none renders: the reference compiles one pipeline per stage from the
        options and every device gets it (src/path_tracer_stage.cc:30-116).  Here a rank whose run-time compilation failed ("renders with the
        general kernels and says so"), that runs under TRHIP_SPECIALIZE=0 or loads another build of libtrhip.so would shade its strips with
        other kernels - at the default arithmetic another implementation inside Vulkan's accuracy, i.e. strips that differ from their
        neighbours' in the last bits.  `allgather(bytes) -> [bytes of rank 0, ...]`: the job's transport for small blobs (the one
        comm.Ipc takes); default: torch.distributed.all_gather_object when a process group exists.  Every rank calls this before the first
        frame (bench.py, tests/test_multi_rank_gloo.py); raises RuntimeError on every rank, naming both programs."""
        if self.world_size == 1:
            return self.program()
        mine = self.program()
        blob = mine["identity"].to_bytes(8, "little") + mine["key"].encode()
        if allgather is None:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError("check_same_program: no transport (pass allgather, or initialise torch.distributed)")
            every = [None] * self.world_size
            dist.all_gather_object(every, blob)
        else:
            every = allgather(blob)
        for r, b in enumerate(every):
            if b[:8] != blob[:8]:
                raise RuntimeError(f"the ranks of this job would render with different shading programs: rank {self.rank} {{{mine['key']}}} but rank {r} "
                                   f"{{{b[8:].decode(errors='replace')}}} (same libtrhip.so, kernel cache and TRHIP_* environment on every rank?)")
        return mine

    def sync(self):
        """Waits for every frame in flight.  An exchange that can tell that a frame is incomplete (the copy-engine exchange: a device-side
        wait for a peer that gave up) says so here, before anybody looks at the frame."""
        for slot in self.slots:
            if slot.stream is not None:
                self.ctx.sync(slot.stream)
        self.ctx.sync()
        if self.exchange is not None and hasattr(self.exchange, "check"):
            self.exchange.check()

    def reset_accumulation(self, reset_sample_counter=False):
        for slot in self.slots:
            for pt in self._stages(slot):
                pt.reset_accumulated_samples()
                if reset_sample_counter:
                    pt.reset_sample_counter()
        if reset_sample_counter:
            self.frame_index = 0
        self.accumulated_frames = 0

    def set_profiling(self, count_work=False, detailed_timing=False):
        for slot in self.slots:
            for pt in self._stages(slot):
                pt.set_profiling(count_work, detailed_timing)

    def reset_counters(self):
        self.sync()
        for slot in self.slots:
            for pt in self._stages(slot):
                pt.reset_counters()

    def counters(self) -> dict:
        """Work counters summed over the frame slots."""
        self.sync()
        total = {}
        for slot in self.slots:
            for pt in self._stages(slot):
                for k, v in pt.counters().items():
                    total[k] = max(total.get(k, 0), v) if k == "stack_overflows" else total.get(k, 0) + v
        return total

    def timings(self) -> dict:
        self.sync()
        total = {}
        for slot in self.slots:
            for pt in self._stages(slot):
                for k, v in pt.timings().items():
                    total[k] = total.get(k, 0) + v
        return total

    def phase_counters(self) -> dict:
        self.sync()
        total = {}
        for slot in self.slots:
            for k, v in slot.pt.phase_counters().items():
                total[k] = [a + b for a, b in zip(total[k], v)] if (k in total and isinstance(v, list)) else (total.get(k, 0) + v if not isinstance(v, list) else v)
        return total

    def path_tracing_ms(self) -> float:
        """The "path tracing" timer the load balancer reads (src/load_balancer.cc:17,25): the last frame of every slot, averaged.
        Waits for the slots."""
        self.sync()
        t = [sum(pt.timings()["path_tracing_ms"] for pt in self._stages(slot)) for slot in self.slots]
        return sum(t) / len(t)

    def set_device_workloads(self, ratios):
        """rt_renderer::set_device_workloads (src/rt_renderer.cc:135-183): only for shuffled strips."""
        if self.strategy in (DISTRIBUTION_SCANLINE, DISTRIBUTION_DUPLICATE):
            return
        self.sync()
        self.dists = self._device_dists(ratios)
        self.dist = self.dists[self.rank]
        new_size = get_distribution_target_size(self.dist)
        for slot in self.slots:
            slot.pt.reset_distribution_params(self.dist)
            if self.rank != 0:
                slot.pt.reset_accumulated_samples()
                if new_size != self.target_size:
                    # A non-primary target has the size of the share (the partial frame that travels is the whole image):
                    # a new share is a new image.  The reference allocates get_distribution_target_max_size once instead
                    # (src/rt_renderer.cc init_resources); either way the kernels are bounded by the allocated size.
                    slot.color = self._alloc_color(self.viewports, *new_size)
        self.target_size = new_size
        self.recv_buffers.pop("ops", None)      # the display rank's receive list is rebuilt for the new shapes
        if self.accumulate and self.stitch is not None:
            # the other devices start over with one sample: blend it into what has accumulated (src/rt_renderer.cc:176-181)
            self.stitch.set_blend_ratio(1.0 / (self.accumulated_frames + 1))

    def _sync_fused_tonemap(self, slot, want: bool):
        """The stage's copy of the tonemap parameters follows self.tonemap.info: an edit of exposure / operator / gamma between frames
        takes effect on the next frame, as it does with the tonemap stage of a multi-device renderer; render(tonemap=False) switches
        the display write off for that frame."""
        now = bytes(self.tonemap.info) if want else None
        if now != slot.fused_info:
            slot.pt.set_fused_tonemap(slot.display if want else None, self.tonemap.info if want else None)
            slot.fused_info = now

    def render_partial(self, stream=None, tonemap=True):
        """The path-tracing part of the next frame on its slot (`stream` overrides the slot's stream)."""
        slot = self.slots[(self.frame_index // self.frames_per_launch) % self.frames_in_flight]
        self.current = slot
        if self.fused_tonemap:
            self._sync_fused_tonemap(slot, tonemap)
        for pt in self._stages(slot):
            if not self.accumulate:
                pt.reset_accumulated_samples()
            if self.frames_in_flight > 1 or self.frames_per_launch > 1:
                pt.set_frame_counter(self.frame_index)       # one stage per slot: slot k renders frames k, k + F, ... (B at a time)
        slot.frame = self.frame_index
        self.frame_index += self.frames_per_launch
        if self.viewports > 0:      # a view shard can be empty (more devices than views)
            self.post.begin_frame(self.sync if self.frames_in_flight > 1 else None)
            st = stream if stream is not None else slot.stream
            if slot.runs is not None:
                tw, th = self.target_size
                for pt, first, count in slot.runs:
                    pt.run_targets({n: _LayerView(b, first * tw * th * PathTracerStage.TARGETS[n][0] * 4)
                                    for n, b in dict(slot.features, color=slot.color).items()}, count, st)
            elif slot.features is not None:
                slot.pt.run_targets(dict(slot.features, color=slot.color), self.viewports, st)
            else:
                slot.pt.run(slot.color, self.viewports, stream if stream is not None else slot.stream)

    def transfer_and_stitch(self, own_slot=None):
        """device_transfer + stitch_stage over RCCL: gather partial frames on rank 0 (default stream).  `own_slot`: the display
        rank's slot whose path tracing the stitch (not the receives) has to wait for."""
        if self.world_size == 1:
            return
        if self.exchange is not None:
            partials = self.exchange.gather_to_display(self.color, self.dists, self.rank, self.world_size, self.viewports, self.recv_buffers, self.ctx)
        else:
            from .transfer import gather_to_display
            partials = gather_to_display(self.color, self.dists, self.rank, self.world_size, self.viewports, self.recv_buffers)
        if own_slot is not None and own_slot.stream is not None:
            self.ctx.stream_wait(None, own_slot.stream)
        if partials:
            peers = sorted(partials)
            self.stitch.run_all([self.dists[r] for r in peers], [partials[r] for r in peers], self.color, self.viewports)
        if self.rank == 0:
            self.stitch.set_blend_ratio(1.0)

    def render(self, tonemap=True, gather_views=False):
        self.render_partial(tonemap=tonemap)
        slot = self.current
        if self.world_size == 1:
            if self.post.frame_order:
                # a history is one chain over the frames of all slots: the chain runs on the default stream, in frame order
                if slot.stream is not None:
                    self.ctx.stream_wait(None, slot.stream)
                self.post_process(None, tonemap=tonemap)
                if slot.stream is not None:
                    self.ctx.stream_wait(slot.stream, None)
            elif tonemap and not self.fused_tonemap:
                self.post_process(slot.stream)       # the whole frame stays on its slot's stream
            self.accumulated_frames += 1
            return
        # Several ranks.  Everything after the path tracing runs on the default stream, which is also torch's current
        # stream: RCCL orders itself after the kernels enqueued there.  With frames in flight the default stream first
        # waits for this slot's path tracing, and the slot's stream afterwards waits for the default stream, so that the
        # next frame of this slot does not overwrite images that are still being sent, stitched or tonemapped.
        # The display rank of a pixel-sharded frame receives into buffers of its own: its receives need not wait for its own
        # path tracing, only the stitch into its image does.
        display_of_pixels = self.shard == "pixels" and self.rank == 0
        if slot.stream is not None and not display_of_pixels:
            self.ctx.stream_wait(None, slot.stream)
        if self.shard == "views":
            # every rank finishes its own views (tonemap is per pixel); `gather_views` ships them to the writer on rank 0
            if (tonemap or self.plan.stages[0] != "tonemap") and self.viewports > 0:      # stages in front of the tonemap run without it
                self.post_process(tonemap=tonemap)
            if gather_views:
                from .transfer import gather_views_to_display
                src = self.display if tonemap else self.color
                self.all_views = gather_views_to_display(src, self.total_viewports, self.rank, self.world_size, self.all_views)
        elif self.shard == "samples":
            from .transfer import reduce_samples_to_display
            reduce_samples_to_display(self.color, self.rank, self.world_size)
            if tonemap and self.rank == 0:
                self.post_process()
        else:
            self.transfer_and_stitch(slot if display_of_pixels else None)
            if tonemap and self.rank == 0:
                self.post_process()
        if slot.stream is not None:
            self.ctx.stream_wait(slot.stream, None)
        self.accumulated_frames += 1

    def post_process(self, stream=None, tonemap=True):
        """The post-processing chain of the last frame (PostProcessingRenderer.run)."""
        self.post.run(self.current, stream, tonemap)

    def download(self, which="color") -> np.ndarray:
        """The most recent frame's partial colour target or tonemapped display image; with a Looking Glass output also "composed" (the
        panel's image, RGBA32F [h][w][4]) and "composed8" (uint8 [h][w][4])."""
        self.sync()
        if which in ("composed", "composed8"):
            if self.post.lkg is None or self.current.composed is None:
                raise KeyError(f"{which}: the renderer has no Looking Glass output (looking_glass=...) or no frame was post-processed")
            ow, oh = self.post.lkg.out_size
            if which == "composed":
                return self.current.composed.download((oh, ow, 4), np.float32)
            return self.current.composed8.download((oh, ow, 4), np.uint8)
        buf = self.color if which == "color" else self.display
        if which == "color":
            tw, th = self.target_size
        else:
            tw, th = self.size
        if self.use_torch:
            self._torch.cuda.synchronize()
            return buf.cpu().numpy()
        return buf.download((self.output_viewports, th, tw, 4), np.float32)

    def close(self):
        if not self.slots:
            return
        self.sync()
        self.post.close()
        for slot in self.slots:
            for pt in self._stages(slot):
                pt.close()
            if slot.stream is not None:
                self.ctx.destroy_stream(slot.stream)
                slot.stream = None
        self.slots = []

    def __del__(self):
        try:
            if self.ctx.h:
                self.close()
        except Exception:
            pass
