"""ctypes binding of libtrhip.so (include/trhip.h).  There is no CPU fallback: if the HIP
library is missing or no GPU is present the calls fail loudly."""
from __future__ import annotations

import ctypes as C
import os

# Hardware queues the HIP runtime spreads its streams over (default 4): frame slots beyond three only pay off with more
# (DESIGN.md section 5).  Read by the runtime when it starts, so it has to be in the environment before the library loads.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
# Memory shared between processes (RCCL's buffers, trhip_ipc_*): the host driver of the target boxes supports dmabuf IPC only.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRHIP_LIB", os.path.join(_HERE, "libtrhip.so"))   # TRHIP_LIB: A/B builds while tuning


class TrhipError(RuntimeError):
    pass


class SceneDescC(C.Structure):
    _fields_ = [
        ("instances", C.c_void_p), ("spans", C.c_void_p), ("instance_count", C.c_uint32),
        ("vertices", C.c_void_p), ("vertex_count", C.c_uint32),
        ("indices", C.c_void_p), ("index_count", C.c_uint32),
        ("point_lights", C.c_void_p), ("point_light_count", C.c_uint32),
        ("directional_lights", C.c_void_p), ("directional_light_count", C.c_uint32),
        ("texture_infos", C.c_void_p), ("texture_count", C.c_uint32), ("texels", C.c_void_p),
        ("envmap", C.c_void_p), ("envmap_width", C.c_uint32), ("envmap_height", C.c_uint32),
        ("alias_table", C.c_void_p), ("environment_factor", C.c_float * 4),
        ("cameras", C.c_void_p), ("camera_count", C.c_uint32),
        ("non_opaque", C.c_void_p), ("gather_emissive_triangles", C.c_uint32)]


class AccelInfoC(C.Structure):
    _fields_ = [("triangle_count", C.c_uint32), ("node_count", C.c_uint32), ("tri_light_count", C.c_uint32),
                ("build_ms", C.c_float), ("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3),
                ("node_bytes", C.c_uint32), ("leaf_count", C.c_uint32)]


class AccelLayoutC(C.Structure):
    """trhip_accel_layout: how the last build laid the acceleration structure out (include/trhip.h)."""
    _fields_ = [("strategy", C.c_int32), ("blas_count", C.c_uint32), ("tlas_leaf_count", C.c_uint32), ("blas_updated", C.c_uint32),
                ("node_bytes", C.c_uint64), ("record_bytes", C.c_uint64), ("blas_ms", C.c_float), ("tlas_ms", C.c_float)]


# trhip_scene_set_accel_strategy
AS_ALL_MERGED, AS_PER_MESH, AS_STATIC_MERGED_DYNAMIC_PER_MESH = 0, 1, 2


class LightAccelInfoC(C.Structure):
    """trhip_light_accel_info: the sphere-light mode and tree of the scene (include/trhip.h)."""
    _fields_ = [("requested", C.c_int32), ("in_effect", C.c_int32), ("sphere_lights", C.c_uint32), ("tree_lights", C.c_uint32),
                ("node_count", C.c_uint32), ("auto_threshold", C.c_uint32), ("tree_bytes", C.c_uint64), ("last_ms", C.c_float),
                ("last_was_refit", C.c_int32)]


class LightCountersC(C.Structure):
    """trhip_light_counters: sphere tests, light-tree node visits and walks that fell back to the loop, of the closest-hit rays."""
    _fields_ = [("sphere_tests", C.c_uint64), ("node_visits", C.c_uint64), ("walk_fallbacks", C.c_uint64)]


# trhip_scene_set_light_accel
LIGHT_ACCEL_AUTO, LIGHT_ACCEL_LOOP, LIGHT_ACCEL_TREE = 0, 1, 2


class TerminalCountersC(C.Structure):
    """trhip_terminal_counters: blocked and fallback rays of the terminal query, whether it is in effect, the emitter set's size."""
    _fields_ = [("blocked_rays", C.c_uint64), ("fallback_rays", C.c_uint64), ("in_effect", C.c_uint32), ("emitter_triangles", C.c_uint32),
                ("threshold", C.c_uint32), ("pad", C.c_uint32)]


# trhip_pt_set_terminal_query
TERMINAL_QUERY_AUTO, TERMINAL_QUERY_OFF = 0, 1
HIT_BLOCKED = -2      # instance_id of a blocked ray in the hits of trhip_trace_terminal


# trhip_pt_set_primary_start
PRIMARY_START_AUTO, PRIMARY_START_OFF = 0, 1


class PrimaryStartInfoC(C.Structure):
    """trhip_primary_start_info: the mode that was set (-1 none), what the next frame does, what the last frame did (-1 none yet)."""
    _fields_ = [("mode", C.c_int32), ("in_effect", C.c_int32), ("last_frame", C.c_int32), ("pad", C.c_int32)]


class PtOptionsC(C.Structure):
    """== path_tracer_stage::options (reference src/path_tracer_stage.hh:13-30), flattened."""
    _fields_ = [
        ("max_bounces", C.c_int32), ("min_ray_dist", C.c_float), ("rng_seed", C.c_uint32), ("sampler", C.c_int32),
        ("samples_per_pixel", C.c_int32), ("samples_per_pass", C.c_int32), ("projection", C.c_int32),
        ("film", C.c_int32), ("film_radius", C.c_float), ("mis_mode", C.c_int32),
        ("russian_roulette_delta", C.c_float), ("indirect_clamping", C.c_float), ("regularization_gamma", C.c_float),
        ("depth_of_field", C.c_int32), ("nee_point", C.c_float), ("nee_directional", C.c_float),
        ("nee_envmap", C.c_float), ("nee_triangles", C.c_float), ("bounce_mode", C.c_int32),
        ("tri_light_mode", C.c_int32), ("hide_lights", C.c_int32), ("use_white_albedo_on_first_bounce", C.c_int32),
        ("transparent_background", C.c_int32), ("pre_transformed_vertices", C.c_int32)]


class DistributionC(C.Structure):
    _fields_ = [("size_x", C.c_uint32), ("size_y", C.c_uint32), ("strategy", C.c_int32),
                ("index", C.c_uint32), ("count", C.c_uint32), ("primary", C.c_uint32)]


class CountersC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("closest_rays", "shadow_rays", "node_visits", "tri_tests", "alpha_tests",
                                          "surface_hits", "stack_overflows")]


class TimingsC(C.Structure):
    _fields_ = ([(n, C.c_float) for n in ("path_tracing_ms", "trace_closest_ms", "trace_shadow_ms", "shade_ms", "raygen_ms", "resolve_ms")]
                + [(n, C.c_uint32) for n in ("trace_closest_launches", "trace_shadow_launches", "shade_launches", "frames")])


class PhaseCountersC(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("lane_node_phases", "lane_tri_phases", "quad_node_phases", "quad_tri_phases",
                                           "lane_node_phases_le16", "lane_node_visits_le16")] + [("lane_node_phase_hist", C.c_uint64 * 8),
                                                                                                 ("closest_node_visits", C.c_uint64)])


class ProgramInfoC(C.Structure):
    """trhip_program_info: which shading program renders a stage (kind 0 general / 1 command-line set ahead of time / 2 compiled), its arithmetic, identity."""
    _fields_ = [("kind", C.c_int32), ("ieee", C.c_int32), ("identity", C.c_uint64), ("key", C.c_char * 240)]


class PtTargetsC(C.Structure):
    """trhip_pt_targets: device images, None = not requested."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "diffuse", "reflection", "albedo", "material", "normal", "pos", "instance_id", "screen_motion")]


class TonemapInfoC(C.Structure):
    _fields_ = [("op", C.c_int32), ("exposure", C.c_float), ("gamma", C.c_float), ("alpha_grid_background", C.c_int32)]


class BmfrOptionsC(C.Structure):
    """trhip_bmfr_options: bmfr_stage::options (settings) + the noise amplitude of the fit (0 = 1e-2)."""
    _fields_ = [("settings", C.c_int32), ("noise_amount", C.c_float)]


class BmfrFeaturesC(C.Structure):
    """trhip_bmfr_features: the gbuffer entries the BMFR stage reads; color is also its output.  instance_id may be None."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "diffuse", "albedo", "normal", "pos", "screen_motion", "instance_id")]


class BmfrTimingsC(C.Structure):
    _fields_ = ([(n, C.c_float) for n in ("preprocess_ms", "fit_ms", "weighted_sum_ms", "accumulate_output_ms", "total_ms")]
                + [("frames", C.c_uint32)])


# trhip_bmfr_options::settings, trhip_bmfr_download
BMFR_DIFFUSE_ONLY, BMFR_DIFFUSE_SPECULAR = 0, 1
(BMFR_NOISY_DIFFUSE, BMFR_NOISY_SPECULAR, BMFR_FILTERED_DIFFUSE, BMFR_FILTERED_SPECULAR, BMFR_FEATURE_ROWS, BMFR_WEIGHTS, BMFR_MIN_MAX,
 BMFR_ACCEPT_BITS, BMFR_BLOCK_OFFSETS, BMFR_PREVIOUS_NORMAL, BMFR_PREVIOUS_POS) = range(11)


class GbufferTargetsC(C.Structure):
    """trhip_gbuffer_targets: what trhip_gbuffer_render writes per viewport; None = not requested."""
    _fields_ = [(n, C.c_void_p) for n in ("normal", "pos", "instance_id")]


class ReprojectionImagesC(C.Structure):
    """trhip_reprojection_images: the images a reprojection stage reads (and, for the temporal stage's colour, writes)."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "normal", "pos", "instance_id", "screen_motion")]


class ReprojectionTimingsC(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("frames", C.c_uint32)]


# trhip_*_reprojection_download; the kinds of a decision record
REPROJECTION_DECISIONS, REPROJECTION_PREVIOUS_COLOR, REPROJECTION_PREVIOUS_NORMAL, REPROJECTION_PREVIOUS_POS = range(4)
REPROJ_NONE, REPROJ_REPROJECTED, REPROJ_SKY_COPY = 0, 1, 2
# the decision record: 8 bytes per pixel
REPROJECTION_RECORD = [("kind", "u1"), ("slot", "u1"), ("bits", "u1"), ("zero", "u1"), ("ox", "<i2"), ("oy", "<i2")]


class TaaOptionsC(C.Structure):
    """trhip_taa_options."""
    _fields_ = [("alpha", C.c_float), ("gamma", C.c_float), ("edge_dilation", C.c_int32), ("anti_shimmer", C.c_int32),
                ("base_camera_index", C.c_uint32), ("projection", C.c_int32)]


class TaaImagesC(C.Structure):
    """trhip_taa_images."""
    _fields_ = [(n, C.c_void_p) for n in ("src", "dst", "screen_motion", "pos", "instance_id")]


class TaaTimingsC(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("frames", C.c_uint32), ("name", C.c_char * 64)]


# trhip_taa_download; the bits of a decision byte
TAA_HISTORY, TAA_DECISIONS = 0, 1
TAA_DECISION_OFFSET_MASK, TAA_DECISION_OUTSIDE, TAA_DECISION_NO_SURFACE = 0x0F, 0x10, 0x20


class LkgOptionsC(C.Structure):
    """trhip_lkg_options."""
    _fields_ = [("viewport_count", C.c_uint32), ("pitch", C.c_float), ("tilt", C.c_float), ("center", C.c_float), ("invert", C.c_int32),
                ("record_view_indices", C.c_int32)]


class LkgTimingsC(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("frames", C.c_uint32), ("name", C.c_char * 64)]


# trhip_lkg_download
LKG_VIEW_INDICES = 0


class ShOptionsC(C.Structure):
    """trhip_sh_options."""
    _fields_ = [("order", C.c_int32), ("resolution", C.c_uint32 * 3), ("samples_per_probe", C.c_uint32), ("temporal_ratio", C.c_float)]


class ShGridDataC(C.Structure):
    """trhip_sh_grid_data: grid_data_buffer as the next render would pack it."""
    _fields_ = [("transform", C.c_float * 16), ("normal_transform", C.c_float * 16), ("grid_size", C.c_uint32 * 3), ("mix_ratio", C.c_float),
                ("cell_scale", C.c_float * 3), ("rotation_x", C.c_float), ("rotation_y", C.c_float)]


class ShTimingsC(C.Structure):
    _fields_ = ([("total_ms", C.c_float), ("frames", C.c_uint32), ("name", C.c_char * 64)] +
                [(n, C.c_float) for n in ("raygen_ms", "trace_closest_ms", "trace_shadow_ms", "shade_ms", "project_ms")])


# trhip_sh_download
SH_GRID, SH_GRID_HALF = 0, 1


class DshgiOptionsC(C.Structure):
    """trhip_dshgi_options."""
    _fields_ = [("order", C.c_int32), ("use_probe_visibility", C.c_int32), ("record_surface", C.c_int32)]


class DshgiGridC(C.Structure):
    """trhip_dshgi_grid."""
    _fields_ = [("grid_half_dev", C.c_void_p), ("resolution", C.c_uint32 * 3), ("transform", C.c_float * 16), ("scaling", C.c_float * 3)]


class DshgiTimingsC(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("frames", C.c_uint32), ("name", C.c_char * 64)]


# trhip_dshgi_download; DSHGI_SURFACE is trhip_dshgi_surface per pixel
DSHGI_INDIRECT, DSHGI_SURFACE = 0, 1
DSHGI_SURFACE_DTYPE = [("pos", "<f4", 3), ("smooth_normal", "<f4", 3), ("mapped_normal", "<f4", 3), ("view", "<f4", 3), ("albedo", "<f4", 4),
                       ("metallic", "<f4"), ("roughness", "<f4"), ("f0", "<f4"), ("transmittance", "<f4"), ("grid", "<i4"), ("instance_id", "<i4")]


class RestirDiOptionsC(C.Structure):
    """trhip_restir_di_options."""
    _fields_ = [("candidates", C.c_uint32), ("spatial_samples", C.c_uint32), ("search_radius", C.c_float), ("max_confidence", C.c_float),
                ("temporal_reuse", C.c_int32), ("min_ray_dist", C.c_float), ("rng_seed", C.c_uint32), ("record", C.c_int32)]


class RestirDiTimingsC(C.Structure):
    _fields_ = [("canonical_ms", C.c_float), ("spatial_ms", C.c_float), ("total_ms", C.c_float), ("frames", C.c_uint32),
                ("canonical_name", C.c_char * 64), ("spatial_name", C.c_char * 64)]


# trhip_restir_di_download and the records behind the codes (include/trhip.h)
(RESTIR_DI_SURFACE, RESTIR_DI_CANONICAL, RESTIR_DI_HISTORY, RESTIR_DI_CANDIDATES, RESTIR_DI_TEMPORAL, RESTIR_DI_SPATIAL,
 RESTIR_DI_FINAL, RESTIR_DI_SAMPLED, RESTIR_DI_LIGHT_WEIGHTS, RESTIR_DI_LIGHT_TABLE, RESTIR_DI_BSDF_CANDIDATES) = range(11)
# trhip_restir_di_set_visibility: the modes by their command-line names
RESTIR_VISIBILITY = {"per-target": 0, "shared": 1, "sampled": 2}
# trhip_restir_di_set_light_selection: the modes by their command-line names; the table's 16-byte entries (download code 9)
RESTIR_LIGHT_SELECTION = {"uniform": 0, "power": 1}
RESTIR_SPHERE_LIGHTS = {"point": 0, "area": 1}      # TRHIP_RESTIR_SPHERE_LIGHTS_*
RESTIR_DI_LIGHT_TABLE_DTYPE = [("alias_id", "<u4"), ("probability", "<u4"), ("pdf", "<f4"), ("alias_pdf", "<f4")]
# trhip_restir_di_bsdf_candidate (download code 10): one per candidate of a stage with BSDF candidates
RESTIR_DI_BSDF_CANDIDATE_DTYPE = [("technique", "<u4"), ("dir", "<f4", 3), ("p_b", "<f4"), ("instance_id", "<i4"), ("primitive_id", "<i4"), ("u", "<f4"),
                                  ("v", "<f4"), ("t", "<f4"), ("denom", "<f4"), ("traced", "<u4")]
RESTIR_DI_NULL_INDEX = (1 << 30) - 1
RESTIR_DI_SURFACE_DTYPE = [("pos", "<f4", 3), ("instance_id", "<i4"), ("mapped_normal", "<f4", 3), ("metallic", "<f4"), ("flat_normal", "<f4", 3),
                           ("roughness", "<f4"), ("view", "<f4", 3), ("transmittance", "<f4"), ("albedo", "<f4", 4), ("emission", "<f4", 3),
                           ("f0", "<f4"), ("ior_in", "<f4"), ("ior_out", "<f4"), ("pad", "<f4", 2)]
RESTIR_DI_RESERVOIR_DTYPE = [("uc_weight", "<f4"), ("target_function", "<f4"), ("light", "<u4"), ("confidence", "<f4"), ("light_data", "<f4", 2),
                             ("pad", "<u4", 2)]
RESTIR_DI_CANDIDATE_DTYPE = [("light", "<u4"), ("light_data", "<f4", 2), ("pdf", "<f4"), ("contribution", "<f4", 3), ("visibility", "<f4"),
                             ("weight", "<f4"), ("draw", "<f4"), ("selected", "<u4"), ("pad", "<u4")]
RESTIR_DI_TEMPORAL_DTYPE = [("px", "<i4"), ("py", "<i4"), ("reuse", "<u4"), ("prev_confidence", "<f4"), ("target", "<f4"), ("weight", "<f4"),
                            ("draw", "<f4"), ("selected", "<u4")]
RESTIR_DI_SPATIAL_DTYPE = [("px", "<i4"), ("py", "<i4"), ("good", "<u4"), ("selected", "<u4"), ("target_n", "<f4"), ("visibility_n", "<f4"),
                           ("jacobian_n", "<f4"), ("m", "<f4"), ("wi", "<f4"), ("draw", "<f4"), ("target_c", "<f4"), ("visibility_c", "<f4"),
                           ("jacobian_c", "<f4"), ("mis_canonical", "<f4"), ("pad", "<f4", 2)]
RESTIR_DI_FINAL_DTYPE = [("contribution", "<f4", 3), ("visibility", "<f4"), ("canonical_m", "<f4"), ("wi", "<f4"), ("draw", "<f4"),
                         ("selected", "<u4")]
RESTIR_DI_SAMPLED_DTYPE = [("visibility", "<f4"), ("uc_weight_before", "<f4"), ("pad", "<u4", 2)]


class RestirGiOptionsC(C.Structure):
    """trhip_restir_gi_options."""
    _fields_ = [("spatial_samples", C.c_uint32), ("search_radius", C.c_float), ("max_confidence", C.c_float), ("temporal_reuse", C.c_int32),
                ("min_ray_dist", C.c_float), ("rng_seed", C.c_uint32), ("record", C.c_int32)]


class RestirGiTimingsC(C.Structure):
    _fields_ = [("initial_ms", C.c_float), ("temporal_ms", C.c_float), ("spatial_ms", C.c_float), ("total_ms", C.c_float), ("frames", C.c_uint32),
                ("initial_name", C.c_char * 64), ("temporal_name", C.c_char * 64), ("spatial_name", C.c_char * 64)]


# trhip_restir_gi_download and the records behind the codes (include/trhip.h); the surface, candidate, temporal, spatial and final
# records are ReSTIR DI's
(RESTIR_GI_SURFACE, RESTIR_GI_CANONICAL, RESTIR_GI_HISTORY, RESTIR_GI_INITIAL, RESTIR_GI_SECONDARY, RESTIR_GI_LIGHT, RESTIR_GI_TEMPORAL,
 RESTIR_GI_SPATIAL, RESTIR_GI_FINAL, RESTIR_GI_PATH, RESTIR_GI_PATH_SURFACE) = range(11)
RESTIR_GI_MAX_BOUNCES = 8
RESTIR_GI_SAMPLER_W = 0x80000000      # the fourth sampler coordinate of the stage's streams (csrc/restir_gi.h)
RESTIR_GI_RESERVOIR_DTYPE = [("x_s", "<f4", 3), ("uc_weight", "<f4"), ("n_s", "<f4", 3), ("target_function", "<f4"), ("L_o", "<f4", 3),
                             ("confidence", "<f4")]
RESTIR_GI_INITIAL_DTYPE = [("draw", "<f4", 2), ("pdf", "<f4"), ("traced", "<u4"), ("dir", "<f4", 3), ("t", "<f4"), ("instance_id", "<i4"),
                           ("primitive_id", "<i4"), ("u", "<f4"), ("v", "<f4"), ("light_draw", "<u4", 4), ("L_o", "<f4", 3), ("target", "<f4"),
                           ("weight", "<f4"), ("sel_draw", "<f4"), ("selected", "<u4"), ("pad", "<u4")]
RESTIR_GI_PATH_DTYPE = [("draw", "<f4", 2), ("pdf", "<f4"), ("traced", "<u4"), ("dir", "<f4", 3), ("t", "<f4"), ("instance_id", "<i4"),
                        ("primitive_id", "<i4"), ("u", "<f4"), ("v", "<f4"), ("light_draw", "<u4", 4), ("light", "<u4"), ("light_data", "<f4", 2),
                        ("light_pdf", "<f4"), ("contribution", "<f4", 3), ("visibility", "<f4"), ("factor", "<f4", 3), ("pad0", "<f4"),
                        ("throughput", "<f4", 3), ("pad1", "<f4"), ("L_o", "<f4", 3), ("pad2", "<f4")]


# every symbol include/trhip.h declares: (name, restype, argtypes)
_vp, _u32, _i, _f = C.c_void_p, C.c_uint32, C.c_int, C.c_float
SYMBOLS = {
    "trhip_image_decode": (_i, [_vp, C.c_size_t, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.POINTER(C.c_uint8))]),
    "trhip_image_free": (None, [C.POINTER(C.c_uint8)]),
    "trhip_exr_decode": (_i, [_vp, C.c_size_t, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.POINTER(C.c_float))]),
    "trhip_exr_encode": (_i, [_vp, _u32, _u32, _i, _i, _i, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]),
    "trhip_exr_free": (None, [_vp]),
    "trhip_device_create": (_i, [_i, C.POINTER(_vp)]),
    "trhip_device_destroy": (None, [_vp]),
    "trhip_last_error": (C.c_char_p, []),
    "trhip_malloc": (_i, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "trhip_image_decode_texels": (_i, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint8))]),
    "trhip_free": (_i, [_vp, _vp]),
    "trhip_upload": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "trhip_download": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "trhip_memset": (_i, [_vp, _vp, _i, C.c_size_t, _vp]),
    "trhip_sync": (_i, [_vp, _vp]),
    "trhip_copy_peer": (_i, [_vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "trhip_scene_upload": (_i, [_vp, C.POINTER(SceneDescC)]),
    "trhip_scene_update_cameras": (_i, [_vp, _vp, _u32]),
    "trhip_scene_set_previous_cameras": (_i, [_vp, _vp, _u32]),
    "trhip_scene_update_instances": (_i, [_vp, _vp, _u32]),
    "trhip_scene_build_accel": (_i, [_vp, C.POINTER(AccelInfoC)]),
    "trhip_scene_refit_accel": (_i, [_vp, C.POINTER(AccelInfoC)]),
    "trhip_pt_set_frame_batch": (_i, [_vp, C.c_uint32]),
    "trhip_scene_update_lights": (_i, [_vp, _vp, C.c_uint32, _vp, C.c_uint32]),
    "trhip_scene_set_build_mode": (_i, [_vp, _i]),
    "trhip_scene_set_accel_strategy": (_i, [_vp, _i]),
    "trhip_scene_set_dynamic_instances": (_i, [_vp, _vp, _u32]),
    "trhip_scene_get_accel_layout": (_i, [_vp, C.POINTER(AccelLayoutC)]),
    "trhip_scene_set_light_accel": (_i, [_vp, _i]),
    "trhip_scene_get_light_accel": (_i, [_vp, C.POINTER(LightAccelInfoC)]),
    "trhip_pt_get_light_counters": (_i, [_vp, C.POINTER(LightCountersC)]),
    "trhip_pt_set_terminal_query": (_i, [_vp, _i]),
    "trhip_pt_get_terminal_counters": (_i, [_vp, C.POINTER(TerminalCountersC)]),
    "trhip_pt_set_primary_start": (_i, [_vp, _i]),
    "trhip_pt_get_primary_start": (_i, [_vp, C.POINTER(PrimaryStartInfoC)]),
    "trhip_pt_get_max_stack_depth": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "trhip_trace_terminal": (_i, [_vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "trhip_stitch_batch": (_i, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, C.c_float, _vp]),
    "trhip_stream_create": (_i, [_vp, C.POINTER(C.c_void_p)]),
    "trhip_stream_destroy": (_i, [_vp, _vp]),
    "trhip_stream_pipe_class": (_i, [_vp, _vp, C.POINTER(C.c_int32)]),
    "trhip_device_get_info": (_i, [_vp, _vp]),
    "trhip_build_id": (C.c_uint64, []),
    "trhip_stream_wait": (_i, [_vp, _vp, _vp]),
    "trhip_stream_wait_peer": (_i, [_vp, _vp, _vp, _vp]),
    "trhip_pt_set_frame_counter": (_i, [_vp, _u32]),
    "trhip_pt_set_lanes": (_i, [_vp, C.c_int]),
    "trhip_pt_set_frame_slots": (_i, [_vp, C.c_int]),
    "trhip_pt_set_fused_tonemap": (_i, [_vp, _vp, _vp]),
    "trhip_pt_get_lane_pipes": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "trhip_pt_set_shading_arithmetic": (_i, [_vp, C.c_int]),
    "trhip_pt_set_specialization": (_i, [_vp, C.c_int]),
    "trhip_pt_precompile": (_i, [C.POINTER(PtOptionsC), C.c_int, C.c_int, C.c_int, C.c_char_p]),
    "trhip_kernel_cache_dir": (C.c_char_p, []),
    "trhip_pt_set_shard": (_i, [_vp, _u32, _u32, _u32, _u32]),
    "trhip_scene_set_skin": (_i, [_vp, _u32, _vp, _vp, _u32]),
    "trhip_scene_skin": (_i, [_vp, _u32, _vp, _u32]),
    "trhip_scene_set_morph_targets": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _u32]),
    "trhip_scene_morph": (_i, [_vp, _u32, _vp, _u32]),
    "trhip_scene_get_vertices": (_i, [_vp, _u32, _vp, _u32]),
    "trhip_scene_set_deformation_motion": (_i, [_vp, _i]),
    "trhip_scene_latch_positions": (_i, [_vp]),
    "trhip_scene_get_previous_positions": (_i, [_vp, _u32, _vp, _u32]),
    "trhip_scene_get_tri_lights": (_i, [_vp, _vp, _u32]),
    "trhip_pt_create": (_i, [_vp, C.POINTER(PtOptionsC), C.POINTER(_vp)]),
    "trhip_direct_create": (_i, [_vp, C.POINTER(PtOptionsC), C.POINTER(_vp)]),
    "trhip_pt_destroy": (None, [_vp]),
    "trhip_pt_set_distribution": (_i, [_vp, C.POINTER(DistributionC)]),
    "trhip_pt_reset_accumulation": (_i, [_vp, _i]),
    "trhip_pt_render": (_i, [_vp, _vp, _u32, _u32, _u32, _vp]),
    "trhip_pt_render_targets": (_i, [_vp, C.POINTER(PtTargetsC), _u32, _u32, _u32, _vp]),
    "trhip_pt_set_profiling": (_i, [_vp, _i, _i]),
    "trhip_pt_get_counters": (_i, [_vp, C.POINTER(CountersC)]),
    "trhip_pt_reset_counters": (_i, [_vp]),
    "trhip_pt_get_timings": (_i, [_vp, C.POINTER(TimingsC)]),
    "trhip_pt_get_phase_counters": (_i, [_vp, C.POINTER(PhaseCountersC)]),
    "trhip_pt_get_program": (_i, [_vp, C.POINTER(ProgramInfoC)]),
    "trhip_calibrate_valu": (_i, [_vp, C.POINTER(C.c_float)]),
    "trhip_calibrate_l1": (_i, [_vp, C.POINTER(C.c_float)]),
    "trhip_feature_render": (_i, [_vp, _i, C.POINTER(DistributionC), _i, _u32, _f, C.POINTER(_f), _vp, _u32, _u32, _vp]),
    "trhip_trace_closest": (_i, [_vp, _u32, _vp, _vp, _i, _vp, _vp]),
    "trhip_trace_shadow": (_i, [_vp, _u32, _vp, _vp, _vp]),
    "trhip_stitch": (_i, [_vp, C.POINTER(DistributionC), _vp, _u32, _u32, _vp, _u32, _f, _vp]),
    "trhip_tonemap": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, C.POINTER(TonemapInfoC), _vp]),
    "trhip_bmfr_create": (_i, [_vp, C.POINTER(BmfrOptionsC), _u32, _u32, _u32, C.POINTER(_vp)]),
    "trhip_bmfr_destroy": (None, [_vp]),
    "trhip_bmfr_run": (_i, [_vp, C.POINTER(BmfrFeaturesC), _u32, _vp]),
    "trhip_bmfr_reset_history": (_i, [_vp]),
    "trhip_bmfr_get_timings": (_i, [_vp, C.POINTER(BmfrTimingsC)]),
    "trhip_bmfr_fit_blocks": (_i, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "trhip_bmfr_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_gbuffer_render": (_i, [_vp, _i, C.POINTER(_u32), _u32, _f, C.POINTER(GbufferTargetsC), _u32, _u32, _vp]),
    "trhip_spatial_reprojection_create": (_i, [_vp, _u32, _u32, _u32, C.POINTER(_u32), _u32, C.POINTER(_f), C.POINTER(_vp)]),
    "trhip_spatial_reprojection_destroy": (None, [_vp]),
    "trhip_spatial_reprojection_run": (_i, [_vp, C.POINTER(ReprojectionImagesC), C.POINTER(ReprojectionImagesC), _vp, _vp]),
    "trhip_spatial_reprojection_get_timings": (_i, [_vp, C.POINTER(ReprojectionTimingsC)]),
    "trhip_spatial_reprojection_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_temporal_reprojection_create": (_i, [_vp, _u32, _u32, _u32, _f, C.POINTER(_vp)]),
    "trhip_temporal_reprojection_destroy": (None, [_vp]),
    "trhip_temporal_reprojection_run": (_i, [_vp, C.POINTER(ReprojectionImagesC), _vp]),
    "trhip_temporal_reprojection_reset_history": (_i, [_vp]),
    "trhip_temporal_reprojection_get_timings": (_i, [_vp, C.POINTER(ReprojectionTimingsC)]),
    "trhip_temporal_reprojection_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_taa_create": (_i, [_vp, C.POINTER(TaaOptionsC), _u32, _u32, _u32, C.POINTER(_vp)]),
    "trhip_taa_destroy": (None, [_vp]),
    "trhip_taa_run": (_i, [_vp, C.POINTER(TaaImagesC), _vp]),
    "trhip_taa_reset_history": (_i, [_vp]),
    "trhip_taa_get_timings": (_i, [_vp, C.POINTER(TaaTimingsC)]),
    "trhip_taa_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_lkg_create": (_i, [_vp, C.POINTER(LkgOptionsC), _u32, _u32, _u32, _u32, C.POINTER(_vp)]),
    "trhip_lkg_destroy": (None, [_vp]),
    "trhip_lkg_run": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "trhip_lkg_get_timings": (_i, [_vp, C.POINTER(LkgTimingsC)]),
    "trhip_lkg_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_sh_create": (_i, [_vp, C.POINTER(PtOptionsC), C.POINTER(ShOptionsC), C.POINTER(_vp)]),
    "trhip_sh_destroy": (None, [_vp]),
    "trhip_sh_set_transform": (_i, [_vp, C.POINTER(_f), C.POINTER(_f)]),
    "trhip_sh_set_frame_counter": (_i, [_vp, _u32]),
    "trhip_sh_reset_history": (_i, [_vp]),
    "trhip_sh_set_lanes": (_i, [_vp, _i]),
    "trhip_sh_set_batch_probes": (_i, [_vp, _u32]),
    "trhip_sh_set_shading_arithmetic": (_i, [_vp, _i]),
    "trhip_sh_get_grid_data": (_i, [_vp, C.POINTER(ShGridDataC)]),
    "trhip_sh_pack_grid_data": (_i, [C.POINTER(_f), C.POINTER(_f), C.POINTER(_u32), _u32, _u32, _u32, _f, C.POINTER(ShGridDataC)]),
    "trhip_sh_render": (_i, [_vp, _vp]),
    "trhip_sh_get_grids": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "trhip_sh_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_sh_get_counters": (_i, [_vp, C.POINTER(CountersC)]),
    "trhip_sh_get_timings": (_i, [_vp, C.POINTER(ShTimingsC)]),
    "trhip_sh_get_primary_start": (_i, [_vp, C.POINTER(PrimaryStartInfoC)]),
    "trhip_sh_set_profiling": (_i, [_vp, _i, _i]),
    "trhip_sh_reset_counters": (_i, [_vp]),
    "trhip_dshgi_create": (_i, [_vp, C.POINTER(DshgiOptionsC), _u32, _u32, _u32, C.POINTER(_vp)]),
    "trhip_dshgi_destroy": (None, [_vp]),
    "trhip_dshgi_set_grids": (_i, [_vp, C.POINTER(DshgiGridC), _u32]),
    "trhip_dshgi_set_instance_grids": (_i, [_vp, C.POINTER(C.c_int32), _u32]),
    "trhip_dshgi_set_brdf_integration": (_i, [_vp, _vp, _u32, _u32]),
    "trhip_dshgi_render": (_i, [_vp, _i, C.POINTER(_u32), _u32, _f, _vp, _vp, _vp]),
    "trhip_dshgi_get_timings": (_i, [_vp, C.POINTER(DshgiTimingsC)]),
    "trhip_dshgi_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_dshgi_pick_grid": (_i, [C.POINTER(_f), C.POINTER(_f), C.POINTER(_u32), C.POINTER(_f), _u32, C.POINTER(_f), C.POINTER(C.c_int32)]),
    "trhip_brdf_integration_generate": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "trhip_restir_di_create": (_i, [_vp, C.POINTER(RestirDiOptionsC), _u32, _u32, _u32, C.POINTER(_vp)]),
    "trhip_restir_di_destroy": (None, [_vp]),
    "trhip_restir_di_reset": (_i, [_vp]),
    "trhip_restir_di_set_visibility": (_i, [_vp, _i]),
    "trhip_restir_di_set_light_selection": (_i, [_vp, _i, C.c_float]),
    "trhip_restir_di_refresh_light_selection": (_i, [_vp, C.POINTER(_u32)]),
    "trhip_restir_di_set_bsdf_candidates": (_i, [_vp, _u32]),
    "trhip_restir_di_set_sphere_lights": (_i, [_vp, _i]),
    "trhip_restir_di_render": (_i, [_vp, _i, C.POINTER(_u32), _u32, _vp, _vp]),
    "trhip_restir_di_get_timings": (_i, [_vp, C.POINTER(RestirDiTimingsC)]),
    "trhip_restir_di_download": (_i, [_vp, _i, _vp, C.c_size_t]),
    "trhip_restir_gi_create": (_i, [_vp, C.POINTER(RestirGiOptionsC), _u32, _u32, _u32, C.POINTER(_vp)]),
    "trhip_restir_gi_destroy": (None, [_vp]),
    "trhip_restir_gi_reset": (_i, [_vp]),
    "trhip_restir_gi_set_bounces": (_i, [_vp, _u32]),
    "trhip_restir_gi_render": (_i, [_vp, _i, C.POINTER(_u32), _u32, _vp, _vp, _vp]),
    "trhip_restir_gi_get_timings": (_i, [_vp, C.POINTER(RestirGiTimingsC)]),
    "trhip_restir_gi_download": (_i, [_vp, _i, _vp, C.c_size_t]),
}

_LIB = None


def lib():
    """Loads libtrhip.so; raises TrhipError when it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TrhipError(f"{LIB_PATH} is missing: build it with `make -C tauray_amd/csrc` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                # the tree's own library exports everything (tests/test_abi_and_host.py); a library named by TRHIP_LIB may be an older
                # build kept for an A/B (tools/ab_libs.sh): calls it does not have fail when they are made
                if "TRHIP_LIB" not in os.environ:
                    raise
                continue
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        raise TrhipError(lib().trhip_last_error().decode("utf-8", "replace"))
