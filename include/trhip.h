/* trhip - C ABI of the MI355X-native path-tracing core.
 *
 * This is the drop-in boundary for Tauray's path_tracer_stage hot path.  The
 * reference has no FFI: its extension point is C++ subclassing
 * (docs/DEVELOPERS.md:3-27; rt_renderer<Pipeline> in src/rt_renderer.hh:28-77).
 * Each entry point below names the reference interface it replaces; the
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: one opaque trhip_device per HIP device, all calls from one host
 * thread, work is enqueued on the caller's hipStream_t (passed as void*; NULL =
 * the default stream) and is asynchronous unless stated.  Every function
 * returns 0 on success, non-zero on failure with a message available from
 * trhip_last_error() (the reference throws std::runtime_error instead).
 * All POD layouts are the reference's GPU-side structs.
 */
#ifndef TRHIP_H
#define TRHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trhip_device trhip_device;
typedef struct trhip_pt trhip_pt;

/* ---- device / memory (replaces tr::context + tr::device, src/context.hh, src/device.hh) */
int trhip_device_create(int hip_device, trhip_device** out);
void trhip_device_destroy(trhip_device* dev);
const char* trhip_last_error(void);
int trhip_malloc(trhip_device* dev, size_t bytes, void** out);           /* gpu_buffer (src/gpu_buffer.hh) */
int trhip_free(trhip_device* dev, void* ptr);
int trhip_upload(trhip_device* dev, void* dst_dev, const void* src_host, size_t bytes, void* stream);
int trhip_download(trhip_device* dev, void* dst_host, const void* src_dev, size_t bytes, void* stream); /* headless readback, src/headless.cc:292-303 */
int trhip_memset(trhip_device* dev, void* dst_dev, int value, size_t bytes, void* stream);
int trhip_sync(trhip_device* dev, void* stream);
/* Frames in flight (MAX_FRAMES_IN_FLIGHT, src/context.hh:26).  Every call takes the stream it is ordered on; a frame
 * slot is a stream plus the stages and images it owns, and `dependencies` between stages on different streams
 * (src/dependency.hh; timeline-semaphore waits in multi_device_stage::run, src/stage.cc:35-76) become
 * trhip_stream_wait: work enqueued on `stream` after the call starts only when everything enqueued on `on` before the
 * call has finished.  No host synchronisation.  NULL is the default stream. */
int trhip_stream_create(trhip_device* dev, void** stream_out);
int trhip_stream_destroy(trhip_device* dev, void* stream);
int trhip_stream_wait(trhip_device* dev, void* stream, void* on);
/* Streams are kept for the life of the process and handed out by the hardware pipe their queue sits on (csrc/stream_pool.hip: queues
 * of one pipe do not overlap launches larger than the chip, so the slots of a renderer and the lanes of a stage are spread over the
 * pipes).  trhip_stream_create returns an idle stream of the pipe with the fewest takers; trhip_stream_destroy hands it back.
 * `pipe_class_out`: the pipe of any stream of this process, the caller's own included (small integers from 0 in the order pipes
 * were seen; -1 with TRHIP_PIPE_PROBE=0): two streams of one class serialise chip-filling launches. */
int trhip_stream_pipe_class(trhip_device* dev, void* stream, int32_t* pipe_class_out);
/* ---- Process requirements (what the library needs from the process it is loaded into; nothing in the reference corresponds -
 * the Vulkan driver owns its queues, src/context.hh:26, src/stage.cc:35-76).
 *  1. GPU_MAX_HW_QUEUES >= 8 in the environment BEFORE the first HIP call of the process (the HIP runtime reads it once).  A lone
 *     frame is cut into four lanes on four streams that must sit on four different hardware pipes to overlap; with the runtime's
 *     default of four hardware queues the streams of one process share fewer pipes: sponza_teapots 1920x1080 renders in 4.55 ms
 *     instead of 3.69, a 1/8 strip in 1.0 instead of 0.75.  Frames are the same bits either way.  The
 *     Python mirror (tauray_amd/_lib.py), bench.py, the tests and the CLI (tauray_amd/host/tauray_hip_cli.cc) set it with
 *     setenv(.., overwrite = 0) before they touch HIP; an embedding application must do the same in its main() or launcher.
 *  2. Streams: create the streams you render on with trhip_stream_create (they come classified by pipe).  A stream of your own
 *     (or NULL - the default stream is classified by trhip_device_create) works too; the first stage that renders on it classifies it with a ~1 ms experiment if - and only if - the stream
 *     is idle and not capturing at that moment; otherwise its pipe stays unknown (-1) and the stage's lanes may share it.
 *     trhip_stream_pipe_class is the explicit form: it SYNCHRONISES `stream`, runs the experiment and remembers the result for
 *     that stream identity.  The library never synchronises a caller's stream anywhere else.
 *  3. trhip_device_get_info tells how many distinct pipes the process reaches (4 on MI355X with requirement 1 met; fewer = the
 *     -19 % case); with TRHIP_DEBUG=1 it and trhip_pt_render warn once on stderr when lanes share a pipe.
 *  4. TRHIP_PIPE_CLASSES=0,1,2,3 pins the classes of the library's streams in creation order and skips every experiment (for
 *     hosts that cannot afford the ~10 ms of probing at start-up or run under a tool that serialises queues);
 *     TRHIP_PIPE_PROBE=0 switches classification off altogether (every stream -1). */
typedef struct trhip_device_info {
    uint32_t struct_size;
    int32_t hip_device;
    char name[64];                    /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    char pci_bus_id[24];              /* "0000:05:00.0" */
    uint8_t uuid[16];
    int32_t compute_units;
    int32_t pipe_classes;             /* distinct hardware pipes the library's streams landed on (0: TRHIP_PIPE_PROBE=0) */
    int32_t pool_streams;             /* streams the library holds on this device (never destroyed) */
    int32_t hw_queues_env;            /* GPU_MAX_HW_QUEUES as this process sees it; 0 = unset (the runtime's default of 4) */
} trhip_device_info;
int trhip_device_get_info(trhip_device* dev, trhip_device_info* out);
/* The same dependency between streams of two devices of one process (the timeline semaphores the reference exports
 * between devices, src/device_transfer.cc:318-347, src/rt_renderer.cc:98-127): work enqueued on `stream` of `dev` after
 * the call starts only when everything enqueued on `on` of `on_dev` before the call has finished. */
int trhip_stream_wait_peer(trhip_device* dev, void* stream, trhip_device* on_dev, void* on);
/* device -> device copy over xGMI (replaces the pinned-host bounce of src/device_transfer.cc:140-290 when all
 * devices live in one process; with one process per GPU the same transfer is an RCCL send/recv) */
int trhip_copy_peer(trhip_device* dst_dev, void* dst, trhip_device* src_dev, const void* src, size_t bytes, void* stream);

/* ---- texture files (host only, no device involved).  What stb_image does for the reference's glTF loader through tinygltf
 * (src/gltf.cc:520-576): a PNG (any colour type and bit depth, interlaced or not) or a baseline / extended-sequential / progressive JPEG file
 * in memory becomes RGBA8, row 0 = top row of the file (include/tauray_image.hh; the C++ loader includes that header, the
 * Python mirror calls this entry point, so both flatten a scene to the same bytes).  *rgba_out is released with
 * trhip_image_free.  channels_in_file: 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA. */
int trhip_image_decode(const void* data, size_t bytes, uint32_t* width, uint32_t* height, uint32_t* channels_in_file, uint8_t** rgba_out);
/* The same file as the texels a scene stores: RGBA8 (*bits = 8), or - a PNG of 16 bits per sample - RGBA16 in host byte order
 * (*bits = 16, 8 bytes per texel): the reference keeps such an image as R16G16B16A16Unorm (src/gltf.cc:548-556).  Released with
 * trhip_image_free. */
int trhip_image_decode_texels(const void* data, size_t bytes, uint32_t* width, uint32_t* height, uint32_t* channels_in_file, uint32_t* bits, uint8_t** texels_out);
void trhip_image_free(uint8_t* rgba);

/* OpenEXR files (include/tauray_exr.hh; what tinyexr is to the reference).  trhip_exr_decode = read_exr of src/texture.cc:70-163:
 * a single-part scanline or tiled file (NONE / RLE / ZIPS / ZIP / PIZ; HALF, FLOAT or UINT channels) becomes interleaved floats,
 * *channels of them per pixel (at most four: R, G, B, A by the first letter of the channel names, or file order when a channel is
 * called anything else), row 0 = top of the data window.  trhip_exr_encode = the file headless::save_image writes
 * (src/headless.cc:355-412) from RGBA32F pixels: channels [A,] B, G, R as half or float; compression = the OpenEXR code
 * (0 none, 1 RLE, 2 ZIPS, 3 ZIP, 4 PIZ - the reference's default, src/headless.hh:56).  Results are released with trhip_exr_free. */
int trhip_exr_decode(const void* data, size_t bytes, uint32_t* width, uint32_t* height, uint32_t* channels, float** pixels_out);
int trhip_exr_encode(const float* rgba, uint32_t width, uint32_t height, int alpha, int half, int compression, uint8_t** bytes_out, size_t* size_out);
void trhip_exr_free(void* p);

/* ---- scene (replaces scene_stage::update's uploads, src/scene_stage.cc:1026-1496) */
typedef struct trhip_scene_desc {
    const void* instances;            /* 288-byte `instance` records (shader/scene.glsl:43-53) */
    const void* spans;                /* u32x4 per instance: vertex_offset, vertex_count, index_offset, triangle_count */
    uint32_t instance_count;
    const void* vertices;             /* 48-byte `vertex` records, model space (src/mesh.hh:19-25) */
    uint32_t vertex_count;
    const uint32_t* indices;          /* per-instance, relative to the instance's vertex span */
    uint32_t index_count;
    const void* point_lights;         /* 64 B (shader/light.glsl:15-27); point lights first, then spotlights */
    uint32_t point_light_count;
    const void* directional_lights;   /* 32 B (shader/light.glsl:7-13) */
    uint32_t directional_light_count;
    const void* texture_infos;        /* u32x4 per texture: width, height, texel_offset (in 4-byte words of `texels`), format (0 = RGBA8, 1 = RGBA16) */
    uint32_t texture_count;
    const uint8_t* texels;            /* RGBA8 (4 bytes per texel) or RGBA16 (8 bytes, host byte order) by the texture's format, row 0 first */
    const float* envmap;              /* RGBA32F lat-long, or NULL (then environment_factor is ignored, proj = -1) */
    uint32_t envmap_width, envmap_height;
    const void* alias_table;          /* 16 B entries (src/environment_map.hh:37-43), one per envmap texel */
    float environment_factor[4];
    const void* cameras;              /* 320-byte camera_data (shader/camera.glsl:13-23), one per viewport */
    uint32_t camera_count;
    const uint8_t* non_opaque;        /* per instance: material::potentially_transparent (src/material.cc:7-11) */
    uint32_t gather_emissive_triangles; /* scene_stage::options::gather_emissive_triangles (src/tauray.cc:384) */
} trhip_scene_desc;

typedef struct trhip_accel_info {
    uint32_t triangle_count;
    uint32_t node_count;
    uint32_t tri_light_count;
    float build_ms;                   /* device time of the whole build */
    float bounds_min[3], bounds_max[3];   /* all-merged: bounds of the triangle centroids (what the Morton codes quantise); two-level
                                            * strategies: the union of the instances' (conservative) world boxes, after a refit too */
    uint32_t node_bytes;              /* bytes one node visit reads (112: six box planes + child refs of a 4-wide node) */
    uint32_t leaf_count;              /* leaves of the tree (= triangle_count: one triangle per leaf); node_count = leaf_count - 1 */
} trhip_accel_info;

/* Copies the scene to the device (the reference's buffers byte for byte) and derives, next to them, one record
 * per index triangle with its three vertices side by side (128 bytes of positions, normals and texture coordinates = one cache line, and
 * 48 bytes of tangents apart), which the shading kernels read instead of indices + vertices (same values, fewer cache lines; rebuilt for
 * a mesh by trhip_scene_skin).  Spans that do not start at a whole
 * triangle, or that share indices over different vertex ranges, are valid input: such a scene gets no records and the general kernels. */
int trhip_scene_upload(trhip_device* dev, const trhip_scene_desc* desc);
int trhip_scene_update_cameras(trhip_device* dev, const void* camera_data, uint32_t count); /* src/scene_stage.cc:1145-1174 */
/* Moving lights: replaces the 64-byte point / spot light records and the 32-byte directional light records of the uploaded
 * scene, same counts (what scene_stage::update rewrites when a light's transformable changed, src/scene_stage.cc:1287-1354).
 * Triangle lights follow their instances (trhip_scene_update_instances + the acceleration-structure update). */
int trhip_scene_update_lights(trhip_device* dev, const void* point_lights, uint32_t point_light_count, const void* directional_lights,
                              uint32_t directional_light_count);
/* camera_pair.previous of every viewport (shader/scene.glsl:176-185); the current cameras until set.  Feeds the motion
 * features and the screen-motion target. */
int trhip_scene_set_previous_cameras(trhip_device* dev, const void* camera_data, uint32_t count);
/* Dynamic scenes: replaces the 288-byte instance records (model, model_normal, model_prev, material) of the uploaded
 * scene, same count and meshes (what scene_stage::update rewrites per frame, src/scene_stage.cc:1066-1116).  The
 * acceleration structure is invalidated: call trhip_scene_build_accel again (full rebuild on the device). */
int trhip_scene_update_instances(trhip_device* dev, const void* instances, uint32_t count);
/* Skinned meshes.  trhip_scene_set_skin marks the mesh of `instance` as animated: `source` is the bind-pose vertex array
 * (mesh::get_animation_source(), src/mesh.hh:47,73; NULL = the vertices uploaded for that instance) and `skins` one
 * {uvec4 joints, vec4 weights} record per vertex (mesh::skin_data, src/mesh.hh:32-36).  trhip_scene_skin runs
 * shader/skinning.comp over it with `joint_count` column-major mat4 joint transforms (global transform * inverse bind
 * matrix, model::update_joints src/model.cc:107-118) and rewrites the instance's vertices in the scene, as
 * scene_stage::record_skinning does per frame (src/scene_stage.cc:1543-1567).  Instances that share the vertex span
 * move together, like instances of one mesh in the reference.  The acceleration structure is invalidated: follow with
 * trhip_scene_refit_accel (the BLAS *update* of src/scene_stage.cc:1569-1612) or trhip_scene_build_accel. */
typedef struct trhip_skin { uint32_t joints[4]; float weights[4]; } trhip_skin;
int trhip_scene_set_skin(trhip_device* dev, uint32_t instance, const void* source_vertices, const trhip_skin* skins, uint32_t vertex_count);
int trhip_scene_skin(trhip_device* dev, uint32_t instance, const float* joint_transforms, uint32_t joint_count);
/* Morph targets (glTF 2.0 section 3.7.2.2; the reference's loader skips them).  trhip_scene_set_morph_targets gives the mesh of `instance`
 * `target_count` targets: each plane is float[target_count][vertex_count][3], the POSITION deltas and - or NULL - the NORMAL and TANGENT
 * (xyz) deltas.  The base they displace is a device copy of the instance's vertices as they stand, or of the bind pose of its skin when it
 * has one: glTF morphs first and skins second, so trhip_scene_set_skin comes first and is refused on an instance that has targets.
 * trhip_scene_morph evaluates base + sum of weights[k] * delta[k] over the non-zero weights, in the order tauray_amd/csrc/morph.h pins
 * (normals and tangents renormalised, uv and tangent.w kept), and writes the result to the instance's vertices in the scene - then, like
 * trhip_scene_skin, the acceleration structure is invalidated: follow with trhip_scene_refit_accel or trhip_scene_build_accel - or, on a
 * skinned instance, to the skin's bind pose: the scene changes at the next trhip_scene_skin.  Instances that share the vertex span move
 * together.  Under a two-level strategy a morphed instance is dynamic like a skinned one.  Refused: an instance out of range or without
 * targets, a vertex_count other than the mesh's, no targets, null positions, a weight count other than target_count, and any value that
 * is not finite.  A scene upload drops the targets, as it drops the skins. */
int trhip_scene_set_morph_targets(trhip_device* dev, uint32_t instance, uint32_t target_count, const float* position_deltas, const float* normal_deltas,
                                  const float* tangent_deltas, uint32_t vertex_count);
int trhip_scene_morph(trhip_device* dev, uint32_t instance, const float* weights, uint32_t weight_count);
/* Reads back the (possibly skinned or morphed) 48-byte vertices of one instance; for tests and tools. */
int trhip_scene_get_vertices(trhip_device* dev, uint32_t instance, void* out_host, uint32_t max_count);
/* Motion of deforming meshes (off by default, and then every output is what it was without these calls).  The
 * previous world position of a hit - feature outputs 6, 7 and 8, the screen_motion target of trhip_pt_render_targets, the temporal reuse
 * of trhip_restir_di_* - is model_prev * interp(model-space positions); with the switch off the positions are the current ones (the
 * reference's ray-traced path, shader/rt.glsl:73-79), so a skinned or morphed mesh reports only its rigid motion.  With the switch on they
 * are the positions of the previous frame:
 *   trhip_scene_set_deformation_motion(dev, on)  kept over uploads, like the acceleration-structure strategy.  On: allocates a plane
 *       float[vertices][3] parallel to the scene's vertex array (12 bytes next to the 48 of a vertex) and fills it from the current
 *       vertices, so until the first latch the motion is the rigid one; an upload while it is on reallocates and refills.  Off: frees it.
 *   trhip_scene_latch_positions(dev)  copies, for every vertex span that has a skin or morph targets (a shared span once; on a morphed and
 *       skinned instance its span, i.e. the skinned result), the positions as they stand in the scene into the plane.  Call it once per
 *       frame, before trhip_scene_morph / trhip_scene_skin: two skin calls in a frame then leave the motion alone, and a mesh that is
 *       not posed again gets previous = current.  Waits for the device first, as trhip_scene_skin does.  Static spans keep what the fill
 *       gave them.  With the switch off it succeeds and does nothing.
 *   trhip_scene_get_previous_positions(dev, instance, out, max_count)  reads back up to max_count float[3] of the instance's span of the
 *       plane; for tests and tools.  Refused: null output, no scene, an instance out of range, the switch off. */
int trhip_scene_set_deformation_motion(trhip_device* dev, int on);
int trhip_scene_latch_positions(trhip_device* dev);
int trhip_scene_get_previous_positions(trhip_device* dev, uint32_t instance, float* out_host, uint32_t max_count);
/* After trhip_scene_update_instances: keeps the topology of the last build and recomputes the world triangles, every
 * child box (level by level, bottom-up) and the tri lights - an acceleration-structure *update* instead of a build
 * (src/acceleration_structure.cc:376-422).  Results are identical to a rebuild; traversal gets slower as the
 * transforms drift from the ones the tree was built for. */
int trhip_scene_refit_accel(trhip_device* dev, trhip_accel_info* out);
/* Replaces vkCmdBuildAccelerationStructuresKHR (src/acceleration_structure.cc:198,266,421) with an
 * on-device build (pre-transform -> bounds -> Morton -> radix sort -> PLOC clustering -> 4-wide collapse) and
 * runs extract_tri_lights (shader/extract_tri_lights.comp:17-54).  Synchronous. */
int trhip_scene_build_accel(trhip_device* dev, trhip_accel_info* out);
/* What the reference tells the driver per mesh (src/acceleration_structure.cc:127-133): static geometry is built with
 * ePreferFastTrace, dynamic geometry with ePreferFastBuild | eAllowUpdate.  prefer_fast_build = 0 (the default):
 * trhip_scene_build_accel follows the clustering with tree-optimisation rounds (parallel reinsertion) and chooses the 4-wide
 * nodes by cost (csrc/bvh_optimize.h): 12 % fewer node visits per ray, 16 instead of 9 ms for a million triangles; != 0: it does
 * neither - for callers that rebuild every frame.  Hits, and therefore frames, do not depend on the choice. */
int trhip_scene_set_build_mode(trhip_device* dev, int prefer_fast_build);
/* How the acceleration structure is laid out (the reference's --as-strategy, scene_stage::options::group_strategy); takes effect at
 * the next trhip_scene_build_accel and is kept over uploads.
 *   TRHIP_AS_ALL_MERGED (the default): every instance's triangles pre-transformed into one tree - the structure and kernels of before.
 *   TRHIP_AS_PER_MESH: one BLAS per distinct mesh span (equal vertex_offset, vertex_count, index_offset and triangle_count), built in
 *     object space and shared by every instance of that span, under a TLAS over the instances.
 *   TRHIP_AS_STATIC_MERGED_DYNAMIC_PER_MESH: the static instances world-space in one merged BLAS under an identity TLAS leaf, the dynamic
 *     ones (trhip_scene_set_dynamic_instances, and every skinned instance) in per-mesh BLASes.
 * An instance here is one glTF primitive with one material, so the reference's `per-material` is TRHIP_AS_PER_MESH exactly, and its
 * `per-model` is TRHIP_AS_PER_MESH wherever a model has one primitive; its default `static-merged-dynamic-per-model` is
 * TRHIP_AS_STATIC_MERGED_DYNAMIC_PER_MESH.  Deviation: the default here stays `all-merged`, so that nothing existing changes.
 * Hits do not depend on the strategy beyond the rounding of the object-space ray (exact for identity transforms).  Under a two-level
 * strategy trhip_scene_refit_accel rebuilds the TLAS from the current transforms, refits the BLASes whose vertices were skinned and the
 * merged static BLAS only if a static instance's record changed: trhip_scene_update_instances + trhip_scene_refit_accel is the
 * reference's rigid-body update. */
#define TRHIP_AS_ALL_MERGED 0
#define TRHIP_AS_PER_MESH 1
#define TRHIP_AS_STATIC_MERGED_DYNAMIC_PER_MESH 2
int trhip_scene_set_accel_strategy(trhip_device* dev, int strategy);
/* Marks instances dynamic (1) or static (0): the reference's !static_mesh || !static_transformable.  `count` = the uploaded instance
 * count; an upload clears the marks.  Skinned instances are dynamic without a mark.  Takes effect at the next build. */
int trhip_scene_set_dynamic_instances(trhip_device* dev, const uint8_t* dynamic, uint32_t count);
typedef struct trhip_accel_layout {
    int32_t strategy;                 /* of the last build */
    uint32_t blas_count;              /* 1 for all-merged */
    uint32_t tlas_leaf_count;         /* 0 for all-merged */
    uint32_t blas_updated;            /* BLASes built or refit by the last build / refit call */
    uint64_t node_bytes;              /* 128-byte node slots of both levels */
    uint64_t record_bytes;            /* triangle records of every BLAS + the 64-byte instance records of the TLAS leaves */
    float blas_ms;                    /* device time of the last call's BLAS work (build or refit) */
    float tlas_ms;                    /* device time of the last TLAS build (0 for all-merged) */
} trhip_accel_layout;
int trhip_scene_get_accel_layout(trhip_device* dev, trhip_accel_layout* out);
/* Sphere lights in closest-hit rays.  The reference builds one AABB per point / spot light into a light BLAS under a TLAS instance of mask
 * 1 << 1 (src/scene_stage.cc:1356-1387, 1456-1466) and intersects it with shader/rt_common_point_light.rint:11-17, shader/rt_common.glsl:36-51,
 * so a closest-hit ray costs the logarithm of the light count.  Here the lights with radius != 0 get a 4-wide tree of their own, built on the
 * device at trhip_scene_upload (and when the mode below first asks for it) and walked after the triangles; trhip_scene_update_lights refits
 * it when the set of lights with a radius stays the same and rebuilds it otherwise, before it returns.  The tree lives behind the light
 * records, independent of trhip_scene_build_accel and of the acceleration-structure strategy.  Hits are bit-identical in every mode.
 *   TRHIP_LIGHT_ACCEL_AUTO (the default): the tree once at least `auto_threshold` lights have a radius, else the loop.
 *   TRHIP_LIGHT_ACCEL_LOOP: every light in a loop, the cost growing with the light count (what this library did before).
 *   TRHIP_LIGHT_ACCEL_TREE: the tree whenever a light has a radius.
 * The mode is kept over uploads.  Until it is set, the environment variable TRHIP_LIGHT_ACCEL=auto|loop|tree chooses it (A/B tools). */
#define TRHIP_LIGHT_ACCEL_AUTO 0
#define TRHIP_LIGHT_ACCEL_LOOP 1
#define TRHIP_LIGHT_ACCEL_TREE 2
int trhip_scene_set_light_accel(trhip_device* dev, int mode);
typedef struct trhip_light_accel_info {
    int32_t requested;                /* TRHIP_LIGHT_ACCEL_*: what was set (or TRHIP_LIGHT_ACCEL chose) */
    int32_t in_effect;                /* TRHIP_LIGHT_ACCEL_LOOP or TRHIP_LIGHT_ACCEL_TREE: what the closest-hit kernels run now */
    uint32_t sphere_lights;           /* point / spot lights with radius != 0 */
    uint32_t tree_lights;             /* leaves of the tree (0: no tree) */
    uint32_t node_count;              /* 128-byte node slots of the tree */
    uint32_t auto_threshold;          /* sphere lights from which TRHIP_LIGHT_ACCEL_AUTO uses the tree */
    uint64_t tree_bytes;              /* header + node slots behind the light records */
    float last_ms;                    /* host wall time of the last build or refit, device work included */
    int32_t last_was_refit;           /* 1: the last tree update was a refit, 0: a build, -1: none since the upload */
} trhip_light_accel_info;
int trhip_scene_get_light_accel(trhip_device* dev, trhip_light_accel_info* out);
/* copies the 64-byte tri_light records back to the host (test hook) */
int trhip_scene_get_tri_lights(trhip_device* dev, void* out_host, uint32_t max_count);

/* ---- path_tracer_stage (src/path_tracer_stage.{hh,cc}, src/rt_camera_stage.{hh,cc}, src/rt_stage.{hh,cc}) */
typedef struct trhip_pt_options {     /* == path_tracer_stage::options flattened (src/path_tracer_stage.hh:13-30) */
    int32_t max_bounces;              /* rt_stage::options::max_ray_depth -> MAX_BOUNCES */
    float min_ray_dist;
    uint32_t rng_seed;                /* raw option; pcg() applied if non-zero (src/rt_stage.cc:82) */
    int32_t sampler;                  /* rt_stage::sampler_type: 0 uniform-random, 1 sobol-owen, 2 sobol-z 2D, 3 sobol-z 3D */
    int32_t samples_per_pixel;
    int32_t samples_per_pass;
    int32_t projection;               /* camera::projection_type: 0 perspective, 1 orthographic, 2 equirectangular */
    int32_t film;                     /* film_filter: 0 point, 1 box, 2 blackman-harris */
    float film_radius;
    int32_t mis_mode;                 /* 0 disabled, 1 balance, 2 power */
    float russian_roulette_delta;
    float indirect_clamping;
    float regularization_gamma;
    int32_t depth_of_field;
    float nee_point, nee_directional, nee_envmap, nee_triangles;  /* light_sampling_weights; 0 disables the class */
    int32_t bounce_mode;              /* bounce_sampling_mode: 0 hemisphere, 1 cosine hemisphere, 2 material */
    int32_t tri_light_mode;           /* tri_light_sampling_mode: 0 area, 1 solid angle, 2 hybrid */
    int32_t hide_lights;
    int32_t use_white_albedo_on_first_bounce;
    int32_t transparent_background;
    int32_t pre_transformed_vertices; /* PRE_TRANSFORMED_VERTICES: shade from the world-space vertex copy of shader/pre_transform.comp (built on first use) */
} trhip_pt_options;

typedef struct trhip_distribution {   /* == distribution_params (src/distribution_strategy.hh:21-28) */
    uint32_t size_x, size_y;
    int32_t strategy;                 /* 0 duplicate, 1 scanline, 2 shuffled strips */
    uint32_t index, count;
    uint32_t primary;
} trhip_distribution;

typedef struct trhip_counters {       /* per trhip_pt, cumulative since the last reset */
    uint64_t closest_rays, shadow_rays;           /* rays actually traced (-> Mray/s) */
    uint64_t node_visits, tri_tests, alpha_tests, surface_hits;   /* only counted when counting is enabled */
    uint64_t stack_overflows;
} trhip_counters;

typedef struct trhip_timings {        /* hipEvent timers with the reference's stage names (src/timer.cc) */
    float path_tracing_ms;            /* "path tracing (N viewports)" of the last trhip_pt_render */
    /* Per-kernel device time, cumulative since the last trhip_pt_reset_counters; only collected while
     * detailed timing is on (event pairs around every launch, no host synchronisation). */
    float trace_closest_ms, trace_shadow_ms, shade_ms, raygen_ms, resolve_ms;
    uint32_t trace_closest_launches, trace_shadow_launches, shade_launches, frames;
} trhip_timings;

int trhip_pt_create(trhip_device* dev, const trhip_pt_options* opt, trhip_pt** out);   /* path_tracer_stage ctor */
/* direct_stage (src/direct_stage.{hh,cc}, shader/direct.rgen): the first hit of every pixel with sphere lights hidden plus
 * samples_per_pass light samples from it; no bounces.  Same handle type and the same calls as the path tracer (set
 * distribution, render, render_targets, counters, timings).  Of the options it reads the sampler, sample counts, film,
 * projection, light-sampling weights, bounce and tri-light modes, min_ray_dist and transparent_background; MIS, clamping,
 * regularisation and roulette do not apply (the reference sets no such defines for it) and max_bounces only sizes the
 * Sobol table. */
int trhip_direct_create(trhip_device* dev, const trhip_pt_options* opt, trhip_pt** out);
void trhip_pt_destroy(trhip_pt* pt);
int trhip_pt_set_distribution(trhip_pt* pt, const trhip_distribution* dist);  /* rt_camera_stage::reset_distribution_params */
int trhip_pt_reset_accumulation(trhip_pt* pt, int reset_sample_counter);      /* reset_accumulated_samples / reset_sample_counter */
/* rt_stage::frame_counter (src/rt_stage.cc:81-86) of the next frame: with one stage per frame slot, slot k of F renders
 * frames k, k + F, ... and sets the counter before each of them (sample_counter = frame_counter * samples_per_pixel). */
int trhip_pt_set_frame_counter(trhip_pt* pt, uint32_t frame_counter);
/* Several consecutive frames in one launch.  After trhip_pt_set_frame_batch(pt, B) a render call takes B * V layers (V = the
 * viewports of one frame) and renders frames f .. f + B - 1 of the stage's frame counter into them, frame-major: layer l is
 * viewport l % V of frame f + l / V, with exactly the samples a separate render call for that frame would have drawn; the frame
 * counter advances by B.  For frames that do not accumulate (offline frames: the caller resets the accumulation between them,
 * src/tauray.cc:1101).  What it is for: a rank of a pixel-sharded multi-GPU job traces an eighth of a frame per call, launches
 * that are too small to fill the chip; four frames per launch cost 12 % less per frame. */
int trhip_pt_set_frame_batch(trhip_pt* pt, uint32_t frames);
/* How many slices of a frame the stage runs concurrently on its own streams: 0 = automatic
 * (by frame size: four lanes from 200 k paths, two from 100 k, each on a hardware pipe of its own - and by trhip_pt_set_frame_slots:
 * two lanes per stage with two slots, one with more), 1 = everything on the caller's stream. */
int trhip_pt_set_lanes(trhip_pt* pt, int lanes);
/* A hint from a renderer with frame slots (MAX_FRAMES_IN_FLIGHT stages of the same scene, src/context.hh:26): how many stages render
 * next to this one on the device.  The stage sizes its persistent launches by it - with two or three frames in flight a trace launch of
 * three blocks per CU leaves the room the neighbours need (two slots: -0 ... 5 %, three: -3 ... 5 %), with four or more the larger grids
 * stay (profiles/r5/frame_slot_grids.txt).  0 (the default) = unknown.  Frames are the same bits whatever the hint. */
int trhip_pt_set_frame_slots(trhip_pt* pt, int slots);
/* The schedule of the stage's last render: how many lanes it ran (1 ... 4) and the hardware pipe class (trhip_stream_pipe_class) of each
 * lane's stream, the caller's stream first.  Lanes on one pipe would have run one after the other. */
int trhip_pt_get_lane_pipes(trhip_pt* pt, int32_t* lanes_out, int32_t pipe_classes_out[4]);
/* View and sample sharding across devices (the reference itself only shards pixels,
 * src/distribution_strategy.cc).  Local layer l of the target shows viewport viewport_base + l * viewport_stride: that
 * viewport's camera (shader/scene.glsl:176-185) and its RNG stream (the viewport index seeds the sampler,
 * shader/sampling.glsl:32-45).  Local sample s of a frame is sample sample_base + s * sample_stride of the pixel's
 * sequence, out of samples_per_pixel * sample_stride per frame (every shard takes the same number).  With these a
 * shard's pixels are the ones a single device renders for that viewport / those samples.  Defaults 0, 1, 0, 1. */
int trhip_pt_set_shard(trhip_pt* pt, uint32_t viewport_base, uint32_t viewport_stride, uint32_t sample_base, uint32_t sample_stride);
/* One frame: update() + every pass of record_command_buffer_pass (src/path_tracer_stage.cc:118-147).
 * `color` is the device RGBA32F image2DArray [viewports][target_h][target_w] where target size is
 * get_distribution_target_size(dist) (src/distribution_strategy.cc:6-19). */
int trhip_pt_render(trhip_pt* pt, void* color_dev, uint32_t target_w, uint32_t target_h, uint32_t viewports, void* stream);
/* The same frame into any subset of the gbuffer targets path_tracer.rgen writes (write_all_outputs,
 * shader/path_tracer.glsl:535-576; gbuffer_target of src/gbuffer.hh): device images [viewports][target_h][target_w],
 * null = not requested.  color / diffuse / reflection are running means over the accumulated samples
 * (shader/gbuffer.glsl:18-28,68-78,118-128); diffuse and reflection are the demodulated light of material.glsl:66-73
 * with a = 1/length of the second path segment.  albedo, material (metallic, roughness, ior/4, transmittance:
 * gbuffer.glsl:256-260), normal (octahedral, math.glsl:480-485), pos and instance_id describe the first hit and are
 * written by the first sample only. */
typedef struct trhip_pt_targets {
    void* color;        /* RGBA32F */
    void* diffuse;      /* RGBA32F */
    void* reflection;   /* RGBA32F */
    void* albedo;       /* RGBA32F */
    void* material;     /* RGBA32F */
    void* normal;       /* RG32F   */
    void* pos;          /* RGBA32F, world space, w = 0 */
    void* instance_id;  /* R32I, -1 = no surface */
    void* screen_motion;/* RG32F: get_camera_projection(previous camera, previous position).xy (shader/camera.glsl:61-67) */
} trhip_pt_targets;
int trhip_pt_render_targets(trhip_pt* pt, const trhip_pt_targets* targets, uint32_t target_w, uint32_t target_h, uint32_t viewports, void* stream);
/* Arithmetic of the shading kernel.  The reference's GLSL runs at the accuracy Vulkan asks of an implementation (SPIR-V
 * precision requirements: `/` 2.5 ULP, inversesqrt 2 ULP, sin / cos 2^-11 absolute, pow through exp2 and log2), and so do the
 * shading kernels here by default (csrc/shade_fast.hip, csrc/shade_spec.hip: v_rcp / v_rsq / v_sqrt /
 * v_sin / v_cos / v_exp / v_log).  ieee != 0: every shading kernel of this stage computes in IEEE fp32 with the C library's
 * sin / cos / pow, expression by expression like the CPU oracle - slower (1.22 instead of 0.97 ms per 1080p frame of the
 * million-triangle bench scene), for comparisons that want the last bit.  Ray traversal and the ray-triangle test are IEEE
 * fp32 in either mode: hits do not depend on it.  The environment variable TRHIP_SHADE_FAST=0 makes ieee the default. */
int trhip_pt_set_shading_arithmetic(trhip_pt* pt, int ieee);
/* Shading program of the stage.  The reference compiles a stage's options into its pipeline as #defines when the stage is built
 * (src/path_tracer_stage.cc:30-116, shaderc at run time through src/shader_source.cc).  Here the ray generation and shading
 * kernels exist ahead of time for the command-line option set and in a general form that reads every option as data; a stage
 * with any other option set gets a program compiled for it the first time it renders (csrc/shade_spec.hip through hipRTC: the
 * sampler, film filter, MIS rule, bounce and triangle-light modes, the light classes in use and the on / off state of roulette,
 * clamping, regularisation, depth of field ... become constants; a few seconds once, then the kernel cache -
 * trhip_kernel_cache_dir - serves it).  Same bits as the general kernels of the same arithmetic, fewer instructions.
 * enable: 1 = specialise (the default unless TRHIP_SPECIALIZE=0), 0 = always the general kernels.  If no program can be built
 * (no libhiprtc) the stage renders with the general kernels and says so once on stderr. */
int trhip_pt_set_specialization(trhip_pt* pt, int enable);
/* Compiles the programs of an option set into the kernel cache ahead of time, so that the first frame does not wait for
 * the compiler: ray generation and shading, for `arch` (NULL = "gfx950"); shade_tris = the scene will have whole-triangle
 * index spans (what trhip_scene_upload derives ShadeTri records from - true for every glTF file), ieee / count_work as in
 * trhip_pt_set_shading_arithmetic / trhip_pt_set_profiling.  Needs no GPU and no device handle. */
int trhip_pt_precompile(const trhip_pt_options* opt, int shade_tris, int ieee, int count_work, const char* arch);
/* Which shading program renders this stage, resolved now (a program for the option set is loaded from the kernel cache or compiled, as the
 * first render would do): the reference compiles one pipeline per stage from its options (src/path_tracer_stage.cc:30-116) and every
 * device of a job gets the same one.  Here a stage can end up on three kinds of kernels, and at the default arithmetic two kinds are two
 * implementations inside Vulkan's accuracy, not the same bits - so the ranks of a multi-GPU job compare
 * `identity` before the first frame (tr::process_rt_renderer, tauray_amd.renderer.RtRenderer: all-gather, mismatch = error) and
 * bench.py records `kind` instead of inferring it from the options.
 *   kind: 0 = the general kernels (every option read from the parameter block), 1 = the ahead-of-time instances of the reference's
 *         command-line option set, 2 = a program compiled for this option set (hipRTC / kernel cache);
 *   ieee: 1 = IEEE fp32 shading, 0 = Vulkan-grade arithmetic;
 *   identity: FNV-1a over kind, arithmetic, the pinned option fields, the embedded device sources of this build of the library, the
 *         build's id (trhip_build_id: every source of csrc/ and the compile flags, so two builds whose ahead-of-time kernels differ - kinds
 *         0 and 1 live in path_tracer.o / shade_fast.o, not in the embedded sources - differ here too) and, for kind 2, the bytes of the
 *         code objects that were loaded;
 *   key: the pinned fields as text (what TRHIP_DEBUG prints). */
typedef struct trhip_program_info { int32_t kind, ieee; uint64_t identity; char key[240]; } trhip_program_info;
int trhip_pt_get_program(trhip_pt* pt, trhip_program_info* out);
uint64_t trhip_build_id(void);              /* 64 bits of SHA-256 over the library's sources and compile flags, fixed when it was built */
const char* trhip_kernel_cache_dir(void);   /* TRHIP_KERNEL_CACHE, else kernel_cache/ next to libtrhip.so, else ~/.cache/trhip; "" = none writable */
int trhip_pt_set_profiling(trhip_pt* pt, int count_work, int detailed_timing);
int trhip_pt_get_counters(trhip_pt* pt, trhip_counters* out);     /* synchronises the stream */
int trhip_pt_reset_counters(trhip_pt* pt);
int trhip_pt_get_timings(trhip_pt* pt, trhip_timings* out);       /* synchronises the stream */
/* Wave-level statistics of the closest-hit loop, cumulative like trhip_counters and only collected while work counting is on
 * (trhip_pt_set_profiling): how many node / triangle phases the waves executed one ray per lane and one ray per quad
 * (csrc/trace_quad.h), and the per-lane node phases by the number of live rays (1-8, 9-16, ..., 57-64).  node_visits divided by
 * the node phases is the number of rays one vector instruction of the traversal serves - what the VALU roofline of bench.py
 * multiplies the issue rate with (a hardware lane count cannot tell a quad's four lanes from four rays). */
typedef struct trhip_phase_counters {
    uint64_t lane_node_phases, lane_tri_phases, quad_node_phases, quad_tri_phases;
    uint64_t lane_node_phases_le16, lane_node_visits_le16;
    uint64_t lane_node_phase_hist[8];
    uint64_t closest_node_visits;     /* node visits of the closest-hit rays alone (trhip_counters::node_visits includes shadow rays) */
} trhip_phase_counters;
int trhip_pt_get_phase_counters(trhip_pt* pt, trhip_phase_counters* out);   /* synchronises the stream */
/* Sphere-light work of the closest-hit rays (trhip_scene_set_light_accel), cumulative like trhip_counters, only counted while work counting
 * is on and cleared by trhip_pt_reset_counters: ray-sphere tests, node visits of the light tree (0 under TRHIP_LIGHT_ACCEL_LOOP), and walks
 * that ran out of their 16-entry stack and tested every light in the loop instead (same hits, the loop's cost). */
typedef struct trhip_light_counters { uint64_t sphere_tests, node_visits, walk_fallbacks; } trhip_light_counters;
int trhip_pt_get_light_counters(trhip_pt* pt, trhip_light_counters* out);   /* synchronises the stream */
/* The deepest per-ray traversal stack (entries, the one in a register included) that a trace launch has reached since the counters were
 * last cleared; kept while work counting is on.  The first 1 + 16 entries of a ray live in a register and LDS, deeper ones in the spill
 * memories (csrc/trace.h LaneStack), so a value above 17 says that the frames so far exercised those. */
int trhip_pt_get_max_stack_depth(trhip_pt* pt, uint32_t* out);              /* synchronises the stream */
/* The last bounce as a first-hit emitter query.  Every path ends at bounce max_bounces - 1, where a surface hit can
 * only add the emission of what was hit, so the last ray of a path needs to know whether it escapes, whether the nearest thing along it is
 * an emitter triangle, or that something else is in the way - and then neither what nor where.
 *   TRHIP_TERMINAL_QUERY_AUTO (the default): the launches of that bounce are the query while the structure is all-merged, max_bounces >= 2,
 *     the scene has at most `threshold` emitter triangles and no sphere light with a radius; otherwise, and under
 *   TRHIP_TERMINAL_QUERY_OFF, they are the closest-hit launches of every other bounce.
 * Frames, ray counts and surface-hit counts do not depend on the mode.  Until it is set, TRHIP_TERMINAL_QUERY=auto|off chooses it
 * (A/B tools; any other value fails trhip_pt_render). */
#define TRHIP_TERMINAL_QUERY_AUTO 0
#define TRHIP_TERMINAL_QUERY_OFF 1
int trhip_pt_set_terminal_query(trhip_pt* pt, int mode);
/* in_effect: what the stage's next frame does.  blocked_rays / fallback_rays: rays of the query that ended at something in front of the
 * nearest emitter, and rays it traced as ordinary closest hits because their path state fails the query's range check; cumulative like
 * trhip_counters, only counted while work counting is on, cleared by trhip_pt_reset_counters. */
typedef struct trhip_terminal_counters { uint64_t blocked_rays, fallback_rays; uint32_t in_effect, emitter_triangles, threshold, pad; } trhip_terminal_counters;
int trhip_pt_get_terminal_counters(trhip_pt* pt, trhip_terminal_counters* out);   /* synchronises the stream */
/* The primary start: how the paths of a pass start.  A path's start - camera ray, sampler state, any-hit seed, Sobol
 * index - is a function of its launch id, the frame parameters and the camera.
 *   TRHIP_PRIMARY_START_AUTO (the default): a pass launches no ray generation kernel.  The closest-hit launch of bounce 0 computes the start
 *     in the lanes that trace the ray and stores the path state for the kernels behind it; the queue lengths and work cursors of a lane are
 *     zeroed by the resolve launch of the pass before.  In effect for a path-tracer stage that renders
 *     the command-line option set with the ahead-of-time kernels (trhip_pt_get_program: kind 1) over an all-merged structure, with
 *     samples_per_pass == 1, while neither work counting nor detailed timing is on (trhip_pt_set_profiling); not for a probe stage or the
 *     direct stage.  Otherwise, and under
 *   TRHIP_PRIMARY_START_OFF, every pass starts with the ray generation launch (one for all lanes of a short frame).
 * Frames and ray counts do not depend on the mode; it may change between frames.  Until it is set, TRHIP_PRIMARY_START=auto|off chooses it
 * (A/B tools; any other value fails trhip_pt_render). */
#define TRHIP_PRIMARY_START_AUTO 0
#define TRHIP_PRIMARY_START_OFF 1
int trhip_pt_set_primary_start(trhip_pt* pt, int mode);
/* mode: what was set (-1: nothing, the environment decides).  in_effect: what the stage's next frame does.  last_frame: what the last frame
 * rendered did (-1: none yet). */
typedef struct trhip_primary_start_info { int32_t mode, in_effect, last_frame, pad; } trhip_primary_start_info;
int trhip_pt_get_primary_start(trhip_pt* pt, trhip_primary_start_info* out);
/* Peak vector-instruction issue rate of the device as it runs now: a loop of independent v_fma_f32 at eight waves per SIMD,
 * in 10^9 wave-level instructions per second (MI355X_MICROARCH.md: 2 cycles per wave64 instruction on a SIMD-32; the clock is
 * what the box sustains).  The peak of the VALU roofline in bench.py; about 2 ms of device time. */
int trhip_calibrate_valu(trhip_device* dev, float* ginst_per_s);
/* Peak rate at which the vector L1 caches (TCP, one per CU) take cache-line accesses, in 10^9 accesses per second over the device:
 * independent 16-byte loads out of an L1-resident footprint, every lane of a wave in a 128-byte line of its own (64 accesses per
 * wave instruction).  One access per clock and CU (tools/ubench/l1_tags.hip, profiles/r3/l1_tag_rate.json) - what the counter
 * TCP_TOTAL_CACHE_ACCESSES counts, and the peak of the L1 level of bench.py's roofline: a traversal step reads its node with seven
 * loads per lane, seven accesses to one line.  About 1 ms of device time. */
int trhip_calibrate_l1(trhip_device* dev, float* gaccesses_per_s);

/* ---- feature_stage (src/feature_stage.cc:22-104): 0 albedo, 1 world normal, 2 view normal, 3 world pos,
 *      4 view pos, 5 distance, 6 world motion, 7 view motion, 8 screen motion, 9 instance id */
int trhip_feature_render(trhip_device* dev, int feature, const trhip_distribution* dist, int projection,
                         uint32_t viewport, float min_ray_dist, const float default_value[4],
                         void* color_dev, uint32_t target_w, uint32_t target_h, void* stream);

/* ---- ray-level queries (parity hooks for traceRayEXT, shader/path_tracer.glsl:38-50,387-403).
 * rays: 8 floats each {ox, oy, oz, tmin, dx, dy, dz, tmax}; hits: {i32 instance, i32 primitive, f32 u, f32 v, f32 t}.
 * seeds == NULL selects the feature renderer's fixed alpha cutoff (shader/rt_feature.rahit:17). */
/* Two queries on one device must not run at the same time (the closest-hit query keeps one spill buffer for the deep stack
 * entries of its quad tails per device): enqueue them on one stream, or order the streams with trhip_stream_wait. */
int trhip_trace_closest(trhip_device* dev, uint32_t n, const void* rays_dev, const void* seeds_dev,
                        int include_lights, void* hits_dev, void* stream);
/* The terminal query (trhip_pt_set_terminal_query) for a list of rays: hits as above, except that a ray with an accepted hit in front of
 * its nearest accepted emitter triangle reports instance -2 and nothing else (blocked).  fallback: NULL, or one uint32 per ray, nonzero =
 * trace this ray as an ordinary closest hit (what a frame does with a path outside the query's range check).  Fails unless the structure
 * is all-merged and holds at most the threshold's emitter triangles; sphere lights are not looked at. */
int trhip_trace_terminal(trhip_device* dev, uint32_t n, const void* rays_dev, const void* seeds_dev, const void* fallback_dev,
                         void* hits_dev, void* stream);
int trhip_trace_shadow(trhip_device* dev, uint32_t n, const void* rays_dev, void* visibility_dev, void* stream);

/* ---- stitch_stage (src/stitch_stage.cc:128-196, shader/stitch_scanline.comp, stitch_shuffled_strips.comp).
 * Scatters one non-primary device's partial image into the primary (full-size) image. */
int trhip_stitch(trhip_device* dev, const trhip_distribution* partial_dist, const void* partial_dev,
                 uint32_t partial_w, uint32_t partial_h, void* primary_dev, uint32_t viewports,
                 float blend_ratio, void* stream);
/* The partial images of all non-primary devices in one launch (the reference dispatches the stitch shader once per
 * device, src/stitch_stage.cc:150-196): `count` entries of what trhip_stitch takes.  With blend_ratio < 1 the partials
 * must not overlap, which the distribution strategies guarantee. */
int trhip_stitch_batch(trhip_device* dev, uint32_t count, const trhip_distribution* partial_dists, const void* const* partials_dev,
                       const uint32_t* partial_ws, const uint32_t* partial_hs, void* primary_dev, uint32_t viewports,
                       float blend_ratio, void* stream);

/* ---- tonemap_stage (src/tonemap_stage.cc:139-164, shader/tonemap*.comp) */
typedef struct trhip_tonemap_info {
    int32_t op;                       /* tonemap_stage::operator_type: 0 linear, 1 gamma, 2 filmic, 3 reinhard, 4 reinhard luminance */
    float exposure, gamma;
    int32_t alpha_grid_background;    /* 0 or grid size (16 when not headless) */
} trhip_tonemap_info;
int trhip_tonemap(trhip_device* dev, const void* in_dev, void* out_dev, uint32_t width, uint32_t height,
                  uint32_t layers, const trhip_tonemap_info* info, void* stream);
/* A renderer with nothing between its path tracer and its tonemap stage (one device, no stitch, no denoiser: rt_renderer with one
 * device, src/rt_renderer.cc) can have the stage's last pass write the display image as it writes the colour target: `display_dev`
 * (same width x height x layers as the colour target, RGBA32F) receives trhip_tonemap(colour) pixel by pixel, the same bits, without the
 * second pass over the frame (a 1080p frame: 47 us after the last lane has finished).  NULL turns it off.  Path tracer stages only. */
int trhip_pt_set_fused_tonemap(trhip_pt* pt, void* display_dev, const trhip_tonemap_info* info);

/* ---- bmfr_stage (src/bmfr_stage.{hh,cc}, shader/bmfr_*.comp; --denoiser=bmfr, src/post_processing_renderer.cc:53-106): blockwise
 * multi-order feature regression between the path tracer and the tonemap stage.  Per frame: (a) temporal accumulation of the noisy
 * diffuse / specular light by reprojection through screen_motion, and the feature rows 1, n, p, p^2 of every 32 x 32 block of a grid
 * that is shifted per frame; (b) a least-squares fit of the ten features to the noisy channels per block (Householder QR); (c) the
 * fitted values per pixel; (d) temporal accumulation of the fitted values and colour = albedo * diffuse + specular.  csrc/bmfr.hip.
 * The images are the targets of trhip_pt_render_targets (RGBA32F / RG32F / R32I, [layers][height][width]); every intermediate -
 * histories of noisy and filtered values, last frame's normal and pos, feature rows, weights, min / max, accept bits - is fp32, owned
 * by the stage and sized when it is created.  Deviations from the reference: the 16 block offsets are this
 * stage's own table; the noise of the fit is a counter-based hash of (block-grid pixel, layer, feature, frame) instead of a
 * per-thread stream; a pixel with instance_id < 0 is "no surface" like one whose pos is NaN (its colour passes through, its row
 * stays out of the fit). */
typedef struct trhip_bmfr trhip_bmfr;
#define TRHIP_BMFR_DIFFUSE_ONLY 0          /* bmfr_stage::bmfr_settings: fit the diffuse light, pass the accumulated specular through */
#define TRHIP_BMFR_DIFFUSE_SPECULAR 1      /* fit both */
typedef struct trhip_bmfr_options {
    int32_t settings;                 /* TRHIP_BMFR_DIFFUSE_ONLY (what --denoiser=bmfr selects) or TRHIP_BMFR_DIFFUSE_SPECULAR */
    float noise_amount;               /* amplitude of the noise added to features 1-9 before the fit; 0 = the reference's 1e-2 */
} trhip_bmfr_options;
typedef struct trhip_bmfr_features {  /* the gbuffer entries the stage reads (src/bmfr_stage.cc:196-240) */
    void* color;                      /* RGBA32F in: noisy, out: denoised */
    void* diffuse;                    /* RGBA32F */
    void* albedo;                     /* RGBA32F */
    void* normal;                     /* RG32F   */
    void* pos;                        /* RGBA32F */
    void* screen_motion;              /* RG32F   */
    void* instance_id;                /* R32I, may be NULL: then only a NaN pos marks "no surface" */
} trhip_bmfr_features;
typedef struct trhip_bmfr_timings {   /* the reference's timer names (src/bmfr_stage.cc), device ms of the last frame */
    float preprocess_ms, fit_ms, weighted_sum_ms, accumulate_output_ms, total_ms;
    uint32_t frames;                  /* frames run since the stage was created */
} trhip_bmfr_timings;
int trhip_bmfr_create(trhip_device* dev, const trhip_bmfr_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_bmfr** out); /* bmfr_stage ctor */
void trhip_bmfr_destroy(trhip_bmfr* bmfr);
/* bmfr_stage::run: one frame, asynchronous on `stream`, no synchronisation.  frame_counter (context::get_frame_counter) picks the block
 * offset (frame_counter % 16) and seeds the noise.  Frames of one stage form one history: run them in frame order on one stream (or
 * on streams ordered with trhip_stream_wait). */
int trhip_bmfr_run(trhip_bmfr* bmfr, const trhip_bmfr_features* features, uint32_t frame_counter, void* stream);
int trhip_bmfr_reset_history(trhip_bmfr* bmfr);   /* camera cut / new scene: the next frame has no history, like a new stage's first */
int trhip_bmfr_get_timings(trhip_bmfr* bmfr, trhip_bmfr_timings* out);   /* waits for the last frame */
/* Parity hooks, as trhip_trace_closest is for traceRayEXT.  trhip_bmfr_fit_blocks: the fit of (b) alone on `blocks` matrices
 * [blocks][10 + channels][1024] (column-major per block: ten feature columns, already scaled and with noise, then the channels;
 * channels = 3 or 6) -> weights [blocks][channels][10].  trhip_bmfr_download: a buffer of the stage as the last frame left it
 * (synchronises the device); `bytes` must be the buffer's size. */
int trhip_bmfr_fit_blocks(trhip_device* dev, uint32_t blocks, uint32_t channels, const float* matrix_dev, float* weights_dev, void* stream);
#define TRHIP_BMFR_NOISY_DIFFUSE 0         /* RGBA32F [layers][h][w], a = history length */
#define TRHIP_BMFR_NOISY_SPECULAR 1        /* RGBA32F */
#define TRHIP_BMFR_FILTERED_DIFFUSE 2      /* RGBA32F, a = history length */
#define TRHIP_BMFR_FILTERED_SPECULAR 3     /* RGBA32F, DIFFUSE_SPECULAR only */
#define TRHIP_BMFR_FEATURE_ROWS 4          /* float [blocks][10 + channels][1024], unscaled, without noise; blocks = layers * (ceil(h/32)+1) * (ceil(w/32)+1) */
#define TRHIP_BMFR_WEIGHTS 5               /* float [blocks][channels][10] */
#define TRHIP_BMFR_MIN_MAX 6               /* float [blocks][6][2]: min, max of features 4-9 */
#define TRHIP_BMFR_ACCEPT_BITS 7           /* uint8 [layers][h][w]: bits 0-3 the taps kept (tl, tr, bl, br), bit 4 no surface */
#define TRHIP_BMFR_BLOCK_OFFSETS 8         /* int32 [16][2]: the table frame_counter % 16 indexes (needs no device) */
#define TRHIP_BMFR_PREVIOUS_NORMAL 9       /* RG32F: the normal target of the last frame */
#define TRHIP_BMFR_PREVIOUS_POS 10         /* RGBA32F: the pos target of the last frame, w = 1 where it had no surface */
int trhip_bmfr_download(trhip_bmfr* bmfr, int which, void* host, size_t bytes);

/* ---- sparse light fields (--spatial-reprojection=i,j,... / --temporal-reprojection=r; src/spatial_reprojection_stage.{hh,cc},
 * src/temporal_reprojection_stage.{hh,cc}, shader/spatial_reprojection.comp, shader/temporal_reprojection.comp).  Only the listed
 * viewports of a camera grid are path traced; the others are filled from them through the G-buffer.  csrc/reprojection.hip.
 * Frame order: path tracer (the sources) -> temporal stage on the sources -> trhip_gbuffer_render (the other viewports) -> spatial stage
 * -> tonemap.  All images are fp32 device images [layers][height][width]. */
typedef struct trhip_gbuffer_targets {
    void* normal;       /* RG32F, octahedral (math.glsl:480-485) */
    void* pos;          /* RGBA32F, world space, w = 0 */
    void* instance_id;  /* R32I, -1 = no surface */
} trhip_gbuffer_targets;
/* The first hit of one ray through every pixel centre of `count` viewports in one launch: compact layers [count][height][width] in the
 * order of `viewports` (any order, repeats allowed); null targets are not written.  pos.xyz and instance_id are what
 * trhip_feature_render features 3 and 9 give for that viewport with a duplicate distribution, bit for bit, normal is the packing of
 * feature 1; a miss writes the ray origin, the packed -direction and -1, as the targets of trhip_pt_render_targets do.  Both
 * acceleration-structure layouts. */
int trhip_gbuffer_render(trhip_device* dev, int projection, const uint32_t* viewports, uint32_t count, float min_ray_dist,
                         const trhip_gbuffer_targets* targets, uint32_t width, uint32_t height, void* stream);
typedef struct trhip_reprojection_images {
    void* color;         /* RGBA32F */
    void* normal;        /* RG32F   */
    void* pos;           /* RGBA32F */
    void* instance_id;   /* R32I    */
    void* screen_motion; /* RG32F, the temporal stage only */
} trhip_reprojection_images;
typedef struct trhip_reprojection_timings { float total_ms; uint32_t frames; } trhip_reprojection_timings;   /* device ms of the last frame's kernel */
/* spatial_reprojection_stage.  Per output pixel of viewport v (natural order):
 *   v is a source: its colour, bit for bit.
 *   a destination with a surface: pos is projected with every source's view_proj (the scene's current cameras, read on the device when
 *     the kernel runs).  The candidate is the source with the smallest z/w below 1 (ties: the first).  A try of source s takes the four
 *     taps at floor(uv * size - 0.5), uv = (xy/w * 0.5 + 0.5, y -> 1 - y); a tap is kept when it is inside the image, has a surface,
 *     dot(n_tap, n) > 0.99 and |pos - pos_tap|^2 < 0.01; the bilinear weights are renormalised over the kept taps and the try succeeds
 *     when the kept weight exceeds 1e-5.  The candidate is tried first; if it fails the other sources are tried in list order, each only
 *     if its depth is below the best accepted so far (below 1 while none is).  Nothing accepted: default_value (the hosts pass NaN).
 *   a destination without a surface: the same pixel of the first source that has no surface there either, else default_value.
 * Deviations from the reference: (1) the tap origin is floor(), where the reference truncates towards zero;
 * (2) a source with w <= 0 is skipped; (3) "no surface" is a NaN pos or instance_id < 0, as in the BMFR stage; (4) the sources are named
 * by a list and the output is in natural viewport order, instead of "the first N layers" and a reorder mask in the tonemap stage;
 * (5) every image is fp32.  view_proj is used as it is: perspective and orthographic cameras. */
typedef struct trhip_spatial_reprojection trhip_spatial_reprojection;
int trhip_spatial_reprojection_create(trhip_device* dev, uint32_t width, uint32_t height, uint32_t total_viewports, const uint32_t* source_viewports,
                                      uint32_t source_count, const float default_value[4], trhip_spatial_reprojection** out);
void trhip_spatial_reprojection_destroy(trhip_spatial_reprojection* stage);
/* sources: {color, normal, pos, instance_id} [source_count] layers in the order of source_viewports; destinations: {normal, pos,
 * instance_id} of the other viewports in ascending order; color_out: RGBA32F [total_viewports][height][width].  Asynchronous on `stream`. */
int trhip_spatial_reprojection_run(trhip_spatial_reprojection* stage, const trhip_reprojection_images* sources,
                                   const trhip_reprojection_images* destinations, void* color_out, void* stream);
int trhip_spatial_reprojection_get_timings(trhip_spatial_reprojection* stage, trhip_reprojection_timings* out);   /* waits for the last frame */
/* Decision record, 8 bytes per pixel: u8 kind (0 none, 1 reprojected, 2 no-surface copy), u8 source slot, u8 keep bits (tl, tr, bl, br),
 * u8 zero, i16 x 2 tap origin.  Spatial: [destinations][h][w]; temporal: [layers][h][w].  Downloads synchronise the device. */
#define TRHIP_REPROJECTION_DECISIONS 0
#define TRHIP_REPROJECTION_PREVIOUS_COLOR 1     /* temporal: RGBA32F, the colour the last frame left */
#define TRHIP_REPROJECTION_PREVIOUS_NORMAL 2    /* temporal: RG32F */
#define TRHIP_REPROJECTION_PREVIOUS_POS 3       /* temporal: RGBA32F, w = 1 where it had no surface */
int trhip_spatial_reprojection_download(trhip_spatial_reprojection* stage, int which, void* host, size_t bytes);
/* temporal_reprojection_stage, in front of the spatial stage on the path-traced layers: the taps above at screen_motion in the previous
 * frame's normal / pos / colour, color = mix(color, reprojected, ratio); the pixel stays as it is when no tap is kept or the result has
 * a NaN.  A no-surface pixel keeps its colour and is never a tap.  After the blend the frame's colour, normal and pos become the
 * stage's history (two copies, ping-pong); the first frame after create or reset_history only stores it.  ratio in (0, 1). */
typedef struct trhip_temporal_reprojection trhip_temporal_reprojection;
int trhip_temporal_reprojection_create(trhip_device* dev, uint32_t width, uint32_t height, uint32_t layers, float ratio, trhip_temporal_reprojection** out);
void trhip_temporal_reprojection_destroy(trhip_temporal_reprojection* stage);
/* images: {color in/out, normal, pos, screen_motion, instance_id or NULL}.  Asynchronous on `stream`; frames of one stage form one history. */
int trhip_temporal_reprojection_run(trhip_temporal_reprojection* stage, const trhip_reprojection_images* images, void* stream);
int trhip_temporal_reprojection_reset_history(trhip_temporal_reprojection* stage);
int trhip_temporal_reprojection_get_timings(trhip_temporal_reprojection* stage, trhip_reprojection_timings* out);
int trhip_temporal_reprojection_download(trhip_temporal_reprojection* stage, int which, void* host, size_t bytes);

/* ---- taa_stage (--taa=N; src/taa_stage.{hh,cc}, shader/taa.comp): temporal antialiasing behind the tonemap stage, the last stage of
 * denoiser -> tonemap -> taa (src/post_processing_renderer.cc:79-106).  csrc/taa.hip, one kernel per frame; the order of operations is
 * pinned in csrc/taa.h.  The hosts give every camera a sub-pixel jitter sequence (pan.zw of camera_data holds the frame's jitter); per
 * output pixel p of layer z, with camera pair (cameras, previous cameras)[base_camera_index + z] of the device's scene as it is when the
 * kernel runs:
 *   1. col = src[p]; map(c) = c^gamma per rgb channel (exp2(gamma * log2(c)), c <= 0 -> 0), under anti_shimmer then c > 1e-5 ? log(c) : -10
 *   2. the ranges of the mapped 3 x 3 window along the 11 axes of the reference's 22-DOP, widened by 1e-5
 *   3. edge_dilation: the window pixel nearest to the camera (depth = dot(pos - origin, forward), strict <, x outer, y inner)
 *   4. motion = screen_motion of that pixel; where it has no surface and the camera is perspective, the previous camera's projection of
 *      the primary ray direction through the centre of p
 *   5. motion += (previous.pan.zw - current.pan.zw) / 2; uv = (motion.x, 1 - motion.y) - offset / size; outside [0, 1 + 2 / size]:
 *      dst = history = col
 *   6. the history at uv through the reference's bicubic filter (Catmull-Rom, twelve clamped-to-edge texels), max(., 0)
 *   7. map(history) is clipped towards map(col) onto the k-DOP, mixed with map(col) by alpha, unmapped; alpha passes through from src.
 *      alpha is 1 on the first frame and after reset_history.
 * Deviations from the reference: (1) the two history images are fp32 (fp16 there); (2) the depth comes from the pos
 * target instead of a depth target; (3) "no surface" is instance_id < 0 (without instance_id: a NaN screen_motion, as in the shader, and
 * every pixel has a depth); (4) a neighbour outside the image is skipped in the depth search (the reference clamps the depth read but then
 * reads screen_motion out of bounds there); (5) the fraction of the bicubic filter's bilinear fetches is used as computed instead of
 * going through a texture coordinate (which loses about 1e-4 of it at 1920 columns); (6) an orthographic miss keeps its written motion
 * (the previous camera's projection of the ray origin; the reference's formula divides by w = 0 there); (7) the unused `rounding` push
 * constant is dropped; (8) a NaN position counts as reprojected outside.  A NaN in one axis of the clip (0 * inf where a large colour
 * absorbs the 1e-5) is dropped by fminf / fmaxf instead of deciding the clip. */
typedef struct trhip_taa trhip_taa;
typedef struct trhip_taa_options {
    float alpha;                      /* weight of the new frame, in (0, 1]; the hosts pass 1 / sequence length */
    float gamma;                      /* of the colour map; the hosts pass the tonemap stage's */
    int32_t edge_dilation, anti_shimmer;
    uint32_t base_camera_index;       /* layer z reads camera pair base_camera_index + z */
    int32_t projection;               /* 0 perspective, 1 orthographic; 2 (equirectangular) is refused */
} trhip_taa_options;
typedef struct trhip_taa_images {
    const void* src;                  /* RGBA32F display-space colour */
    void* dst;                        /* RGBA32F; may equal src (then it is copied from the new history after the kernel), else must not overlap it */
    const void* screen_motion;        /* RG32F */
    const void* pos;                  /* RGBA32F, required with edge_dilation */
    const void* instance_id;          /* R32I, may be NULL */
} trhip_taa_images;
typedef struct trhip_taa_timings {    /* the reference's timer, device ms of the last frame */
    float total_ms;
    uint32_t frames;                  /* frames run since the stage was created */
    char name[64];                    /* "temporal antialiasing (N viewports)" */
} trhip_taa_timings;
/* Refuses width, height or layers of 0, alpha outside (0, 1] and projection 2. */
int trhip_taa_create(trhip_device* dev, const trhip_taa_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_taa** out);
void trhip_taa_destroy(trhip_taa* stage);
/* One frame: one kernel between two events on `stream`, no synchronisation.  Frames of one stage form one history: run them in frame
 * order on one stream (or on streams ordered with trhip_stream_wait). */
int trhip_taa_run(trhip_taa* stage, const trhip_taa_images* images, void* stream);
int trhip_taa_reset_history(trhip_taa* stage);   /* camera cut / new scene: the next frame passes through, like a new stage's first */
int trhip_taa_get_timings(trhip_taa* stage, trhip_taa_timings* out);   /* waits for the last frame */
#define TRHIP_TAA_HISTORY 0           /* RGBA32F [layers][h][w]: what the next frame will read */
#define TRHIP_TAA_DECISIONS 1         /* uint8 [layers][h][w]: bits 0-3 the dilation offset as (x + 1) * 3 + (y + 1), bit 4 reprojected outside
                                         (passed through), bit 5 no surface */
int trhip_taa_download(trhip_taa* stage, int which, void* host, size_t bytes);   /* synchronises the device */

/* ---- looking_glass_composition_stage (--display=looking-glass; src/looking_glass_composition_stage.{hh,cc},
 * shader/looking_glass_composition.comp): the last stage of a light-field chain.  It interleaves the N views, sub-pixel by sub-pixel, into
 * the one image a lenticular panel shows.  csrc/looking_glass.hip, one kernel per frame; the order of operations is pinned in
 * csrc/looking_glass.h.  Per output pixel p:
 *   1. calibration = (pitch, tilt * pitch, pitch / (3 * out_w), -center), every component negated under invert (computed by the host, in float)
 *   2. uv = (p + 0.5) / out_size; uvf = (uv.x, 1 - uv.y)
 *   3. per channel c = 0, 1, 2: d = ((uvf.x * cal.x + uvf.y * cal.y) + c * cal.z) + cal.w; view = clamp(int(floor(fract(d) * N)), 0, N - 1)
 *   4. out[c] = channel c of that view, sampled bilinearly with clamp to edge at the unflipped uv (the shader flips y twice)
 *   5. alpha = 1; dst_rgba8 = uint8(clamp(c, 0, 1) * 255 + 0.5) per channel and 255 for alpha
 * Deviations from the reference: (1) the views are fp32 where the reference's are B8G8R8A8: dst_rgba8 is the reference's
 * output format (in r, g, b, a order), the fp32 dst is extra; (2) the bilinear weights are fp32 where Vulkan's sampler uses 8-bit fixed
 * point; (3) a NaN or a negative input passes through to dst and is clamped in dst_rgba8 (a NaN gives 0). */
typedef struct trhip_lkg trhip_lkg;
typedef struct trhip_lkg_options {
    uint32_t viewport_count;          /* 1..255 */
    float pitch, tilt, center;        /* the reference's corrected_pitch, tilt, center (src/looking_glass.cc:240-241) */
    int32_t invert;
    int32_t record_view_indices;      /* keep a uint8[4] per output pixel for trhip_lkg_download */
} trhip_lkg_options;
typedef struct trhip_lkg_timings {    /* the reference's timer, device ms of the last frame */
    float total_ms;
    uint32_t frames;                  /* frames run since the stage was created */
    char name[64];                    /* "looking glass composition" */
} trhip_lkg_timings;
/* Refuses a view or output size of 0 or with an extent above 16384, a viewport_count of 0 or above 255 and a pitch, tilt or center that is
 * not finite. */
int trhip_lkg_create(trhip_device* dev, const trhip_lkg_options* opt, uint32_t view_w, uint32_t view_h, uint32_t out_w, uint32_t out_h, trhip_lkg** out);
void trhip_lkg_destroy(trhip_lkg* stage);
/* One frame: src RGBA32F [views][view_h][view_w] in display space; dst RGBA32F [out_h][out_w] or NULL; dst_rgba8 uint8 [out_h][out_w][4] or
 * NULL (not both NULL).  One kernel between two events on `stream`, no synchronisation.  The stage has no history: it may run on a frame
 * slot's own stream. */
int trhip_lkg_run(trhip_lkg* stage, const void* src, void* dst, void* dst_rgba8, void* stream);
int trhip_lkg_get_timings(trhip_lkg* stage, trhip_lkg_timings* out);   /* waits for the last frame */
#define TRHIP_LKG_VIEW_INDICES 0      /* uint8 [out_h][out_w][4]: the view of r, g, b; 0 (record_view_indices only) */
int trhip_lkg_download(trhip_lkg* stage, int which, void* host, size_t bytes);   /* synchronises the device */

/* ---- sh_path_tracer_stage + sh_compact_stage (src/sh_path_tracer_stage.{hh,cc}, shader/sh_path_tracer.rgen, src/sh_grid.{hh,cc},
 * shader/sh_compact.comp): bakes a grid of light probes as spherical-harmonics coefficients - the server half of the reference's DDISH-GI.
 * csrc/sh_probes.hip; the order of operations is pinned in csrc/sh_probes.h.  For probe (x, y, z) of a grid of resolution R and sample s of
 * N = samples_per_probe:
 *   1. ls = init_local_sampler(uvec4(x, y, z, s)) with sample_counter = frame_counter * N and the rng_seed rule of src/rt_stage.cc:81-82
 *   2. probe-space offset: 0 (point film), generate_spatial_sample(ls) * 2 - 1 (box), sample_blackman_harris_ball(generate_spatial_sample(ls))
 *   3. local_pos = ((vec3(p) + offset * film_radius + 0.5) / vec3(R)) * 2 - 1; global_pos = (transform * vec4(local_pos, 1)).xyz
 *   4. local_dir = even_sample_sphere(s, N, (rotation_x, rotation_y)); global_dir = normalize(normal_transform * local_dir), with
 *      rotation_x = pcg(frame_counter * N) / float(0xFFFFFFFF), rotation_y the same of frame_counter * N + 1 and
 *      normal_transform = mat4(get_matrix_orientation(transform))
 *   5. evaluate_ray with HIDE_LIGHTS and INDIRECT_CLAMP_FIRST_BOUNCE (shader/path_tracer.glsl:422-427, 465-467): the bounce loop of the path
 *      tracer stage on its general kernels; value = modulate_color(first_hit_material, diffuse.rgb, reflection.rgb), no emission term
 *   6. dist = clamp(distance(first_hit_vertex.pos, global_pos) * length(local_dir * cell_scale), 0, sqrt(3)), cell_scale = 0.5 * vec3(R) / scaling
 *   7. coefficient l of the probe = sum over s of vec4(value, dist) * (4 pi / N) * sh_basis(local_dir)[l]
 *   8. out = mix(previous, new, mix_ratio), mix_ratio = max(1 / history_length, temporal_ratio); history_length counts renders since
 *      creation or trhip_sh_reset_history; with mix_ratio >= 1 the previous value is not read
 *   9. one RGBA32F volume [rz][ry * C][rx], C = (order + 1)^2, coefficient l of probe (x, y, z) at (x, y + l * ry, z), and its RGBA16F copy
 *      in the same layout (what sh_grid::create_texture holds after sh_compact)
 * Deviations from the reference: (1) the stage keeps a frame counter of its own for the sampler and the rotation
 * (trhip_sh_set_frame_counter; it advances by one per render) where the reference reads the context's; (2) only sampler = 0
 * (uniform-random, the command line's default) is accepted: the Sobol samplers take their index from a pixel launch; (3) the N samples of
 * a probe are summed in one fixed tree (csrc/sh_probes.h) where the reference splits them into invocations and z-slices for Vulkan's 3D
 * image limit: the same sum in another order.
 * Of `path` the stage reads max_bounces, min_ray_dist, rng_seed, sampler, film, film_radius, mis_mode, russian_roulette_delta,
 * indirect_clamping, regularization_gamma, nee_point, nee_directional, nee_envmap, nee_triangles, bounce_mode and tri_light_mode; the sample
 * counts, projection, depth of field, hide_lights, white albedo, transparent background and pre-transformed vertices do not apply. */
typedef struct trhip_sh trhip_sh;
typedef struct trhip_sh_options {     /* sh_path_tracer_stage::options (src/sh_path_tracer_stage.hh) + sh_grid (src/sh_grid.hh) */
    int32_t order;                    /* 0..4; C = (order + 1)^2 coefficients per probe */
    uint32_t resolution[3];           /* sh_grid::get_resolution, each 1..1024 */
    uint32_t samples_per_probe;       /* N >= 1; a probe's samples fit one batch (at most 1920 * 1080) */
    float temporal_ratio;             /* in [0, 1] */
} trhip_sh_options;
typedef struct trhip_sh_grid_data {   /* grid_data_buffer of src/sh_path_tracer_stage.cc:10-19 as the next render would pack it (test hook) */
    float transform[16], normal_transform[16];   /* column-major */
    uint32_t grid_size[3];
    float mix_ratio;
    float cell_scale[3];
    float rotation_x, rotation_y;
} trhip_sh_grid_data;
typedef struct trhip_sh_timings {     /* the reference's timer, device ms of the last render (every batch, the projection included) */
    float total_ms;
    uint32_t frames;                  /* renders since the stage was created */
    char name[64];                    /* "SH path tracing" */
    /* Per-kernel device time, only collected while detailed timing is on (trhip_sh_set_profiling: one lane, an event pair around every
     * launch): the bounce loop's kernels cumulative since trhip_sh_reset_counters (as trhip_timings), k_sh_project of the last render. */
    float raygen_ms, trace_closest_ms, trace_shadow_ms, shade_ms, project_ms;
} trhip_sh_timings;
/* sh_path_tracer_stage ctor.  Refuses a zero resolution, an order outside 0..4, samples_per_probe < 1, a temporal_ratio outside [0, 1],
 * sampler != 0 and a null device (there is no CPU fallback). */
int trhip_sh_create(trhip_device* dev, const trhip_pt_options* path, const trhip_sh_options* opt, trhip_sh** out);
void trhip_sh_destroy(trhip_sh* stage);
/* The grid's transformable: get_global_transform() (column-major; maps [-1, 1]^3 onto the grid's box) and get_scaling()
 * (src/sh_path_tracer_stage.cc:119-132).  Identity and (1, 1, 1) until set.  Refuses a transform that is not finite. */
int trhip_sh_set_transform(trhip_sh* stage, const float transform[16], const float scaling[3]);
int trhip_sh_set_frame_counter(trhip_sh* stage, uint32_t frame_counter);   /* context::get_frame_counter of the next render */
int trhip_sh_reset_history(trhip_sh* stage);                               /* history_length = 0: the next render replaces the grid */
int trhip_sh_set_lanes(trhip_sh* stage, int lanes);                        /* trhip_pt_set_lanes of the stage's bounce loop */
/* A grid is rendered in batches of whole probes; 0 (the default) = as many as fit 1920 * 1080 paths, the frame the lane schedule was tuned
 * on.  The grids do not depend on it (tests). */
int trhip_sh_set_batch_probes(trhip_sh* stage, uint32_t probes);
int trhip_sh_set_shading_arithmetic(trhip_sh* stage, int ieee);            /* trhip_pt_set_shading_arithmetic of the bounce loop */
/* TEST AND TOOL HOOKS - the four entries below replace nothing of the reference and are not what an adapter binds; they are exported
 * like trhip_taa_download and trhip_bmfr_fit_blocks, for the tests and tools/sh_probe_bake_probe.py.
 * grid_data_buffer as sh_path_tracer_stage::update packs it (src/sh_path_tracer_stage.cc:115-137): of the stage's next render, or - host
 * only, no device - of render number history_length (>= 1) at frame_counter of a grid with these parameters.  Both hosts call the second
 * one for their sh_grid_parameters, so a comparison of the hosts checks their argument marshalling; the values are checked against
 * tests/sh_probes_model.py, which is written from the rule and shares no code with the library. */
int trhip_sh_get_grid_data(trhip_sh* stage, trhip_sh_grid_data* out);
int trhip_sh_pack_grid_data(const float transform[16], const float scaling[3], const uint32_t resolution[3], uint32_t samples_per_probe,
                            uint32_t frame_counter, uint32_t history_length, float temporal_ratio, trhip_sh_grid_data* out);
/* sh_path_tracer_stage::update + record_command_buffer and sh_compact_stage: one render of the whole grid, asynchronous on `stream`.  Renders
 * of one stage form one history: run them in order on one stream (or on streams ordered with trhip_stream_wait).  Refuses a device
 * without a scene or without an acceleration structure. */
int trhip_sh_render(trhip_sh* stage, void* stream);
/* The device images, for a consumer (trhip_dshgi_set_grids takes the RGBA16F one: sample_sh_grid reads it): valid for the life of the stage. */
int trhip_sh_get_grids(trhip_sh* stage, void** grid_dev, void** grid_half_dev);
#define TRHIP_SH_GRID 0               /* RGBA32F [rz][ry * C][rx] */
#define TRHIP_SH_GRID_HALF 1          /* RGBA16F, the same layout */
int trhip_sh_download(trhip_sh* stage, int which, void* host, size_t bytes);   /* synchronises the device */
int trhip_sh_get_counters(trhip_sh* stage, trhip_counters* out);   /* rays traced, cumulative (trhip_pt_get_counters of the bounce loop); synchronises the stream */
int trhip_sh_get_primary_start(trhip_sh* stage, trhip_primary_start_info* out);   /* trhip_pt_get_primary_start of the bounce loop: a probe stage has a ray generation of its own, the mode is never in effect */
int trhip_sh_get_timings(trhip_sh* stage, trhip_sh_timings* out);  /* waits for the last render */
int trhip_sh_set_profiling(trhip_sh* stage, int count_work, int detailed_timing);   /* tool hook: trhip_pt_set_profiling of the bounce loop */
int trhip_sh_reset_counters(trhip_sh* stage);                      /* tool hook: trhip_pt_reset_counters of the bounce loop; synchronises the stream */

/* ---- dshgi_renderer's indirect light (src/dshgi_renderer.{hh,cc}, shader/forward.frag:100-159, shader/spherical_harmonics.glsl:80-312,
 * src/scene_stage.cc:1119-1131, src/scene.cc:163-211, src/sh_grid.cc:116-144, shader/ggx.glsl:69-72): the consumer half of the reference's
 * DDISH-GI - direct light plus indirect light looked up in the baked SH grids, no bounce rays per pixel.  csrc/dshgi.hip; the order of
 * operations is pinned in csrc/dshgi.h.  Per pixel of each viewport one ray goes through the pixel centre, as trhip_gbuffer_render traces
 * it.  On a hit:
 *   1. shade_surface gives v (pos, smooth_normal, mapped_normal) and mat; view = normalize(v.pos - camera origin)
 *   2. grid g = instance_grids[hit.instance_id] (trhip_dshgi_pick_grid below); per grid pos_from_world = affineInverse(transform),
 *      normal_from_world = mat4(inverse(get_matrix_orientation(transform))), grid_clamp = 0.5 / R
 *   3. sample_pos = pos_from_world * v.pos; sample_normal (of smooth_normal), sh_normal (of mapped_normal) and
 *      sh_ref = reflect(view, mapped_normal) go through normal_from_world and are normalized
 *   4. sample_sh_grid, chosen per stage by use_probe_visibility (the reference's --use-probe-visibility; off = trilinear):
 *      trilinear   p = clamp(sample_pos * 0.5 + 0.5, grid_clamp, 1 - grid_clamp); c = p * R - 0.5; lo = floor(c), hi = min(lo + 1, R - 1), the
 *                  weights are the fractions in fp32; eight RGBA16F texels per coefficient at (x, y + l * ry, z), one fixed chain of sums
 *      visibility  spherical_harmonics.glsl:245-308: interp_pos, the eight weight[k], normal_factor,
 *                  visibility = calc_sh_value(lc, -normalize(sample_dir * inv_grid_size)).w,
 *                  visibility_factor = clamp(visibility - sample_dist + 0.4, 0, 1), renormalised by sum_weight (0 when the sum is 0).
 *                  clamp(x, lo, hi) is fmin(fmax(x, lo), hi): a shading point exactly on a probe has sample_dir = 0 / 0 there, both
 *                  factors become 0 and that corner has weight 0 (GLSL leaves clamp(NaN) undefined)
 *   5. incoming_diffuse = max(sum coef[l].rgb * cosine_lobe(sh_normal)[l], 0), band factors 1, 2/3, 1/4, 0, -1/24;
 *      incoming_reflection = max(sum coef[l].rgb * ggx_lobe(sh_ref, sqrt(mat.roughness))[l], 0), the fitted zh curves of lines 126-151
 *   6. brdf_indirect: cos_v = max(dot(mapped_normal, -view), 0); fresnel = fresnel_schlick_attenuated(cos_v, f0, roughness);
 *      kd = (1 - fresnel)(1 - metallic)(1 - transmittance); bi = the bilinear, clamp-to-edge fetch of the BRDF-integration table at
 *      (cos_v, sqrt(roughness)); diffuse = kd * incoming_diffuse; reflection = incoming_reflection * mix(fresnel * bi.x + bi.y, 1, metallic)
 *   7. indirect = modulate_color(mat, diffuse, reflection), no emission term; a miss or an instance without a grid (index -1) gives 0
 *   8. colour.rgb = direct.rgb + indirect, one fp32 add per channel; alpha is the direct stage's (modulate_color is linear, so this
 *      equals the reference's single call)
 * Deviations from the reference: (1) the reference rasterises the first hit and lights it with shadow maps; here the
 * first hit is a ray and direct light is the direct stage (trhip_direct_create); (2) Vulkan's sampler filters the trilinear branch with
 * 8-bit fixed-point weights, these are fp32; (3) the reference gives an instance without a grid an ambient colour, here it gets 0;
 * (4) the BRDF-integration table is generated (below) unless one is uploaded. */
typedef struct trhip_dshgi trhip_dshgi;
typedef struct trhip_dshgi_options {
    int32_t order;                    /* 0..4, the order the grids were baked at */
    int32_t use_probe_visibility;     /* 0 = SH_INTERPOLATION_TRILINEAR */
    int32_t record_surface;           /* keep TRHIP_DSHGI_SURFACE (test hook) */
} trhip_dshgi_options;
typedef struct trhip_dshgi_grid {     /* sh_grid + its transformable + its texture */
    const void* grid_half_dev;        /* RGBA16F [rz][ry * C][rx], trhip_sh_get_grids' second image or any upload of that layout */
    uint32_t resolution[3];           /* each 1..1024 */
    float transform[16];              /* get_global_transform(), column-major */
    float scaling[3];                 /* get_global_scaling() */
} trhip_dshgi_grid;
typedef struct trhip_dshgi_surface {  /* TRHIP_DSHGI_SURFACE: what the kernel shaded a pixel with; instance_id -1 = a miss (the rest 0) */
    float pos[3], smooth_normal[3], mapped_normal[3], view[3], albedo[4];
    float metallic, roughness, f0, transmittance;
    int32_t grid, instance_id;
} trhip_dshgi_surface;
typedef struct trhip_dshgi_timings {  /* device ms of the last render */
    float total_ms;
    uint32_t frames;
    char name[64];                    /* "dshgi indirect" */
} trhip_dshgi_timings;
/* Refuses a null device (there is no CPU fallback), an order outside 0..4 and a zero width, height or layer count. */
int trhip_dshgi_create(trhip_device* dev, const trhip_dshgi_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_dshgi** out);
void trhip_dshgi_destroy(trhip_dshgi* stage);
/* The scene's grids; the library derives pos_from_world, normal_from_world and grid_clamp.  The images stay the caller's.  Synchronous. */
int trhip_dshgi_set_grids(trhip_dshgi* stage, const trhip_dshgi_grid* grids, uint32_t count);
/* sh_grid_index of every instance of the scene, -1 = none.  Refuses an index outside the grids set.  Synchronous. */
int trhip_dshgi_set_instance_grids(trhip_dshgi* stage, const int32_t* instance_grids, uint32_t count);
/* The BRDF-integration table, RG32F [h][w] on the device: texel (i, j) holds scale and bias at cos_v = (i + 0.5) / w and
 * sqrt(roughness) = (j + 0.5) / h.  The stage keeps a copy.  Synchronous. */
int trhip_dshgi_set_brdf_integration(trhip_dshgi* stage, const void* table_dev, uint32_t w, uint32_t h);
/* One frame of `count` viewports (at most the stage's layers), one launch per 64, asynchronous on `stream`: out_color_dev RGBA32F
 * [count][h][w] = direct_color_dev + indirect.  `out` may alias `direct`; a null `direct` writes the indirect term alone (alpha 0).
 * Refuses: no grids set, an instance count different from the scene's, no table, a device without a scene or acceleration structure. */
int trhip_dshgi_render(trhip_dshgi* stage, int projection, const uint32_t* viewports, uint32_t count, float min_ray_dist,
                       const void* direct_color_dev, void* out_color_dev, void* stream);
int trhip_dshgi_get_timings(trhip_dshgi* stage, trhip_dshgi_timings* out);   /* waits for the last render */
#define TRHIP_DSHGI_INDIRECT 0        /* RGBA32F [layers][h][w]: the indirect term of the last render, alpha 0 */
#define TRHIP_DSHGI_SURFACE 1         /* trhip_dshgi_surface [layers][h][w] (record_surface only) */
int trhip_dshgi_download(trhip_dshgi* stage, int which, void* host, size_t bytes);   /* test hook; synchronises the device */
/* get_sh_grid and get_largest_sh_grid (src/scene.cc:163-211) for `position` (the hosts pass model[3] of an instance): inside several grids
 * the densest wins (`>` on density), otherwise the nearest within its guard distance (`<=` on sh_grid::point_distance with the grid's
 * radius, later grids win ties), otherwise the grid of largest volume; -1 when there is none.  transforms 16, scalings 3, resolutions 3
 * values and one radius per grid.  Host only, no device: both hosts call it, the model of tests/dshgi_model.py checks it. */
int trhip_dshgi_pick_grid(const float* transforms, const float* scalings, const uint32_t* resolutions, const float* radii, uint32_t count,
                          const float position[3], int32_t* index);
/* The table the reference loads from data/brdf_integration.exr, evaluated on the device: size x size cells of `samples` Hammersley samples
 * of the split sum with this library's GGX terms (csrc/dshgi.h), cell (i, j) at cos_v = (i + 0.5) / size, alpha = ((j + 0.5) / size)^2.
 * out_dev_rg32f: size * size * 8 bytes.  Asynchronous on `stream`.  The hosts generate 256 x 256 with 1024 samples. */
int trhip_brdf_integration_generate(trhip_device* dev, uint32_t size, uint32_t samples, void* out_dev_rg32f, void* stream);

/* ---- ReSTIR DI: reservoir resampling of direct light, written after shader/restir_di.glsl, shader/restir_di_canonical_and_temporal.rgen
 * and shader/restir_di_spatial.rgen, which the reference carries but no longer wires up (its --renderer=restir is ReSTIR PT and is not
 * built here: this is `restir-di` everywhere).  csrc/restir_di.hip; the order of operations and of random draws is pinned in
 * csrc/restir_di.h.  Per frame and chunk of 64 viewports two launches:
 *   canonical  the first hit of the pixel centre's ray, its surface record, `candidates` light samples drawn as sample_canonical draws
 *              them and resampled (RIS) with target = luminance(light_contribution * shadow ray) (decision 17: the ray is a mode); with temporal_reuse the history
 *              reservoir of the stochastically reprojected pixel is merged by confidence unless temporal_edge_detection rejects it
 *   spatial    up to spatial_samples neighbours within search_radius, merged with pairwise MIS and the reconnection Jacobian, one shadow
 *              ray per re-evaluation (decision 17: the ray is a mode); the chosen sample is shaded with one more, in every mode: colour = contribution * uc_weight + emission, alpha 1
 * Decisions where the shaders are stale, undefined or depart from this library:
 *   1. BSDF: the ggx_bsdf_pdf lobes through modulate_bsdf, as the direct stage's light sample gets them, shading_view.z clamped to 1e-5
 *      (restir_di.glsl:234-244 calls a ggx_brdf signature that no longer exists).
 *   2. The first hit is a traced ray, not a raster G-buffer; view = normalize(pos - ray origin).
 *   3. light_data and the previous frame's normal and position are fp32 (the previous surface record), not rg16 / rg16_snorm images.
 *   4. A directional light with dir_cutoff >= 1 has light_pdf = dir_prob / light_count (the shader's -1 marker, restir_di.glsl:319, gives a
 *      negative resampling weight).
 *   5. The two kernels draw from disjoint random streams (sampler coordinate w = 2 * frame and 2 * frame + 1, plus rng_seed as
 *      init_local_sampler adds it); the shaders seed both passes alike.  The order of draws within a kernel is the shaders'.
 *   6. The default visibility path is a shadow ray inside every target function; the shaders' SHARED_VISIBILITY and SAMPLE_VISIBILITY
 *      are the modes `shared` and `sampled` of trhip_restir_di_set_visibility (decisions 17 to 22).
 *   7. An empty neighbour slot is skipped (restir_di_spatial.rgen:145-149 reads out of bounds and adds 0).
 *   8. The first frame after create or reset has no history; history light indices refer to the current frame's light arrays, an index
 *      past the end counts as the null sample.
 *   9. One pass per frame; no accumulation over frames.
 *  10. Sphere lights are lit as points (color / max(dist^2, 1e-7)); shadow rays do not see lights.
 *  11. A draw that takes no light class (no lights, or u.w past the sum of the probabilities by rounding) is the null sample with pdf 1
 *      (restir_di.glsl:265-353 has no such branch and leaves its outputs undefined).
 *  12. A NaN resampling weight is 0 in every merge (the shader says so for candidates only, restir_di_canonical_and_temporal.rgen:98-100).
 *  13. A neighbour candidate without a surface is passed over like one off screen (restir_di_spatial.rgen:111-116 compares NaN positions);
 *      round() of an offset is floor(x + 0.5) (GLSL leaves the tie to the implementation).
 *  14. A contribution without a positive component casts no shadow ray and has visibility 0 (the product is 0 either way).
 *  15. Triangle lights are sampled by solid angle; the light class weights are all 1.
 *  16. sin, cos, pow and atan2 of the resampling code (light sampling, light_contribution, the neighbour offsets) are the double function of
 *      the float argument rounded once, not the device library's sinf / cosf / powf / atan2f: GLSL leaves their accuracy open, and this is
 *      the one rounding a host model can repeat bit for bit - in all but the rarest case, a double result so near a float rounding boundary
 *      that two libraries' doubles fall on either side of it.  The first hit is shaded as every other stage shades it.
 *  17. Visibility modes.  per-target (0, the default) casts candidates + 2 * spatial_samples + 1 shadow rays a pixel.  shared (1): no
 *      target function traces - candidates, the neighbour's sample here, the canonical sample at the neighbour - and the only ray is the
 *      chosen sample's shading.  sampled (2): as shared, plus one ray for the sample the candidates chose.  An untraced target's
 *      visibility factor, recorded as such, is 1 where decision 14 would cast a ray and 0 otherwise, so
 *      target = luminance(contribution * visibility) describes every mode.  No mode adds, removes or reorders a random draw.
 *  18. sampled: behind the candidates' uc_weight and ahead of the temporal merge the reservoir's sample is evaluated once more at the
 *      pixel and traced by decision 14 (no ray and visibility 0 for the null sample), then uc_weight *= visibility
 *      (restir_di_canonical_and_temporal.rgen:115-122).  The temporal merge is the same in every mode.
 *  19. shared and sampled: a bad neighbour takes no slot (restir_di_spatial.rgen:123-129 is compiled out); the first spatial_samples good
 *      ones are held in draw order; the 2 * spatial_samples offset draws stay.
 *  20. The shading ray stays in every mode.  sampled: uc_weight *= visibility ahead of the history reservoir, and the colour is
 *      contribution * visibility * uc_weight + emission with that multiplied weight (restir_di_spatial.rgen:266-269,281).  Limit: under a
 *      partly transparent occluder (0 < visibility < 1) `sampled` counts the factor once per pass that traced it; it is exact for opaque
 *      occluders only.
 *  21. shared is unbiased like per-target (a target without visibility is a valid target; the traced ray is in the integrand).  sampled
 *      is biased wherever visibility differs between the pixels that share a sample: the paper's biased variant.
 *  22. A reservoir does not mix the samples of two target functions: the mode changes only while the stage holds no history.  ReSTIR GI's
 *      own kernels keep their visibility path whatever the mode of the ReSTIR DI stage beside them.
 *  23. Light selection (trhip_restir_di_set_light_selection).  uniform (0, the default) draws a point or triangle
 *      light as sample_canonical does, index = clamp(int(u * n), 0, n - 1) with pdf 1 / n.  power (1) draws it in proportion to a weight:
 *      a point or spot light's is luminance(color) - the spot cone and the radius are ignored -, a triangle light's
 *      luminance(r9g9b9e5_to_rgb(emission_factor)) * (0.5 * |cross(pos[1] - pos[0], pos[2] - pos[0])|) - the emission texture is
 *      ignored -, a negative, NaN or infinite weight is 0.  Directional lights, the environment and the four class probabilities
 *      (decision 15) keep their rule.
 *  24. Inside a class of n lights p_i = (1 - f) * w_i / sum(w) + f / n with the caller's uniform_fraction f in (0, 1]; 1 / n when
 *      sum(w) = 0.  The uniform share is what keeps the estimator unbiased where the weight is blind - textures, cones, a table that is
 *      stale because lights moved since it was built -: a light that contributes has a positive pdf.
 *  25. The table: one 16-byte alias entry per light, the point lights' table then the triangle lights', each over its own n slots,
 *      built on the host (include/tauray_alias.hh) in the work-list order and threshold encoding of the environment map's table, in
 *      double steps; pdf and alias_pdf are float(p_i) of the slot and of its alias.
 *  26. The draw: p = uint64(word) * n, slot = p >> 32, low = uint32(p), word = the draw's x for a point and z for a triangle light (the
 *      words uniform selection reads); e = table[slot]; low > e.probability takes e.alias_id with e.alias_pdf, else the slot with
 *      e.pdf; light_pdf = pdf * prob_point, or (tri_pdf * pdf) * prob_tri with the point on the triangle from x and y as ever.  No
 *      draw is added or removed.  Limit: a light's frequency differs from its recorded pdf by at most n / 2^32 relative, the
 *      granularity of `low` and of the slot.
 *  27. The pdf of a candidate is no part of a reservoir, so the table may be rebuilt while the stage holds history
 *      (trhip_restir_di_refresh_light_selection); the mode and the fraction change only without history: uc_weight does not mix two
 *      candidate distributions silently (as decision 22).
 *  28. ReSTIR GI's kernels draw the light sample at a secondary hit uniformly whatever the selection of the ReSTIR DI stage beside them.
 *  29. BSDF candidates (trhip_restir_di_set_bsdf_candidates; Bitterli et al. 2020 section 3.1, Talbot's RIS).  Behind
 *      the L = options.candidates light candidates, drawn exactly as before, the canonical pass draws B = bsdf_candidates (0..8, L + B <= 32,
 *      default 0) candidates from the surface's BSDF; M = L + B.  A BSDF candidate takes two draws from the pass's stream, null or not:
 *      one whose four unit words are ggx_bsdf_sample's `ur`, one whose unit x is update_reservoir's selection draw.  The temporal
 *      merge's draw follows them.
 *  30. Its direction: tbn, shading_view and mat as the contribution builds them (z of the view clamped to 1e-5);
 *      ggx_bsdf_sample<RoundedMath>(ur, shading_view, mat, out_dir), dir = normalize(tbn * out_dir).  p_b(x) is one function of (surface,
 *      world direction) for candidates of both techniques, the value of ggx_bsdf_pdf<RoundedMath>(dir * tbn, shading_view, mat); the pdf
 *      the sampler returns is not used (the two disagree on the transmission lobe).
 *  31. A BSDF candidate is the null sample with weight 0 and traces nothing when out_dir has a NaN or is 0, when p_b is not > 0 - this
 *      includes zero roughness, whose specular lobe is a delta: mirrors gain nothing - or when dot(dir, flat_normal) < 1e-6, where the
 *      contribution is 0 under decision 5's rule: transmitted directions find no direct light.
 *  32. Otherwise one closest-hit ray (pos, dir, min_ray_dist, inf).  A hit on an instance with light_base_id >= 0 is the triangle sample
 *      (type 1, index = light_base_id + primitive, light_data = (1 - u - v, u): light_data.x weighs pos[0] and .y pos[1], a hit's u and v
 *      weigh vertices 1 and 2); a miss with an environment is the environment sample (type 3, index 0, light_data = the lat-long uv of
 *      dir: x = atan2(dir.z, dir.x) / (2 pi) + 0.5, y = atan2(-dir.y, sqrt(dir.x^2 + dir.z^2)) / pi + 0.5, RoundedMath's atan2); a
 *      non-emissive hit, a miss without an environment and an index past the triangle light count are the null sample.
 *  33. The found sample is fetched and evaluated like any other, so its contribution is what a light candidate of that identity gets.
 *      Its visibility factor is 1 where the contribution has a positive component and 0 otherwise in every visibility mode: the
 *      closest-hit ray is the visibility, no shadow ray is added.  Limit: an environment sample's direction is rebuilt from its uv and
 *      differs from the traced one by rounding.  Rays a pixel: B closest-hit rays more than decision 17 counts, in every mode.
 *  34. p_l(x), the pdf with which the light technique produces the sample's identity: a light candidate's light_pdf; for a triangle
 *      found by a BSDF ray (tri_pdf * sel) * prob_tri with tri_pdf the solid-angle pdf of that triangle from pos (sample_canonical's
 *      formula and 1e9 rule, the ray's length that of the contribution's direction to the triangle's plane), sel = 1 / n_tri or, under
 *      power selection, table[n_point + index].pdf; for an environment sample table[pixel].pdf * prob_env with pixel =
 *      clamp(floor(uv * size)), sample_canonical's layout (not latlong_direction_to_pixel_id's + 0.5).  A class of probability 0: 0.
 *      p_b of a light candidate: 0 for point and directional samples, which the BSDF technique cannot produce; decision 30's function
 *      at the contribution's direction for triangle and environment samples.
 *  35. The balance heuristic: denom = float(L) * p_l + float(B) * p_b; weight = ((float(M) / (float(M) + prev_confidence)) * target) /
 *      denom; a NaN weight or denom <= 0 gives 0.  confidence += 1 per candidate of either technique.  Everything behind the loops -
 *      uc_weight, the sampled mode's ray, the temporal merge - is unchanged.  With B = 0 the stage launches the kernels it launched.
 *  36. The pdfs enter only the candidate weight.  bsdf_candidates changes only while the stage holds no history (as decisions 22 and
 *      27).  ReSTIR GI's kernels are untouched.  Out of scope: sphere lights (the stage lights them as points), delta lobes.
 *  37. Sphere lights (trhip_restir_di_set_sphere_lights).  point, the default, is decision 10 and the kernels that
 *      were.  area: a point-light sample whose light has radius != 0 is a point on that sphere; a light of radius 0 is what it was in
 *      both modes.  The sample keeps type 0 and its index; light_data is the octahedral encoding of the outward unit normal n of the
 *      point (encode: p = n.xy / (|n.x| + |n.y| + |n.z|), for n.z < 0 p = (1 - |p.yx|) * sign(p.xy) with sign(0) = 1; decode:
 *      n = (p.x, p.y, 1 - |p.x| - |p.y|), t = max(-n.z, 0), n.x += n.x >= 0 ? -t : t, likewise n.y, normalise).  No transcendental
 *      function: the model repeats the bits.  A point fixed in the world is what a neighbour or the next frame can evaluate again; the
 *      cone's random numbers are not kept.
 *  38. The draw.  Behind either sampler of the light candidates (uniform or power; its u.x chose the index, u.y and u.z are free) a
 *      type-0 sample with radius != 0 follows sample_point_light: d = pos - pl.pos, dist2 = dot(d, d), k = 1 - r^2 / dist2,
 *      cutoff = k > 0 ? sqrt(k) : -1, dir = sample_cone((u.y, u.z), -normalize(d), cutoff), b = dot(d, dir),
 *      len = -b - sqrt(max(b^2 - dist2 + r^2, 0)), x = pos + dir * len, n = normalize(x - pl.pos), data = encode(n),
 *      solid_pdf = 1 / (2 pi (1 - cutoff)), 1e9 when n has a NaN or len <= min_ray_dist; light_pdf = (the index's pdf) * solid_pdf.
 *      No draw is added or removed; both streams stay where they are.
 *  39. The contribution of such a sample: n = decode(data), x = pl.pos + r * n, p = x - pos, dir = normalize(p), dist2 = dot(p, p),
 *      normal = n, colour = pl.color * spot(normalize(pl.pos - pos)) / (r^2 pi) - the direct stage's radiance and its argument of the
 *      spot cone -, 0 when dot(n, dir) >= 0: the point faces away, or the receiver is inside the sphere.  The candidate's own
 *      contribution is evaluated from data like everyone else's (one code path; the limit environment samples have).  The flat-normal
 *      test, the lobes, modulate_bsdf and the NaN test are unchanged.
 *      Limit: a receiver inside a sphere gets 0 from it, while the direct stage and the path tracer light it (their shadow ray there
 *      has a negative length and finds nothing): on such pixels area mode does not converge to the direct stage's image.
 *  40. Jacobian, visibility and the merges are unchanged code: the normal is no longer 0, so the reconnection Jacobian is the
 *      solid-angle ratio a triangle sample gets; the shadow ray ends min_ray_dist short of x; shadow rays go on not seeing lights.
 *  41. Power selection: the weights keep ignoring the radius.
 *  42. BSDF candidates: a BSDF ray does not return a sphere light and type-0 samples keep p_b = 0.  Unbiased - the light technique
 *      alone covers the whole visible cap -, a limit on glossy surfaces under large lamps.
 *  43. The mode is a compile-time parameter of the sample kind (RestirDiKindT<SPHERE>, restir_di.h) and the area mode's kernels are a
 *      translation unit of their own (restir_di_sphere.hip): the point instances are the code they were.
 *  44. A reservoir does not mix samples of two meanings of light_data: the mode changes only while the stage holds no history.  Limits:
 *      ReSTIR GI's own light sample at a secondary hit stays a point; the camera ray does not see sphere lights. */
typedef struct trhip_restir_di trhip_restir_di;
typedef struct trhip_restir_di_options {
    uint32_t candidates;              /* 1..32 light samples per pixel (RIS_SAMPLE_COUNT) */
    uint32_t spatial_samples;         /* 0..4 (SPATIAL_SAMPLE_COUNT) */
    float search_radius;              /* pixels, > 0, at most 1024 */
    float max_confidence;             /* >= 1, the clamp of the temporal merge */
    int32_t temporal_reuse;           /* 0 / 1 */
    float min_ray_dist;               /* > 0 */
    uint32_t rng_seed;                /* raw; pcg() applied if non-zero, as the path tracer's */
    int32_t record;                   /* keep the decision records (test hook) */
} trhip_restir_di_options;
typedef struct trhip_restir_di_surface {      /* the shader's `domain`; instance_id -1 = a miss (the rest 0) */
    float pos[3]; int32_t instance_id;
    float mapped_normal[3], metallic;
    float flat_normal[3], roughness;
    float view[3], transmittance;
    float albedo[4];
    float emission[3], f0;
    float ior_in, ior_out, pad[2];
} trhip_restir_di_surface;
typedef struct trhip_restir_di_reservoir {    /* light = light_type << 30 | light_index; the null sample is type 0, index (1u << 30) - 1 */
    float uc_weight, target_function; uint32_t light; float confidence;
    float light_data[2]; uint32_t pad[2];
} trhip_restir_di_reservoir;
typedef struct trhip_restir_di_candidate {    /* per candidate; contribution is unshadowed; selected: update_reservoir took it */
    uint32_t light; float light_data[2], pdf;
    float contribution[3], visibility;
    float weight, draw; uint32_t selected, pad;
} trhip_restir_di_candidate;
typedef struct trhip_restir_di_temporal {     /* per pixel; target, weight, draw are 0 without reuse */
    int32_t px, py; uint32_t reuse; float prev_confidence;
    float target, weight, draw; uint32_t selected;
} trhip_restir_di_temporal;
typedef struct trhip_restir_di_spatial {      /* per neighbour slot; px -1 = empty; _n: the neighbour's sample here, _c: the canonical sample there */
    int32_t px, py; uint32_t good, selected;
    float target_n, visibility_n, jacobian_n, m;
    float wi, draw, target_c, visibility_c;
    float jacobian_c, mis_canonical, pad[2];
} trhip_restir_di_spatial;
typedef struct trhip_restir_di_final {        /* per pixel: the chosen sample's unshadowed contribution and its shadow ray, the canonical merge */
    float contribution[3], visibility;
    float canonical_m, wi, draw; uint32_t selected;
} trhip_restir_di_final;
typedef struct trhip_restir_di_sampled {      /* per pixel: decision 18's shadow ray (1, none traced, in the modes per-target and shared) and the candidates' uc_weight it
                                               * multiplied (shared: that weight, multiplied by nothing; per-target: 0) */
    float visibility, uc_weight_before; uint32_t pad[2];
} trhip_restir_di_sampled;
typedef struct trhip_restir_di_bsdf_candidate {   /* per candidate of a stage with BSDF candidates, next to trhip_restir_di_candidate (whose pdf is p_l) */
    uint32_t technique;               /* 0: a light candidate, 1: a BSDF candidate */
    float dir[3];                     /* light: the contribution's direction; BSDF: the traced one, 0 when the sampler gave none */
    float p_b;
    int32_t instance_id, primitive_id;   /* the BSDF ray's hit; instance -1 and t -1: a miss, nothing traced or a light candidate */
    float u, v, t;
    float denom; uint32_t traced;     /* 1: the closest-hit ray was cast */
} trhip_restir_di_bsdf_candidate;
typedef struct trhip_restir_di_timings {      /* device ms of the last render */
    float canonical_ms, spatial_ms, total_ms;
    uint32_t frames;
    char canonical_name[64], spatial_name[64];    /* "restir di canonical", "restir di spatial" */
} trhip_restir_di_timings;
/* Refuses a null device (there is no CPU fallback), zero or oversized dimensions and every option outside its range. */
int trhip_restir_di_create(trhip_device* dev, const trhip_restir_di_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_restir_di** out);
void trhip_restir_di_destroy(trhip_restir_di* stage);
int trhip_restir_di_reset(trhip_restir_di* stage);        /* forgets the history and restarts the frame counter */
/* The visibility mode (decisions 17 to 22); a stage is created per-target.  Refuses a null stage, a mode outside 0..2 and, while the stage
 * holds history (a frame rendered since create or reset), any mode but the history's. */
#define TRHIP_RESTIR_VISIBILITY_PER_TARGET 0
#define TRHIP_RESTIR_VISIBILITY_SHARED 1
#define TRHIP_RESTIR_VISIBILITY_SAMPLED 2
int trhip_restir_di_set_visibility(trhip_restir_di* stage, int mode);
/* The light selection (decisions 23 to 28); a stage is created uniform.  Refuses a null stage, a mode outside 0..1, a uniform_fraction
 * outside (0, 1] or NaN (checked, and otherwise ignored, for uniform), power on a device without a scene and, while the stage holds
 * history, any change of mode or fraction.  With power it builds the table from the scene's lights as they are: the weights kernel, a
 * download, the host builder, an upload; it waits for the device. */
#define TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM 0
#define TRHIP_RESTIR_LIGHT_SELECTION_POWER 1
int trhip_restir_di_set_light_selection(trhip_restir_di* stage, int mode, float uniform_fraction);
/* The BSDF candidates a pixel draws behind its light candidates (decisions 29 to 36); a stage is created with 0, and with 0 it launches
 * the kernels it always launched.  Refuses a null stage, n > 8, candidates + n > 32 and, while the stage holds history, any change; it
 * is accepted again after trhip_restir_di_reset.  With record it allocates the records of candidates + n candidates a pixel and waits
 * for the device. */
int trhip_restir_di_set_bsdf_candidates(trhip_restir_di* stage, uint32_t n);
/* How a point light with a radius is lit (decisions 37 to 44); a stage is created point, and in that mode it launches the kernels it
 * always launched.  Refuses a null stage, a mode outside 0..1 and, while the stage holds history, any mode but the history's; it is
 * accepted again after trhip_restir_di_reset. */
#define TRHIP_RESTIR_SPHERE_LIGHTS_POINT 0
#define TRHIP_RESTIR_SPHERE_LIGHTS_AREA 1
int trhip_restir_di_set_sphere_lights(trhip_restir_di* stage, int mode);
/* Rebuilds the table after the scene's lights or instances changed; allowed while the stage holds history (decision 27).  The build is
 * skipped when the lights' weights are byte-equal to those the table was built from: *rebuilt (may be null) is 1 or 0.  Waits for the
 * device.  A uniform stage: nothing, 0.  trhip_restir_di_render refuses, in power mode, a scene whose point or triangle light count
 * differs from the table's until this call; it never builds or synchronises on its own. */
int trhip_restir_di_refresh_light_selection(trhip_restir_di* stage, uint32_t* rebuilt);
/* One frame of `count` viewports (at most the stage's layers), two launches per 64, asynchronous on `stream`: out_color_dev RGBA32F
 * [count][h][w].  Refuses a device without a scene or acceleration structure and a viewport out of range.  History is kept per layer, the
 * position in the list: with temporal_reuse, a list that differs from the last frame's is refused until trhip_restir_di_reset. */
int trhip_restir_di_render(trhip_restir_di* stage, int projection, const uint32_t* viewports, uint32_t count, void* out_color_dev, void* stream);
int trhip_restir_di_get_timings(trhip_restir_di* stage, trhip_restir_di_timings* out);   /* waits for the last render */
#define TRHIP_RESTIR_DI_SURFACE 0     /* trhip_restir_di_surface [layers][h][w] of the last frame */
#define TRHIP_RESTIR_DI_CANONICAL 1   /* trhip_restir_di_reservoir [layers][h][w]: what the canonical kernel wrote */
#define TRHIP_RESTIR_DI_HISTORY 2     /* trhip_restir_di_reservoir [layers][h][w]: what the spatial kernel wrote */
#define TRHIP_RESTIR_DI_CANDIDATES 3  /* trhip_restir_di_candidate [layers][h][w][candidates + bsdf_candidates] (record only, as the three below) */
#define TRHIP_RESTIR_DI_TEMPORAL 4    /* trhip_restir_di_temporal [layers][h][w] */
#define TRHIP_RESTIR_DI_SPATIAL 5     /* trhip_restir_di_spatial [layers][h][w][spatial_samples] */
#define TRHIP_RESTIR_DI_FINAL 6       /* trhip_restir_di_final [layers][h][w] */
#define TRHIP_RESTIR_DI_SAMPLED 7     /* trhip_restir_di_sampled [layers][h][w] (record only) */
#define TRHIP_RESTIR_DI_LIGHT_WEIGHTS 8   /* float [n_point + n_tri]: the weights the table was built from (power selection; with and without record) */
#define TRHIP_RESTIR_DI_LIGHT_TABLE 9     /* 16-byte alias entries { uint32 alias_id, probability; float pdf, alias_pdf }, same order */
#define TRHIP_RESTIR_DI_BSDF_CANDIDATES 10 /* trhip_restir_di_bsdf_candidate [layers][h][w][candidates + bsdf_candidates] (record only; refused with 0 BSDF candidates) */
int trhip_restir_di_download(trhip_restir_di* stage, int which, void* host, size_t bytes);   /* test hook; synchronises the device */

/* ---- ReSTIR GI: reservoir resampling of indirect light (after Ouyang et al. 2021 and the ReSTIR DI stage above, whose
 * resampling rule it keeps; the reference has no such renderer, its --renderer=restir is ReSTIR PT and is not built here: this is
 * `restir-gi` everywhere).  csrc/restir_gi.hip; the order of operations and of random draws is pinned in csrc/restir_gi.h.  A sample is
 * a point x_s on a surface, its geometric normal n_s towards the pixel that found it and the radiance L_o it sent there.  Per frame and
 * chunk of 64 viewports three launches:
 *   initial    the first hit and its surface record (DI's), one cosine-hemisphere ray from it, the closest hit x_s, one light sample at
 *              x_s drawn as sample_canonical draws it, with its shadow ray: L_o = contribution * visibility / light_pdf
 *   temporal   no rays: the initial sample's weight (DI's rule with one candidate), and with temporal_reuse the merge of the history
 *              reservoir of the stochastically reprojected pixel unless temporal_edge_detection rejects it
 *   spatial    up to spatial_samples neighbours within search_radius, merged with pairwise MIS and the reconnection Jacobian, one shadow
 *              ray per re-evaluation; out.rgb = in.rgb + contribution * visibility * uc_weight of the chosen sample, out.a = in.a
 * The contribution of a sample at a surface is the ggx_bsdf_pdf lobes through modulate_bsdf for the direction to x_s, times L_o; 0 when
 * the direction is below the surface's flat normal or behind n_s.  The stage's three random streams are disjoint from each other and
 * from both of DI's (fourth sampler coordinate 0x80000000 + 3 * frame + pass).
 * With trhip_restir_gi_set_bounces(B > 1) the initial launch continues the path from x_s over B - 1 further vertices, each found by a
 * cosine-hemisphere ray from the one before it and lit by one light sample of its own: L_o = the sum over the vertices of throughput *
 * light sample (no emission, no Russian roulette); the null-sample test, the target and the reservoirs take that sum.
 * Limits:
 *   1. L_o is the radiance x_s sent towards the pixel that found it and is not evaluated again for a pixel that reuses the sample: the
 *      paper's Lambertian assumption, a bias on glossy secondary surfaces.
 *   2. No transmission: the contribution is 0 below the flat normal.
 *   3. A surface with roughness below 0.001 gets no specular indirect light (no delta lobes).
 *   4. History samples are not validated again when geometry or lights move; max_confidence bounds their age.
 *   5. Sphere lights are points, as in DI.  Cosine-hemisphere sampling only, at most 8 bounces without Russian roulette, one device. */
typedef struct trhip_restir_gi trhip_restir_gi;
typedef struct trhip_restir_gi_options {
    uint32_t spatial_samples;         /* 0..4 */
    float search_radius;              /* pixels, > 0, at most 1024 */
    float max_confidence;             /* >= 1, the clamp of the temporal merge */
    int32_t temporal_reuse;           /* 0 / 1 */
    float min_ray_dist;               /* > 0 */
    uint32_t rng_seed;                /* raw; pcg() applied if non-zero, as the path tracer's */
    int32_t record;                   /* keep the decision records (test hook) */
} trhip_restir_gi_options;
typedef struct trhip_restir_gi_reservoir {    /* the null sample has n_s = 0 and L_o = 0 */
    float x_s[3], uc_weight;
    float n_s[3], target_function;
    float L_o[3], confidence;
} trhip_restir_gi_reservoir;
typedef struct trhip_restir_gi_initial {      /* per pixel; the last row is the temporal kernel's update_reservoir of the initial sample */
    float draw[2], pdf; uint32_t traced;      /* unit .xy of the direction's draw; traced: the secondary ray was cast */
    float dir[3], t;                          /* the secondary ray and its hit as trace_closest4 returns it, instance_id -1: none */
    int32_t instance_id, primitive_id; float u, v;
    uint32_t light_draw[4];                   /* the four words sample_canonical took at x_s */
    float L_o[3], target;                     /* L_o: the sum over the path's vertices; target: of the initial sample at the pixel (visibility 1) */
    float weight, sel_draw; uint32_t selected, pad;
} trhip_restir_gi_initial;
typedef struct trhip_restir_gi_path {         /* per pixel and extra vertex k + 1 = 2 .. bounces; nine aligned 16-byte words */
    float draw[2], pdf; uint32_t traced;      /* unit .xy of the direction's draw at vertex k, its pdf; traced: the ray was cast */
    float dir[3], t;                          /* the ray from vertex k and its hit as trace_closest4 returns it, instance_id -1: none */
    int32_t instance_id, primitive_id; float u, v;
    uint32_t light_draw[4];                   /* the four words sample_canonical took at vertex k + 1 */
    uint32_t light; float light_data[2], light_pdf;    /* the light sample as trhip_restir_di_candidate has it; no sample: index 2^30 - 1 */
    float contribution[3], visibility;
    float factor[3], pad0;                    /* contribution of vertex k + 1 (radiance 1) at vertex k, / pdf */
    float throughput[3], pad1;                /* T_{k+1}; 0 where no hit formed it */
    float L_o[3], pad2;                       /* the running sum behind this vertex */
} trhip_restir_gi_path;
typedef struct trhip_restir_gi_timings {      /* device ms of the last render */
    float initial_ms, temporal_ms, spatial_ms, total_ms;
    uint32_t frames;
    char initial_name[64], temporal_name[64], spatial_name[64];    /* "restir gi initial", "restir gi temporal", "restir gi spatial" */
} trhip_restir_gi_timings;
/* Refuses a null device (there is no CPU fallback), zero or oversized dimensions and every option outside its range. */
int trhip_restir_gi_create(trhip_device* dev, const trhip_restir_gi_options* opt, uint32_t width, uint32_t height, uint32_t layers, trhip_restir_gi** out);
void trhip_restir_gi_destroy(trhip_restir_gi* stage);
int trhip_restir_gi_reset(trhip_restir_gi* stage);        /* forgets the history and restarts the frame counter */
/* The vertices of a sample's path behind the pixel, 1..8; 1 after create: L_o is one light sample at x_s.  Refuses a count outside 1..8,
 * a null stage, and, while the stage holds history (a frame since create or reset), another count than the history's: a reservoir does
 * not mix the samples of two estimators.  With record the path records are allocated here. */
int trhip_restir_gi_set_bounces(trhip_restir_gi* stage, uint32_t bounces);
/* One frame of `count` viewports (at most the stage's layers), three launches per 64, asynchronous on `stream`: out_color_dev RGBA32F
 * [count][h][w] = in_color_dev + indirect light; in_color_dev may be null ((0, 0, 0, 1) everywhere) or out_color_dev itself.  Refuses a
 * device without a scene or acceleration structure and a viewport out of range.  History is kept per layer, the position in the list:
 * with temporal_reuse, a list that differs from the last frame's is refused until trhip_restir_gi_reset. */
int trhip_restir_gi_render(trhip_restir_gi* stage, int projection, const uint32_t* viewports, uint32_t count, const void* in_color_dev, void* out_color_dev,
                           void* stream);
int trhip_restir_gi_get_timings(trhip_restir_gi* stage, trhip_restir_gi_timings* out);   /* waits for the last render */
#define TRHIP_RESTIR_GI_SURFACE 0     /* trhip_restir_di_surface [layers][h][w] of the last frame */
#define TRHIP_RESTIR_GI_CANONICAL 1   /* trhip_restir_gi_reservoir [layers][h][w]: what the temporal kernel wrote */
#define TRHIP_RESTIR_GI_HISTORY 2     /* trhip_restir_gi_reservoir [layers][h][w]: what the spatial kernel wrote */
#define TRHIP_RESTIR_GI_INITIAL 3     /* trhip_restir_gi_initial [layers][h][w] (record only, as the five below) */
#define TRHIP_RESTIR_GI_SECONDARY 4   /* trhip_restir_di_surface [layers][h][w]: x_s's surface record, instance_id -1 without a secondary hit */
#define TRHIP_RESTIR_GI_LIGHT 5       /* trhip_restir_di_candidate [layers][h][w]: the light sample at x_s (weight, draw, selected are 0) */
#define TRHIP_RESTIR_GI_TEMPORAL 6    /* trhip_restir_di_temporal [layers][h][w] */
#define TRHIP_RESTIR_GI_SPATIAL 7     /* trhip_restir_di_spatial [layers][h][w][spatial_samples] */
#define TRHIP_RESTIR_GI_FINAL 8       /* trhip_restir_di_final [layers][h][w] */
#define TRHIP_RESTIR_GI_PATH 9        /* trhip_restir_gi_path [layers][h][w][bounces - 1] (record and bounces > 1 only, as the one below) */
#define TRHIP_RESTIR_GI_PATH_SURFACE 10   /* trhip_restir_di_surface [layers][h][w][bounces - 1]: the extra vertices, instance_id -1 where the lane had ended */
int trhip_restir_gi_download(trhip_restir_gi* stage, int which, void* host, size_t bytes);   /* test hook; synchronises the device */

#ifdef __cplusplus
}
#endif
#endif
