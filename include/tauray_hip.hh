// tauray_hip.hh - C++17 host layer over the trhip C ABI, keeping Tauray's renderer/stage surface for the
// path-tracer hot path (header-only; link with -ltrhip).
//
// Class and function names, option fields and the render() sequence follow the reference:
//   distribution_strategy / distribution_params ... src/distribution_strategy.{hh,cc}
//   scene_stage .................................... src/scene_stage.{hh,cc} (uploads + acceleration structure)
//   path_tracer_stage (+ options) .................. src/path_tracer_stage.{hh,cc}, rt_camera_stage, rt_stage
//   stitch_stage, tonemap_stage .................... src/stitch_stage.{hh,cc}, src/tonemap_stage.{hh,cc}
//   rt_renderer .................................... src/rt_renderer.{hh,cc}: per-device stages, transfer, stitch, tonemap
//   headless ....................................... src/headless.{hh,cc}: readback, NaN report, file naming, EXR/RAW writers
//   load_balancer .................................. src/load_balancer.{hh,cc}
// Errors are thrown as std::runtime_error carrying trhip_last_error(), like the reference.
#ifndef TAURAY_HIP_HH
#define TAURAY_HIP_HH
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#ifdef TAURAY_HIP_WITH_ZLIB
#include <zlib.h>
#endif

#include "trhip.h"
#include "tauray_exr.hh"

namespace tr
{

inline void check(int rc)
{
    if(rc != 0) throw std::runtime_error(trhip_last_error());
}

struct uvec2 { uint32_t x = 0, y = 0; };

// A struct option of the reference (TR_STRUCT_OPT, src/options.cc): comma-separated values, positional in the order of `names` or name=value
inline std::map<std::string, std::string> parse_struct_option(const std::string& option, const std::string& text, const std::vector<std::string>& names)
{
    std::map<std::string, std::string> out;
    std::stringstream ss(text); std::string tok;
    size_t position = 0;
    while(std::getline(ss, tok, ','))
    {
        const size_t eq = tok.find('=');
        std::string name;
        if(eq == std::string::npos)
        {
            if(position >= names.size()) throw std::runtime_error(option + ": more than " + std::to_string(names.size()) + " values");
            name = names[position++];
        }
        else
        {
            name = tok.substr(0, eq); tok = tok.substr(eq + 1);
            if(std::find(names.begin(), names.end(), name) == names.end()) throw std::runtime_error(option + ": " + name + " is not one of its fields");
        }
        if(tok.empty()) throw std::runtime_error(option + ": " + name + " has no value");
        out[name] = tok;
    }
    return out;
}
inline double struct_number(const std::string& option, const std::map<std::string, std::string>& v, const std::string& name, double fallback)
{
    auto it = v.find(name);
    if(it == v.end()) return fallback;
    size_t used = 0;
    double d = 0;
    try { d = std::stod(it->second, &used); } catch(std::exception&) { used = 0; }
    if(used != it->second.size()) throw std::runtime_error(option + ": " + name + "=" + it->second + " is not a number");
    return d;
}

//==============================================================================
// distribution_strategy.hh
//==============================================================================
enum distribution_strategy
{
    DISTRIBUTION_DUPLICATE = 0,
    DISTRIBUTION_SCANLINE = 1,
    DISTRIBUTION_SHUFFLED_STRIPS = 2
};

struct distribution_params
{
    uvec2 size;
    distribution_strategy strategy = DISTRIBUTION_SCANLINE;
    unsigned index = 0;
    unsigned count = 1;
    bool primary = true;
};

inline uvec2 get_distribution_render_size(const distribution_params& p)
{
    switch(p.strategy)
    {
    case DISTRIBUTION_DUPLICATE: return p.size;
    case DISTRIBUTION_SCANLINE: return uvec2{p.size.x, (p.size.y - p.index + p.count - 1) / p.count};
    default: return uvec2{p.count, 1};
    }
}

inline uvec2 get_distribution_target_size(const distribution_params& p)
{
    if(p.primary) return p.size;
    if(p.strategy == DISTRIBUTION_SHUFFLED_STRIPS) return uvec2{p.size.x, (p.count + p.size.x - 1) / p.size.x};
    return get_distribution_render_size(p);
}

// src/distribution_strategy.cc:21-31 returns the frame size for shuffled strips.  The ids a device can be handed reach past the
// pixel count, though: the 2^b regions are padded to a common size (45 x 51 = 2 295 pixels are 16 regions of 144 = 2 304 ids), a
// device with (nearly) the whole frame gets `count` > pixels, and its partial image - `count` pixels in rows of size.x - is a row
// taller than the frame.  The reference's targets are Vulkan images, whose out-of-bounds stores are dropped and whose padded ids
// fall on no pixel anyway; a linear buffer needs the padded range, or the last valid pixels of such a share are written past its end
// (found by tests/test_cpp_host.py::test_cpp_random_multi_device_runs: workloads 0, 1 on two devices).
inline uvec2 get_distribution_target_max_size(const distribution_params& p)
{
    if(p.strategy == DISTRIBUTION_SHUFFLED_STRIPS)
    {
        unsigned n = p.size.x * p.size.y, b = 31;
        while((n >> b) < 128 && b > 0) b--;                  // calculate_shuffled_strips_b
        const size_t regions = size_t(1) << b, padded = ((size_t(n) + regions - 1) / regions) << b;
        return uvec2{p.size.x, (unsigned)((padded + p.size.x - 1) / p.size.x)};
    }
    return get_distribution_target_size(p);
}

inline uvec2 get_ray_count(const distribution_params& p)
{
    if(p.strategy == DISTRIBUTION_SHUFFLED_STRIPS) return uvec2{p.count, 1};
    return get_distribution_render_size(p);
}

inline unsigned calculate_shuffled_strips_b(uvec2 size)
{
    unsigned n = size.x * size.y;
    unsigned b = 31;
    while((n >> b) < 128 && b > 0) b--;
    return b;
}

inline unsigned calculate_shuffled_strips_pixels_per_device(uvec2 size, float max_ratio)
{
    unsigned b = calculate_shuffled_strips_b(size);
    size_t n_regions = size_t(1) << b;
    size_t region = (size_t(size.x) * size.y + n_regions - 1) / n_regions;
    return (unsigned)std::ceil(max_ratio * region * (1 << b));
}

inline distribution_params get_device_distribution_params(
    uvec2 full_image_size, distribution_strategy strategy, double workload_offset, double workload_size,
    unsigned device_index, unsigned device_count, bool primary
){
    distribution_params d;
    d.strategy = strategy;
    d.size = full_image_size;
    d.primary = primary;
    if(strategy == DISTRIBUTION_SHUFFLED_STRIPS)
    {
        unsigned before = calculate_shuffled_strips_pixels_per_device(full_image_size, workload_offset);
        unsigned after = calculate_shuffled_strips_pixels_per_device(full_image_size, workload_offset + workload_size);
        d.index = before;
        d.count = after - before;
    }
    else
    {
        d.index = device_index;
        d.count = device_count;
    }
    return d;
}

inline trhip_distribution to_abi(const distribution_params& p)
{
    return trhip_distribution{p.size.x, p.size.y, (int32_t)p.strategy, p.index, p.count, p.primary ? 1u : 0u};
}

//==============================================================================
// device (context holds one per HIP device; --fake-devices repeats a device, src/context.cc:415-416)
//==============================================================================
class device
{
public:
    explicit device(int hip_device): hip_device(hip_device) { check(trhip_device_create(hip_device, &h)); }
    device(const device&) = delete;
    ~device() { trhip_device_destroy(h); }

    void* alloc(size_t bytes) { void* p = nullptr; check(trhip_malloc(h, bytes, &p)); return p; }
    void free(void* p) { trhip_free(h, p); }
    void sync(void* stream = nullptr) { check(trhip_sync(h, stream)); }
    // Frame slots: a stream per frame in flight (MAX_FRAMES_IN_FLIGHT, src/context.hh:26); `dependencies` between stages on
    // different streams (src/dependency.hh) = stream_wait: `stream` continues once everything now on `on` has finished.
    void* create_stream() { void* st = nullptr; check(trhip_stream_create(h, &st)); return st; }
    void destroy_stream(void* stream) { check(trhip_stream_destroy(h, stream)); }
    void stream_wait(void* stream, void* on) { check(trhip_stream_wait(h, stream, on)); }

    trhip_device* h = nullptr;
    int hip_device;
};

//==============================================================================
// scene: the flattened scene_stage inputs (SURVEY.md Appendix A arrays)
//==============================================================================
struct gltf_animation;      // node tree + animation clips of a loaded glTF file (include/tauray_gltf.hh)

// sh_grid + its transformable (src/sh_grid.{hh,cc}; TR_data.light_probe of type GRID, src/gltf.cc:462-481): a grid of light probes in the box
// the transform maps [-1, 1]^3 onto.
struct sh_grid
{
    uint32_t resolution[3] = {1, 1, 1};
    float radius = 0.0f;
    float transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // get_global_transform(), column-major
    float scaling[3] = {1, 1, 1};                                               // get_scaling(), made absolute
    int order = 2;                                                              // sh_grid::set_order (--sh-order)
    static int get_coef_count(int order) { return (order + 1) * (order + 1); }
};

struct scene_data
{
    std::vector<uint8_t> instances, spans, vertices, indices, point_lights, directional_lights, texture_infos, texels,
        envmap, alias_table, cameras, non_opaque;
    uint32_t envmap_width = 0, envmap_height = 0;
    float environment_factor[4] = {0, 0, 0, 0};
    uint32_t gather_emissive_triangles = 0;
    uint32_t projection = 0;
    // Skinned vertex groups (mesh::get_skin + model::get_joints, src/mesh.hh:32-36, src/model.hh): the instance's vertices above are
    // the bind pose; `joint_transforms` (column-major mat4 per joint: global transform of the joint node * inverse bind matrix,
    // model::update_joints src/model.cc:107-118) is the pose scene_stage::set_scene applies - the file's rest pose when a loader
    // filled it in.  Not part of the .trsc dump.
    struct skinned_mesh { uint32_t instance = 0; std::vector<trhip_skin> skins; std::vector<float> joint_transforms; };
    std::vector<skinned_mesh> skinned;
    // Vertex groups with morph targets (tauray_amd/csrc/morph.h): the target-major delta planes float[target_count][vertices][3] (normal /
    // tangent planes empty when no target carries them), the weights now (the file's defaults until tr::scene_animator plays a `weights`
    // channel) and the glTF node that drives them.  Not part of the .trsc dump, like the skins.
    struct morphed_mesh { uint32_t instance = 0, target_count = 0; std::vector<float> position_deltas, normal_deltas, tangent_deltas, weights; int node = -1; };
    std::vector<morphed_mesh> morphed;
    // What tr::scene_animator needs to play the file's animation clips (tauray_gltf.hh); null for scenes without a node tree.
    std::shared_ptr<gltf_animation> animation;
    std::vector<uint8_t> previous_cameras;       // camera_pair.previous of the current frame (empty = the cameras themselves)
    std::vector<sh_grid> sh_grids;               // the file's light-probe grids, in node order (not part of the .trsc dump)

    uint32_t instance_count() const { return (uint32_t)(instances.size() / 288); }
    uint32_t camera_count() const { return (uint32_t)(cameras.size() / 320); }
    uint32_t point_light_count() const { return (uint32_t)(point_lights.size() / 64); }
    uint32_t directional_light_count() const { return (uint32_t)(directional_lights.size() / 32); }
    bool has_tri_lights() const
    {
        for(uint32_t i = 0; i < instance_count(); ++i)
        {
            const float* e = reinterpret_cast<const float*>(instances.data() + 288 * i + 208 + 32);   // mat.emission_factor
            if(e[0] != 0 || e[1] != 0 || e[2] != 0) return true;
        }
        return false;
    }
};

// .trsc reader (written by tauray_amd/scene_io.py)
inline scene_data load_scene_dump(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if(!f) throw std::runtime_error("Failed to open " + path);
    char magic[4]; uint32_t version = 0;
    f.read(magic, 4); f.read(reinterpret_cast<char*>(&version), 4);
    if(std::memcmp(magic, "TRSC", 4) != 0 || version != 1) throw std::runtime_error(path + " is not a version-1 scene dump");
    scene_data s;
    std::vector<uint8_t>* sections[] = {&s.instances, &s.spans, &s.vertices, &s.indices, &s.point_lights, &s.directional_lights,
        &s.texture_infos, &s.texels, &s.envmap, &s.alias_table, &s.cameras, &s.non_opaque};
    for(auto* sec: sections)
    {
        uint64_t n = 0;
        f.read(reinterpret_cast<char*>(&n), 8);
        sec->resize(n);
        f.read(reinterpret_cast<char*>(sec->data()), (std::streamsize)n);
    }
    f.read(reinterpret_cast<char*>(&s.envmap_width), 4);
    f.read(reinterpret_cast<char*>(&s.envmap_height), 4);
    f.read(reinterpret_cast<char*>(s.environment_factor), 16);
    f.read(reinterpret_cast<char*>(&s.gather_emissive_triangles), 4);
    f.read(reinterpret_cast<char*>(&s.projection), 4);
    if(!f) throw std::runtime_error(path + " is truncated");
    return s;
}

class scene_stage
{
public:
    // scene_stage::options::group_strategy (src/scene_stage.hh): how the acceleration structure is laid out (trhip_scene_set_accel_strategy;
    // TRHIP_AS_ALL_MERGED by default, the reference's `all-merged`) and which instances are dynamic (the reference's
    // !static_mesh || !static_transformable; one mark per instance, empty = all static).
    struct options
    {
        int as_strategy = TRHIP_AS_ALL_MERGED;
        std::vector<uint8_t> dynamic;
        // trhip_scene_set_deformation_motion: screen motion follows the deformation of skinned and morphed meshes;
        // apply() then latches their positions before it morphs and skins.  Off: their rigid motion only, the reference's ray-traced path.
        bool deformation_motion = false;
    };
    explicit scene_stage(device& dev): dev(&dev) {}
    scene_stage(device& dev, const options& opt): dev(&dev), opt(opt) {}

    void set_scene(const scene_data& s)
    {
        trhip_scene_desc d = {};
        d.instances = s.instances.data(); d.spans = s.spans.data(); d.instance_count = s.instance_count();
        d.vertices = s.vertices.data(); d.vertex_count = (uint32_t)(s.vertices.size() / 48);
        d.indices = reinterpret_cast<const uint32_t*>(s.indices.data()); d.index_count = (uint32_t)(s.indices.size() / 4);
        d.point_lights = s.point_lights.data(); d.point_light_count = s.point_light_count();
        d.directional_lights = s.directional_lights.data(); d.directional_light_count = s.directional_light_count();
        d.texture_infos = s.texture_infos.data(); d.texture_count = (uint32_t)(s.texture_infos.size() / 16);
        d.texels = s.texels.data();
        if(!s.envmap.empty())
        {
            d.envmap = reinterpret_cast<const float*>(s.envmap.data());
            d.envmap_width = s.envmap_width; d.envmap_height = s.envmap_height;
            d.alias_table = s.alias_table.data();
        }
        std::memcpy(d.environment_factor, s.environment_factor, 16);
        d.cameras = s.cameras.data(); d.camera_count = s.camera_count();
        d.non_opaque = s.non_opaque.data();
        d.gather_emissive_triangles = s.gather_emissive_triangles;
        check(trhip_scene_upload(dev->h, &d));
        // the device handle keeps the switch over uploads; set behind the upload, so that a plane is never filled for the scene that leaves
        check(trhip_scene_set_deformation_motion(dev->h, opt.deformation_motion ? 1 : 0));
        // skinned meshes: the uploaded vertices are the bind pose; pose them before the build (the reference runs skinning.comp on
        // the first scene update, src/scene_stage.cc:1543-1567)
        // morph targets come ahead of skinning (glTF 2.0 section 3.7.2.2): the skins are set first, so that a morphed and skinned mesh
        // morphs its bind pose, the file's default weights are applied, and the rest pose skins the result
        for(const scene_data::skinned_mesh& sk: s.skinned) set_skin(sk.instance, sk.skins.data(), (uint32_t)sk.skins.size());
        for(const scene_data::morphed_mesh& mm: s.morphed)
        {
            set_morph_targets(mm.instance, mm.target_count, mm.position_deltas.data(), mm.normal_deltas.empty() ? nullptr : mm.normal_deltas.data(),
                              mm.tangent_deltas.empty() ? nullptr : mm.tangent_deltas.data(), (uint32_t)(mm.position_deltas.size() / (3 * (size_t)std::max(mm.target_count, 1u))));
            morph(mm.instance, mm.weights.data(), (uint32_t)mm.weights.size());
        }
        for(const scene_data::skinned_mesh& sk: s.skinned) skin(sk.instance, sk.joint_transforms.data(), (uint32_t)(sk.joint_transforms.size() / 16));
        if(opt.deformation_motion) latch_positions();      // the plane was filled with the uploaded bind pose: a still scene has previous = current
        check(trhip_scene_set_accel_strategy(dev->h, opt.as_strategy));
        if(!opt.dynamic.empty())
        {
            if(opt.dynamic.size() != s.instance_count()) throw std::runtime_error("scene_stage: one dynamic mark per instance");
            check(trhip_scene_set_dynamic_instances(dev->h, opt.dynamic.data(), (uint32_t)opt.dynamic.size()));
        }
        check(trhip_scene_set_build_mode(dev->h, 0));     // first build of a scene: ePreferFastTrace
        check(trhip_scene_build_accel(dev->h, &accel));
    }
    trhip_accel_layout layout() const { trhip_accel_layout l; check(trhip_scene_get_accel_layout(dev->h, &l)); return l; }

    // Per-frame scene changes of scene_stage::update (src/scene_stage.cc:1066-1116, 1543-1612).  `update_acceleration`
    // keeps the tree and recomputes its boxes (a BLAS/TLAS update) or, with `rebuild`, builds it again on the device.
    void update_instances(const void* instances_288, uint32_t count) { check(trhip_scene_update_instances(dev->h, instances_288, count)); }
    void set_previous_cameras(const void* camera_data_320, uint32_t count) { check(trhip_scene_set_previous_cameras(dev->h, camera_data_320, count)); }
    // mesh(mesh* animation_source) + mesh::skin_data: bind pose (nullptr = the uploaded vertices) and one skin per vertex
    void set_skin(uint32_t instance, const trhip_skin* skins, uint32_t vertex_count, const void* source_vertices_48 = nullptr)
    {
        check(trhip_scene_set_skin(dev->h, instance, source_vertices_48, skins, vertex_count));
    }
    // model::update_joints + shader/skinning.comp: column-major mat4 per joint
    void skin(uint32_t instance, const float* joint_transforms, uint32_t joint_count) { check(trhip_scene_skin(dev->h, instance, joint_transforms, joint_count)); }
    // morph targets (tauray_amd/csrc/morph.h): delta planes float[target_count][vertex_count][3] (normals / tangents may be nullptr) over the
    // instance's vertices as they stand, or over the bind pose of its skin (set_skin comes first); morph() evaluates them with new weights
    void set_morph_targets(uint32_t instance, uint32_t target_count, const float* position_deltas, const float* normal_deltas, const float* tangent_deltas, uint32_t vertex_count)
    {
        check(trhip_scene_set_morph_targets(dev->h, instance, target_count, position_deltas, normal_deltas, tangent_deltas, vertex_count));
    }
    void morph(uint32_t instance, const float* weights, uint32_t weight_count) { check(trhip_scene_morph(dev->h, instance, weights, weight_count)); }
    // Motion of deforming meshes: the switch (kept over scenes), and the latch of the positions of every skinned or morphed mesh as the
    // previous positions of the frame to come - once per frame, before morph() and skin(); nothing happens while the switch is off.
    void set_deformation_motion(bool on) { check(trhip_scene_set_deformation_motion(dev->h, on ? 1 : 0)); opt.deformation_motion = on; }
    void latch_positions() { check(trhip_scene_latch_positions(dev->h)); }
    void update_cameras(const void* camera_data_320, uint32_t count) { check(trhip_scene_update_cameras(dev->h, camera_data_320, count)); }
    // One frame's worth of scene changes (scene_stage::update after update(scene, dt), src/scene.cc:226-235): the instance records,
    // joint matrices and cameras of `s` - as tr::scene_animator::update left them - go to the device and the acceleration
    // structure is updated once.  With `deformation_motion` (by default: as the switch stands) the positions are latched first: latch,
    // morph, skin, one refit.
    void apply(const scene_data& s, bool rebuild = false) { apply(s, rebuild, opt.deformation_motion); }
    void apply(const scene_data& s, bool rebuild, bool deformation_motion)
    {
        update_instances(s.instances.data(), s.instance_count());
        if(deformation_motion) latch_positions();
        for(const scene_data::morphed_mesh& mm: s.morphed) morph(mm.instance, mm.weights.data(), (uint32_t)mm.weights.size());      // morph, then skin, then one refit
        for(const scene_data::skinned_mesh& sk: s.skinned) skin(sk.instance, sk.joint_transforms.data(), (uint32_t)(sk.joint_transforms.size() / 16));
        update_cameras(s.cameras.data(), s.camera_count());
        if(!s.previous_cameras.empty()) set_previous_cameras(s.previous_cameras.data(), (uint32_t)(s.previous_cameras.size() / 320));
        if(s.point_light_count() || s.directional_light_count())
            check(trhip_scene_update_lights(dev->h, s.point_lights.data(), s.point_light_count(), s.directional_lights.data(), s.directional_light_count()));
        update_acceleration(rebuild);
    }
    void update_acceleration(bool rebuild = false)
    {
        // geometry that is rebuilt after its first build is dynamic: ePreferFastBuild (src/acceleration_structure.cc:129-131)
        if(rebuild) check(trhip_scene_set_build_mode(dev->h, 1));
        check(rebuild ? trhip_scene_build_accel(dev->h, &accel) : trhip_scene_refit_accel(dev->h, &accel));
    }

    device* dev;
    options opt;
    trhip_accel_info accel = {};
};

//==============================================================================
// rt_common.hh enums + path_tracer_stage
//==============================================================================
enum class film_filter { POINT = 0, BOX, BLACKMAN_HARRIS };
enum class multiple_importance_sampling_mode { MIS_DISABLED, MIS_BALANCE_HEURISTIC, MIS_POWER_HEURISTIC };
enum class bounce_sampling_mode { HEMISPHERE, COSINE_HEMISPHERE, MATERIAL };
enum class tri_light_sampling_mode { AREA, SOLID_ANGLE, HYBRID };
enum class sampler_type { UNIFORM_RANDOM = 0, SOBOL_OWEN, SOBOL_Z_ORDER_2D, SOBOL_Z_ORDER_3D };

struct light_sampling_weights
{
    float point_lights = 1.0f;
    float directional_lights = 1.0f;
    float envmap = 1.0f;
    float emissive_triangles = 1.0f;
};

class path_tracer_stage
{
public:
    // rt_stage::options + rt_camera_stage::options + path_tracer_stage::options; defaults are the reference's
    // CLI defaults (src/options.hh), not the struct defaults, because that is what `tauray scene.glb` renders with.
    struct options
    {
        int max_ray_depth = 8;
        float min_ray_dist = 1e-4f;
        int rng_seed = 0;
        sampler_type local_sampler = sampler_type::UNIFORM_RANDOM;
        distribution_params distribution;
        size_t active_viewport_count = 1;
        int samples_per_pixel = 1;
        int samples_per_pass = 1;
        int projection = 0;                 // camera::projection_type
        bool transparent_background = false;
        bool use_white_albedo_on_first_bounce = false;
        bool hide_lights = false;
        bool pre_transformed_vertices = false;   // --pre-transform-vertices (src/options.hh)
        film_filter film = film_filter::POINT;
        multiple_importance_sampling_mode mis_mode = multiple_importance_sampling_mode::MIS_POWER_HEURISTIC;
        float film_radius = 0.5f;
        float russian_roulette_delta = 0;
        float indirect_clamping = 0;
        float regularization_gamma = 0.0f;
        bool depth_of_field = false;
        light_sampling_weights sampling_weights;
        bounce_sampling_mode bounce_mode = bounce_sampling_mode::MATERIAL;
        tri_light_sampling_mode tri_light_mode = tri_light_sampling_mode::SOLID_ANGLE;
    };

    path_tracer_stage(device& dev, scene_stage& ss, void* color_target, const options& opt, bool direct_only = false)
    : dev(&dev), ss(&ss), color(color_target), opt(opt)
    {
        trhip_pt_options o = {};
        o.max_bounces = opt.max_ray_depth; o.min_ray_dist = opt.min_ray_dist; o.rng_seed = (uint32_t)opt.rng_seed;
        o.sampler = (int)opt.local_sampler; o.samples_per_pixel = opt.samples_per_pixel; o.samples_per_pass = opt.samples_per_pass;
        o.projection = opt.projection; o.film = (int)opt.film; o.film_radius = opt.film_radius; o.mis_mode = (int)opt.mis_mode;
        o.russian_roulette_delta = opt.russian_roulette_delta; o.indirect_clamping = opt.indirect_clamping;
        o.regularization_gamma = opt.regularization_gamma; o.depth_of_field = opt.depth_of_field;
        o.nee_point = opt.sampling_weights.point_lights; o.nee_directional = opt.sampling_weights.directional_lights;
        o.nee_envmap = opt.sampling_weights.envmap; o.nee_triangles = opt.sampling_weights.emissive_triangles;
        o.bounce_mode = (int)opt.bounce_mode; o.tri_light_mode = (int)opt.tri_light_mode; o.hide_lights = opt.hide_lights;
        o.use_white_albedo_on_first_bounce = opt.use_white_albedo_on_first_bounce;
        o.transparent_background = opt.transparent_background;
        o.pre_transformed_vertices = opt.pre_transformed_vertices;
        check(direct_only ? trhip_direct_create(dev.h, &o, &pt) : trhip_pt_create(dev.h, &o, &pt));
        reset_distribution_params(opt.distribution);
    }
    path_tracer_stage(const path_tracer_stage&) = delete;
    ~path_tracer_stage() { trhip_pt_destroy(pt); }

    void reset_accumulated_samples() { check(trhip_pt_reset_accumulation(pt, 0)); }
    void reset_sample_counter() { check(trhip_pt_reset_accumulation(pt, 1)); }
    void reset_distribution_params(distribution_params distribution)
    {
        opt.distribution = distribution;
        trhip_distribution d = to_abi(distribution);
        check(trhip_pt_set_distribution(pt, &d));
    }
    // one stage per frame slot: slot k of F renders frames k, k + F, ... (rt_stage::frame_counter, src/rt_stage.cc:81-86)
    void set_frame_counter(uint32_t frame_counter) { check(trhip_pt_set_frame_counter(pt, frame_counter)); }
    // `frames` consecutive frames per run(): the target holds frames * active_viewport_count layers, frame-major (trhip_pt_set_frame_batch)
    void set_frame_batch(uint32_t frames) { check(trhip_pt_set_frame_batch(pt, frames)); frame_batch = frames; }
    // slices of a frame run concurrently inside the stage: 0 = automatic, 1 = none (several frames in flight instead)
    void set_lanes(int lanes) { check(trhip_pt_set_lanes(pt, lanes)); }
    void set_frame_slots(int slots) { check(trhip_pt_set_frame_slots(pt, slots)); }
    // the last pass of a frame also writes tonemap(colour) into `display` (a renderer with nothing between this stage and its tonemap stage)
    void set_fused_tonemap(void* display, const trhip_tonemap_info* info) { check(trhip_pt_set_fused_tonemap(pt, display, info)); }
    // which shading program renders this stage (general kernels / the command-line set's ahead-of-time instances / compiled for the option
    // set), resolved now, and its identity - what the devices of a job compare before the first frame (trhip_pt_get_program)
    trhip_program_info program() const { trhip_program_info p; check(trhip_pt_get_program(pt, &p)); return p; }
    // view / sample shard of a multi-device job: global viewport and sample addressing
    void set_shard(uint32_t viewport_base, uint32_t viewport_stride, uint32_t sample_base = 0, uint32_t sample_stride = 1)
    {
        check(trhip_pt_set_shard(pt, viewport_base, viewport_stride, sample_base, sample_stride));
    }
    // stage::run: enqueue the frame (all passes) on `stream` (default: the device's stream)
    void run(void* stream = nullptr)
    {
        uvec2 ts = get_distribution_target_size(opt.distribution);
        check(trhip_pt_render(pt, color, ts.x, ts.y, (uint32_t)opt.active_viewport_count * frame_batch, stream));
    }
    // the same frame into a gbuffer (src/gbuffer.hh: the entries path_tracer.rgen writes); null members are skipped
    using gbuffer_target = trhip_pt_targets;
    void run(const gbuffer_target& targets)
    {
        uvec2 ts = get_distribution_target_size(opt.distribution);
        check(trhip_pt_render_targets(pt, &targets, ts.x, ts.y, (uint32_t)opt.active_viewport_count, nullptr));
    }
    float get_duration_ms() { trhip_timings t; check(trhip_pt_get_timings(pt, &t)); return t.path_tracing_ms; }
    trhip_counters get_counters() { trhip_counters c; check(trhip_pt_get_counters(pt, &c)); return c; }

    device* dev;
    scene_stage* ss;
    void* color;
    options opt;
    trhip_pt* pt = nullptr;
    uint32_t frame_batch = 1;
};

// direct_stage (src/direct_stage.{hh,cc}): first hit + samples_per_pass light samples, same surface as path_tracer_stage.
// Its reference defaults differ (Blackman-Harris film of radius 1, hybrid tri-light sampling): set them in `options`.
class direct_stage: public path_tracer_stage
{
public:
    direct_stage(device& dev, scene_stage& ss, void* color_target, const options& opt)
    : path_tracer_stage(dev, ss, color_target, opt, true) {}
};

//==============================================================================
// tonemap_stage / load_balancer
//==============================================================================
class tonemap_stage
{
public:
    enum operator_type { LINEAR = 0, GAMMA_CORRECTION, FILMIC, REINHARD, REINHARD_LUMINANCE };
    struct options
    {
        operator_type tonemap_operator = FILMIC;
        float exposure = 1.0f;
        float gamma = 2.2f;
        bool alpha_grid_background = false;
    };
    tonemap_stage(device& dev, const options& opt): dev(&dev), opt(opt) {}
    trhip_tonemap_info info() const { return {(int32_t)opt.tonemap_operator, opt.exposure, opt.gamma, opt.alpha_grid_background ? 16 : 0}; }
    void run(const void* in, void* out, uvec2 size, uint32_t layers, void* stream = nullptr)
    {
        const trhip_tonemap_info i = info();
        check(trhip_tonemap(dev->h, in, out, size.x, size.y, layers, &i, stream));
    }
    device* dev;
    options opt;
};

// bmfr_stage (src/bmfr_stage.{hh,cc}): the BMFR denoiser between the path tracer and the tonemap stage.  The reference's constructor
// takes the current and the previous gbuffer; here the stage keeps last frame's normal / pos and its histories itself (trhip_bmfr_*),
// so there is one gbuffer: the images trhip_pt_render_targets wrote, `layers` of them of `size`.  color is denoised in place.
class bmfr_stage
{
public:
    enum class bmfr_settings { DIFFUSE_ONLY = TRHIP_BMFR_DIFFUSE_ONLY, DIFFUSE_SPECULAR = TRHIP_BMFR_DIFFUSE_SPECULAR };
    struct options
    {
        bmfr_settings settings = bmfr_settings::DIFFUSE_ONLY;
        float noise_amount = 0.0f;      // 0 = the reference's 1e-2
    };
    bmfr_stage(device& dev, const trhip_bmfr_features& current_features, uvec2 size, uint32_t layers, const options& opt)
    : dev(&dev), features(current_features), opt(opt)
    {
        const trhip_bmfr_options o = {(int32_t)opt.settings, opt.noise_amount};
        check(trhip_bmfr_create(dev.h, &o, size.x, size.y, layers, &h));
    }
    bmfr_stage(const bmfr_stage&) = delete;
    ~bmfr_stage() { trhip_bmfr_destroy(h); }
    // stage::run: one frame on `stream`; frame_counter = context::get_frame_counter()
    void run(uint32_t frame_counter, void* stream = nullptr) { check(trhip_bmfr_run(h, &features, frame_counter, stream)); }
    void reset_history() { check(trhip_bmfr_reset_history(h)); }
    trhip_bmfr_timings get_timings() { trhip_bmfr_timings t; check(trhip_bmfr_get_timings(h, &t)); return t; }

    device* dev;
    trhip_bmfr_features features;
    options opt;
    trhip_bmfr* h = nullptr;
};

// The first-hit G-buffer of viewports that are not path traced (trhip_gbuffer_render): normal, pos and instance id of one ray through every
// pixel centre for a list of viewports in one launch, as compact layers in list order.
class gbuffer_stage
{
public:
    gbuffer_stage(device& dev, uvec2 size, int projection, float min_ray_dist): dev(&dev), size(size), projection(projection), min_ray_dist(min_ray_dist) {}
    void run(const std::vector<uint32_t>& viewports, const trhip_gbuffer_targets& targets, void* stream = nullptr)
    {
        check(trhip_gbuffer_render(dev->h, projection, viewports.data(), (uint32_t)viewports.size(), min_ray_dist, &targets, size.x, size.y, stream));
    }
    device* dev;
    uvec2 size;
    int projection;
    float min_ray_dist;
};

// The active viewports of a sparse light field as arithmetic runs {base, stride, count} in list order - what set_shard expresses:
// 0,4,8 is one run, 18..26 is one run, 0,1,5 is {0, 1, 2}, {5, 1, 1}.
struct viewport_run { uint32_t base, stride, count; };
inline std::vector<viewport_run> viewport_runs(const std::vector<uint32_t>& v)
{
    std::vector<viewport_run> runs;
    for(size_t i = 0; i < v.size();)
    {
        uint32_t count = 1, stride = 1;
        if(i + 1 < v.size() && v[i + 1] > v[i])
        {
            stride = v[i + 1] - v[i];
            while(i + count < v.size() && v[i + count] > v[i + count - 1] && v[i + count] - v[i + count - 1] == stride) ++count;
        }
        runs.push_back({v[i], stride, count});
        i += count;
    }
    return runs;
}

// A non-empty list of distinct viewports of the grid that leaves some to reproject (what both hosts refuse otherwise).
inline void check_viewport_list(const std::vector<uint32_t>& v, size_t total, const std::string& what)
{
    if(v.empty()) throw std::runtime_error(what + ": the viewport list is empty");
    for(uint32_t x: v) if(x >= total) throw std::runtime_error(what + ": viewport " + std::to_string(x) + " is out of range (the scene has " + std::to_string(total) + " viewports)");
    for(size_t i = 0; i < v.size(); ++i) for(size_t j = 0; j < i; ++j) if(v[i] == v[j]) throw std::runtime_error(what + ": a viewport is listed twice");
    if(v.size() >= total) throw std::runtime_error(what + ": the list names every viewport: there is nothing to reproject");
}

// spatial_reprojection_stage (src/spatial_reprojection_stage.{hh,cc}): fills the viewports that were not path traced from the ones that
// were, through the G-buffer (trhip_spatial_reprojection_*).  `source_viewports`: the path-traced viewports in the order of the source
// images' layers; the output holds every viewport in natural order.
class spatial_reprojection_stage
{
public:
    spatial_reprojection_stage(device& dev, uvec2 size, uint32_t total_viewports, const std::vector<uint32_t>& source_viewports)
    : dev(&dev), sources(source_viewports)
    {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        const float default_value[4] = {nan, nan, nan, nan};      // src/spatial_reprojection_stage.cc: what nothing reprojects to
        check(trhip_spatial_reprojection_create(dev.h, size.x, size.y, total_viewports, sources.data(), (uint32_t)sources.size(), default_value, &h));
        for(uint32_t v = 0; v < total_viewports; ++v)
            if(std::find(sources.begin(), sources.end(), v) == sources.end()) destinations.push_back(v);
    }
    spatial_reprojection_stage(const spatial_reprojection_stage&) = delete;
    ~spatial_reprojection_stage() { trhip_spatial_reprojection_destroy(h); }
    void run(const trhip_reprojection_images& source_images, const trhip_reprojection_images& destination_images, void* color_out, void* stream = nullptr)
    {
        check(trhip_spatial_reprojection_run(h, &source_images, &destination_images, color_out, stream));
    }
    trhip_reprojection_timings get_timings() { trhip_reprojection_timings t; check(trhip_spatial_reprojection_get_timings(h, &t)); return t; }

    device* dev;
    std::vector<uint32_t> sources, destinations;
    trhip_spatial_reprojection* h = nullptr;
};

// temporal_reprojection_stage (src/temporal_reprojection_stage.{hh,cc}): color = mix(color, last frame's colour found through
// screen_motion, temporal_ratio) on the path-traced layers; the stage keeps last frame's colour, normal and pos itself.
class temporal_reprojection_stage
{
public:
    struct options { float temporal_ratio = 0.75f; };
    temporal_reprojection_stage(device& dev, uvec2 size, uint32_t layers, const options& opt): dev(&dev), opt(opt)
    {
        check(trhip_temporal_reprojection_create(dev.h, size.x, size.y, layers, opt.temporal_ratio, &h));
    }
    temporal_reprojection_stage(const temporal_reprojection_stage&) = delete;
    ~temporal_reprojection_stage() { trhip_temporal_reprojection_destroy(h); }
    void run(const trhip_reprojection_images& images, void* stream = nullptr) { check(trhip_temporal_reprojection_run(h, &images, stream)); }
    void reset_history() { check(trhip_temporal_reprojection_reset_history(h)); }
    trhip_reprojection_timings get_timings() { trhip_reprojection_timings t; check(trhip_temporal_reprojection_get_timings(h, &t)); return t; }

    device* dev;
    options opt;
    trhip_temporal_reprojection* h = nullptr;
};

// taa_stage (src/taa_stage.{hh,cc}): temporal antialiasing behind the tonemap stage (trhip_taa_*): this frame's display-space colour is
// blended into the stage's history, found through screen_motion with the cameras' jitter (camera_data::pan.zw) removed and clipped to the
// 3 x 3 neighbourhood's k-DOP.  The stage keeps its two history images itself and reads the device scene's cameras / previous cameras.
class taa_stage
{
public:
    struct options
    {
        float blending_ratio = 0.125f;      // alpha: the weight of the new frame, 1 / the length of the jitter sequence
        float gamma = 2.2f;                 // the tonemap stage's (src/post_processing_renderer.cc:215)
        bool edge_dilation = true, anti_shimmer = false;      // src/options.hh:406-411
        uint32_t base_camera_index = 0;
        int projection = 0;
    };
    taa_stage(device& dev, uvec2 size, uint32_t layers, const options& opt): dev(&dev), opt(opt)
    {
        const trhip_taa_options o = {opt.blending_ratio, opt.gamma, opt.edge_dilation ? 1 : 0, opt.anti_shimmer ? 1 : 0, opt.base_camera_index, opt.projection};
        check(trhip_taa_create(dev.h, &o, size.x, size.y, layers, &h));
    }
    taa_stage(const taa_stage&) = delete;
    ~taa_stage() { trhip_taa_destroy(h); }
    void run(const trhip_taa_images& images, void* stream = nullptr) { check(trhip_taa_run(h, &images, stream)); }
    void reset_history() { check(trhip_taa_reset_history(h)); }
    trhip_taa_timings get_timings() { trhip_taa_timings t; check(trhip_taa_get_timings(h, &t)); return t; }

    device* dev;
    options opt;
    trhip_taa* h = nullptr;
};

// looking_glass_composition_stage (src/looking_glass_composition_stage.{hh,cc}): the last stage of a light-field chain (trhip_lkg_*): the
// views of `src` (RGBA32F [views][view_size.y][view_size.x], display space) are interleaved, sub-pixel by sub-pixel, into the one image of
// `output_size` a lenticular panel shows - as RGBA32F and / or as the reference's 8 bits.  pitch, tilt and center are the reference's
// corrected_pitch, tilt and center (looking_glass_calibration of tauray_gltf.hh computes them).  The stage has no history.
class looking_glass_composition_stage
{
public:
    struct options
    {
        uint32_t viewport_count = 48;       // 1..255
        float pitch = 0.0f, tilt = 0.0f, center = 0.0f;
        bool invert = false;
        bool record_view_indices = false;   // keep the view of every sub-pixel for download_view_indices (a test hook)
    };
    looking_glass_composition_stage(device& dev, uvec2 view_size, uvec2 output_size, const options& opt): dev(&dev), view_size(view_size), output_size(output_size), opt(opt)
    {
        const trhip_lkg_options o = {opt.viewport_count, opt.pitch, opt.tilt, opt.center, opt.invert ? 1 : 0, opt.record_view_indices ? 1 : 0};
        check(trhip_lkg_create(dev.h, &o, view_size.x, view_size.y, output_size.x, output_size.y, &h));
    }
    looking_glass_composition_stage(const looking_glass_composition_stage&) = delete;
    ~looking_glass_composition_stage() { trhip_lkg_destroy(h); }
    void run(const void* src, void* dst, void* dst_rgba8 = nullptr, void* stream = nullptr) { check(trhip_lkg_run(h, src, dst, dst_rgba8, stream)); }
    trhip_lkg_timings get_timings() { trhip_lkg_timings t; check(trhip_lkg_get_timings(h, &t)); return t; }
    std::vector<uint8_t> download_view_indices()
    {
        std::vector<uint8_t> out(size_t(output_size.x) * output_size.y * 4);
        check(trhip_lkg_download(h, TRHIP_LKG_VIEW_INDICES, out.data(), out.size()));
        return out;
    }

    device* dev;
    uvec2 view_size, output_size;
    options opt;
    trhip_lkg* h = nullptr;
};

// grid_data_buffer of render number `history_length` (>= 1) of a grid at `frame_counter`, as sh_path_tracer_stage::update packs it
// (src/sh_path_tracer_stage.cc:115-137): transform, normal_transform, cell_scale, the rotations of the direction lattice, mix_ratio.  Needs no device.
inline trhip_sh_grid_data sh_grid_parameters(const sh_grid& g, uint32_t samples_per_probe, uint32_t frame_counter, uint32_t history_length, float temporal_ratio)
{
    trhip_sh_grid_data out;
    check(trhip_sh_pack_grid_data(g.transform, g.scaling, g.resolution, samples_per_probe, frame_counter, history_length, temporal_ratio, &out));
    return out;
}

// sh_path_tracer_stage followed by sh_compact_stage (src/sh_path_tracer_stage.{hh,cc}, src/sh_compact_stage.cc; trhip_sh_*): bakes one sh_grid
// as spherical-harmonics coefficients on the path tracer's kernels.  The stage owns both volumes: RGBA32F [rz][ry * C][rx] and its RGBA16F copy.
class sh_path_tracer_stage
{
public:
    struct options      // the reference's defaults (src/sh_path_tracer_stage.hh:14-31, rt_stage::options)
    {
        int max_ray_depth = 8;
        float min_ray_dist = 1e-4f;
        int rng_seed = 0;
        sampler_type local_sampler = sampler_type::UNIFORM_RANDOM;      // the only one the stage accepts
        int samples_per_probe = 1;
        film_filter film = film_filter::BLACKMAN_HARRIS;
        multiple_importance_sampling_mode mis_mode = multiple_importance_sampling_mode::MIS_POWER_HEURISTIC;
        float film_radius = 1.0f;
        float russian_roulette_delta = 0;
        float temporal_ratio = 0.02f;
        float indirect_clamping = 100.0f;
        float regularization_gamma = 1.0f;
        light_sampling_weights sampling_weights;
        bounce_sampling_mode bounce_mode = bounce_sampling_mode::MATERIAL;
        tri_light_sampling_mode tri_light_mode = tri_light_sampling_mode::SOLID_ANGLE;
        int sh_order = 2;
    };
    sh_path_tracer_stage(device& dev, const sh_grid& grid, const options& opt): dev(&dev), grid(grid), opt(opt)
    {
        trhip_pt_options o = {};
        o.max_bounces = opt.max_ray_depth; o.min_ray_dist = opt.min_ray_dist; o.rng_seed = (uint32_t)opt.rng_seed; o.sampler = (int)opt.local_sampler;
        o.samples_per_pixel = 1; o.samples_per_pass = 1;
        o.film = (int)opt.film; o.film_radius = opt.film_radius; o.mis_mode = (int)opt.mis_mode; o.russian_roulette_delta = opt.russian_roulette_delta;
        o.indirect_clamping = opt.indirect_clamping; o.regularization_gamma = opt.regularization_gamma;
        o.nee_point = opt.sampling_weights.point_lights; o.nee_directional = opt.sampling_weights.directional_lights;
        o.nee_envmap = opt.sampling_weights.envmap; o.nee_triangles = opt.sampling_weights.emissive_triangles;
        o.bounce_mode = (int)opt.bounce_mode; o.tri_light_mode = (int)opt.tri_light_mode;
        trhip_sh_options so = {};
        so.order = opt.sh_order; so.samples_per_probe = (uint32_t)std::max(opt.samples_per_probe, 0); so.temporal_ratio = opt.temporal_ratio;
        for(int i = 0; i < 3; ++i) so.resolution[i] = grid.resolution[i];
        check(trhip_sh_create(dev.h, &o, &so, &h));
        check(trhip_sh_set_transform(h, grid.transform, grid.scaling));
    }
    sh_path_tracer_stage(const sh_path_tracer_stage&) = delete;
    ~sh_path_tracer_stage() { trhip_sh_destroy(h); }
    void set_frame_counter(uint32_t frame_counter) { check(trhip_sh_set_frame_counter(h, frame_counter)); }
    void reset_history() { check(trhip_sh_reset_history(h)); }
    void run(void* stream = nullptr) { check(trhip_sh_render(h, stream)); }
    trhip_sh_timings get_timings() { trhip_sh_timings t; check(trhip_sh_get_timings(h, &t)); return t; }
    trhip_counters get_counters() { trhip_counters c; check(trhip_sh_get_counters(h, &c)); return c; }
    uint32_t coef_count() const { return (uint32_t)sh_grid::get_coef_count(opt.sh_order); }
    // The float volume unfolded to an image of width rx and height ry * C * rz (its rows in memory order)
    uvec2 unfolded_size() const { return uvec2{grid.resolution[0], grid.resolution[1] * coef_count() * grid.resolution[2]}; }
    std::vector<float> download()
    {
        const uvec2 sz = unfolded_size();
        std::vector<float> out(size_t(sz.x) * sz.y * 4);
        check(trhip_sh_download(h, TRHIP_SH_GRID, out.data(), out.size() * sizeof(float)));
        return out;
    }

    device* dev;
    sh_grid grid;
    options opt;
    trhip_sh* h = nullptr;
};

// sh_renderer (src/sh_renderer.{hh,cc}): one sh_path_tracer_stage per sh_grid of the scene, each with the grid's order.
class sh_renderer
{
public:
    using options = sh_path_tracer_stage::options;
    sh_renderer(device& dev, const std::vector<sh_grid>& grids, const options& opt)
    {
        if(grids.empty()) throw std::runtime_error("sh_renderer: the scene has no light-probe grid (TR_data.light_probe of type GRID)");
        for(const sh_grid& g: grids)
        {
            options o = opt;
            o.sh_order = g.order;
            stages.emplace_back(new sh_path_tracer_stage(dev, g, o));
        }
    }
    void render(void* stream = nullptr) { for(auto& s: stages) s->run(stream); }
    std::vector<std::unique_ptr<sh_path_tracer_stage>> stages;
};

// get_sh_grid, then get_largest_sh_grid (src/scene.cc:163-211) for `position`: the index into `grids`, -1 without any.  Needs no device.
inline int dshgi_pick_grid(const std::vector<sh_grid>& grids, const float position[3])
{
    std::vector<float> transforms, scalings, radii;
    std::vector<uint32_t> resolutions;
    for(const sh_grid& g: grids)
    {
        transforms.insert(transforms.end(), g.transform, g.transform + 16);
        scalings.insert(scalings.end(), g.scaling, g.scaling + 3);
        resolutions.insert(resolutions.end(), g.resolution, g.resolution + 3);
        radii.push_back(g.radius);
    }
    int32_t index = -1;
    check(trhip_dshgi_pick_grid(transforms.data(), scalings.data(), resolutions.data(), radii.data(), (uint32_t)grids.size(), position, &index));
    return index;
}

// sh_grid_index of every instance (src/scene_stage.cc:1075-1083): the grid picked for model[3], the instance's origin.
inline std::vector<int32_t> dshgi_instance_grids(const std::vector<sh_grid>& grids, const scene_data& scene)
{
    std::vector<int32_t> out(scene.instance_count());
    for(uint32_t i = 0; i < scene.instance_count(); ++i)
    {
        float p[3];
        std::memcpy(p, scene.instances.data() + 288 * size_t(i) + 16 + 48, sizeof(p));      // model[3].xyz
        out[i] = dshgi_pick_grid(grids, p);
    }
    return out;
}

// The indirect light of dshgi_renderer (shader/forward.frag; trhip_dshgi_*): first hit, SH grid lookup, brdf_indirect, added to the direct
// stage's colour.  `size`, `layers`: the images of a frame.
class dshgi_stage
{
public:
    struct options
    {
        int sh_order = 2;
        bool use_probe_visibility = false;      // --use-probe-visibility; off = SH_INTERPOLATION_TRILINEAR
        bool record_surface = false;
        int projection = 0;
        float min_ray_dist = 1e-4f;
    };
    dshgi_stage(device& dev, uvec2 size, uint32_t layers, const options& opt): dev(&dev), size(size), layers(layers), opt(opt)
    {
        trhip_dshgi_options o = {};
        o.order = opt.sh_order; o.use_probe_visibility = opt.use_probe_visibility; o.record_surface = opt.record_surface;
        check(trhip_dshgi_create(dev.h, &o, size.x, size.y, layers, &h));
    }
    dshgi_stage(const dshgi_stage&) = delete;
    ~dshgi_stage() { trhip_dshgi_destroy(h); }
    // `images`: the RGBA16F volume of each grid on the device (trhip_sh_get_grids' second image)
    void set_grids(const std::vector<sh_grid>& grids, const std::vector<const void*>& images)
    {
        std::vector<trhip_dshgi_grid> g(grids.size());
        for(size_t i = 0; i < grids.size(); ++i)
        {
            g[i].grid_half_dev = images[i];
            std::memcpy(g[i].resolution, grids[i].resolution, sizeof(g[i].resolution));
            std::memcpy(g[i].transform, grids[i].transform, sizeof(g[i].transform));
            std::memcpy(g[i].scaling, grids[i].scaling, sizeof(g[i].scaling));
        }
        check(trhip_dshgi_set_grids(h, g.data(), (uint32_t)g.size()));
    }
    void set_instance_grids(const std::vector<int32_t>& v) { check(trhip_dshgi_set_instance_grids(h, v.data(), (uint32_t)v.size())); }
    void set_brdf_integration(const void* table_dev, uint32_t w, uint32_t h_) { check(trhip_dshgi_set_brdf_integration(h, table_dev, w, h_)); }
    // out = direct + indirect for the listed viewports; a null `direct` writes the indirect term alone, `out` may be `direct`
    void run(const std::vector<uint32_t>& viewports, const void* direct, void* out, void* stream = nullptr)
    {
        check(trhip_dshgi_render(h, opt.projection, viewports.data(), (uint32_t)viewports.size(), opt.min_ray_dist, direct, out, stream));
    }
    trhip_dshgi_timings get_timings() { trhip_dshgi_timings t; check(trhip_dshgi_get_timings(h, &t)); return t; }

    device* dev;
    uvec2 size;
    uint32_t layers;
    options opt;
    trhip_dshgi* h = nullptr;
};

// What the single-device renderers of whole viewports share (dshgi_renderer, restir_di_renderer, restir_gi_renderer): the zeroed `color` and `display` images of
// every viewport (one per camera), the tonemap stage, the list of all viewports and the tail of a frame that tonemaps it.  A derived
// renderer's destructor releases the stages that write the images; the images go after them.
class viewport_frame_renderer
{
public:
    viewport_frame_renderer(device& dev, const scene_data& scene, uvec2 size, const tonemap_stage::options& tonemap_opt)
    : dev(&dev), size(size), viewports(std::max(scene.camera_count(), 1u))
    {
        const size_t bytes = size_t(size.x) * size.y * 16 * viewports;
        color = dev.alloc(bytes); display = dev.alloc(bytes);
        check(trhip_memset(dev.h, color, 0, bytes, nullptr));
        check(trhip_memset(dev.h, display, 0, bytes, nullptr));
        tonemap.reset(new tonemap_stage(dev, tonemap_opt));
        for(uint32_t v = 0; v < viewports; ++v) viewport_list.push_back(v);
    }
    viewport_frame_renderer(const viewport_frame_renderer&) = delete;
    ~viewport_frame_renderer() { dev->free(color); dev->free(display); }

    device* dev;
    uvec2 size;
    uint32_t viewports;
    std::unique_ptr<tonemap_stage> tonemap;
    std::vector<uint32_t> viewport_list;
    void* color = nullptr;
    void* display = nullptr;

protected:
    void finish_frame(void* stream) { tonemap->run(color, display, size, viewports, stream); }
};

// dshgi_renderer (src/dshgi_renderer.{hh,cc}): per frame the scene's probe grids are baked (sh_renderer), the direct stage renders every
// viewport, the indirect light of the grids is added (dshgi_stage), the frame is tonemapped - all on one stream.  The first bake has
// history 1, so the grids are complete before they are read.  The reference rasterises and uses shadow maps; here the first hit is a ray
// and direct light is the direct stage.  Direct light is what the reference's raster pass lights with - point and
// directional lights: the direct stage samples neither the emissive triangles nor the environment map (it still shows them where a pixel
// sees them), because the probes see both and the indirect term carries their light.
class dshgi_renderer: public viewport_frame_renderer
{
public:
    struct options
    {
        path_tracer_stage::options direct;      // the direct stage; its distribution is set here
        sh_renderer::options sh;                // the bake
        bool use_probe_visibility = false;
        std::vector<float> brdf_integration;    // RG32F [h][w]; empty = the generated 256 x 256 table of 1024 samples
        uint32_t brdf_integration_width = 0, brdf_integration_height = 0;
        tonemap_stage::options tonemap;
    };
    dshgi_renderer(device& dev, scene_stage& ss, const scene_data& scene, uvec2 size, const options& opt_)
    : viewport_frame_renderer(dev, scene, size, opt_.tonemap), grids(scene.sh_grids), opt(opt_), sh(dev, scene.sh_grids, opt_.sh)
    {
        opt.direct.distribution = distribution_params{size, DISTRIBUTION_DUPLICATE, 0, 1, true};
        opt.direct.active_viewport_count = viewports;
        opt.direct.sampling_weights.emissive_triangles = 0; opt.direct.sampling_weights.envmap = 0;
        direct.reset(new direct_stage(dev, ss, color, opt.direct));
        dshgi_stage::options io;
        io.sh_order = grids[0].order; io.use_probe_visibility = opt.use_probe_visibility; io.projection = opt.direct.projection; io.min_ray_dist = opt.direct.min_ray_dist;
        indirect.reset(new dshgi_stage(dev, size, viewports, io));
        std::vector<const void*> images;
        for(auto& st: sh.stages) { void* half = nullptr; check(trhip_sh_get_grids(st->h, nullptr, &half)); images.push_back(half); }
        indirect->set_grids(grids, images);
        uint32_t tw = 256, th = 256;
        if(!opt.brdf_integration.empty()) { tw = opt.brdf_integration_width; th = opt.brdf_integration_height; }
        void* table = dev.alloc(size_t(tw) * th * 8);
        if(opt.brdf_integration.empty()) check(trhip_brdf_integration_generate(dev.h, tw, 1024, table, nullptr));
        else
        {
            if(opt.brdf_integration.size() != size_t(tw) * th * 2) throw std::runtime_error("dshgi_renderer: the BRDF-integration table is not width * height * 2 floats");
            check(trhip_upload(dev.h, table, opt.brdf_integration.data(), size_t(tw) * th * 8, nullptr));
        }
        dev.sync();
        indirect->set_brdf_integration(table, tw, th);
        dev.free(table);
        set_scene(scene);
    }
    ~dshgi_renderer() { direct.reset(); indirect.reset(); }
    // the instances have moved (the scene stage holds them already): every instance picks its grid again
    void set_scene(const scene_data& scene)
    {
        instance_grids = dshgi_instance_grids(grids, scene);
        indirect->set_instance_grids(instance_grids);
    }
    void render(void* stream = nullptr)
    {
        sh.render(stream);
        direct->reset_accumulated_samples();
        direct->run(stream);
        indirect->run(viewport_list, color, color, stream);
        finish_frame(stream);
    }

    std::vector<sh_grid> grids;
    options opt;
    sh_renderer sh;
    std::unique_ptr<direct_stage> direct;
    std::unique_ptr<dshgi_stage> indirect;
    std::vector<int32_t> instance_grids;
};

// ReSTIR DI (trhip_restir_di_*; written after shader/restir_di.glsl and its two ray generation shaders): per frame the canonical kernel
// (first hit, RIS over light candidates, temporal merge) and the spatial kernel (neighbour merge, shading).  `size`, `layers`: the images
// of a frame.  The decisions where the shaders are stale or undefined are listed in trhip.h and DESIGN.md section 21.
// The options the two ReSTIR stages share, their checks and their parsing; `who` is the renderer in a message ("restir-di"), `o` the
// command-line option ("--restir").
struct restir_shared_options
{
    uint32_t spatial_samples = 2;
    float search_radius = 32.0f;
    float max_confidence = 16.0f;
    bool temporal_reuse = true;
    float min_ray_dist = 1e-4f;
    uint32_t rng_seed = 0;
    bool record = false;
    int projection = 0;

protected:
    // what trhip_restir_*_create refuses of these, said without a device
    void check_shared(const std::string& who) const
    {
        if(spatial_samples > 4) throw std::runtime_error(who + ": spatial_samples " + std::to_string(spatial_samples) + " is outside 0..4");
        if(!(search_radius > 0.0f) || !(search_radius <= 1024.0f)) throw std::runtime_error(who + ": search_radius must be in (0, 1024]");
        if(!(max_confidence >= 1.0f) || !std::isfinite(max_confidence)) throw std::runtime_error(who + ": max_confidence must be finite and at least 1");
        if(!(min_ray_dist > 0.0f) || !std::isfinite(min_ray_dist)) throw std::runtime_error(who + ": min_ray_dist must be finite and positive");
    }
    using fields = std::map<std::string, std::string>;
    static void whole(const char* o, const fields& v, const char* name, uint32_t& field, double lo, double hi)
    {
        const double n = struct_number(o, v, name, (double)field);
        if(!(n >= lo) || !(n <= hi) || n != std::floor(n))
            throw std::runtime_error(std::string(o) + ": " + name + " must be a whole number in " + std::to_string((int)lo) + ".." + std::to_string((int)hi));
        field = (uint32_t)n;
    }
    void parse_shared(const char* o, const fields& v)
    {
        whole(o, v, "spatial_samples", spatial_samples, 0, 4);
        search_radius = (float)struct_number(o, v, "search_radius", search_radius);
        max_confidence = (float)struct_number(o, v, "max_confidence", max_confidence);
        auto it = v.find("temporal_reuse");
        if(it != v.end())
        {
            const std::string& t = it->second;
            if(t == "on" || t == "true" || t == "1") temporal_reuse = true;
            else if(t == "off" || t == "false" || t == "0") temporal_reuse = false;
            else throw std::runtime_error(std::string(o) + ": temporal_reuse=" + t + " is neither on nor off");
        }
    }
    // the fields trhip_restir_di_options and trhip_restir_gi_options share
    template<class C> void fill_shared(C& o) const
    {
        o.spatial_samples = spatial_samples; o.search_radius = search_radius; o.max_confidence = max_confidence;
        o.temporal_reuse = temporal_reuse; o.min_ray_dist = min_ray_dist; o.rng_seed = rng_seed; o.record = record;
    }
};

class restir_di_stage
{
public:
    // Set the fields by name: the shared base's fields come first in aggregate order, `candidates` after them.
    struct options: restir_shared_options
    {
        uint32_t candidates = 4;          // --restir=candidates,spatial_samples,search_radius,max_confidence,temporal_reuse
        int visibility = TRHIP_RESTIR_VISIBILITY_PER_TARGET;      // --restir-visibility=per-target|shared|sampled (trhip_restir_di_set_visibility)
        // --restir-light-selection=uniform|power[,fraction] (trhip_restir_di_set_light_selection): how a point or triangle light candidate is
        // drawn, and the share of the power mode's pdf that stays uniform
        int light_selection = TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM;
        float uniform_fraction = 0.1f;
        // --restir-bsdf-candidates=N (trhip_restir_di_set_bsdf_candidates): candidates a pixel draws from its surface's BSDF behind the light
        // candidates, 0..8, at most 32 together
        uint32_t bsdf_candidates = 0;
        // --restir-sphere-lights=point|area (trhip_restir_di_set_sphere_lights): a point light with a radius lit as a point or as a sphere
        int sphere_lights = TRHIP_RESTIR_SPHERE_LIGHTS_POINT;
        // what trhip_restir_di_create, trhip_restir_di_set_visibility, trhip_restir_di_set_light_selection,
        // trhip_restir_di_set_bsdf_candidates and trhip_restir_di_set_sphere_lights refuse, said without a device
        void check() const
        {
            if(candidates < 1 || candidates > 32) throw std::runtime_error("restir-di: candidates " + std::to_string(candidates) + " is outside 1..32");
            if(visibility < TRHIP_RESTIR_VISIBILITY_PER_TARGET || visibility > TRHIP_RESTIR_VISIBILITY_SAMPLED)
                throw std::runtime_error("restir-di: visibility " + std::to_string(visibility) + " is outside 0..2");
            if(light_selection < TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM || light_selection > TRHIP_RESTIR_LIGHT_SELECTION_POWER)
                throw std::runtime_error("restir-di: light_selection " + std::to_string(light_selection) + " is outside 0..1");
            if(!(uniform_fraction > 0.0f) || !(uniform_fraction <= 1.0f)) throw std::runtime_error("restir-di: uniform_fraction must be in (0, 1]");
            if(bsdf_candidates > 8) throw std::runtime_error("restir-di: bsdf_candidates " + std::to_string(bsdf_candidates) + " is outside 0..8");
            if(candidates + bsdf_candidates > 32)
                throw std::runtime_error("restir-di: candidates " + std::to_string(candidates) + " + bsdf_candidates " + std::to_string(bsdf_candidates) + " is above 32");
            if(sphere_lights < TRHIP_RESTIR_SPHERE_LIGHTS_POINT || sphere_lights > TRHIP_RESTIR_SPHERE_LIGHTS_AREA)
                throw std::runtime_error("restir-di: sphere_lights " + std::to_string(sphere_lights) + " is outside 0..1");
            check_shared("restir-di");
        }
        // --restir-sphere-lights=MODE
        void parse_sphere_lights(const std::string& text)
        {
            if(text == "point") sphere_lights = TRHIP_RESTIR_SPHERE_LIGHTS_POINT;
            else if(text == "area") sphere_lights = TRHIP_RESTIR_SPHERE_LIGHTS_AREA;
            else throw std::runtime_error("--restir-sphere-lights: " + text + " is neither point nor area");
        }
        // --restir-light-selection=uniform|power[,fraction]
        void parse_light_selection(const std::string& text)
        {
            const size_t comma = text.find(',');
            const std::string name = text.substr(0, comma);
            if(name == "uniform") light_selection = TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM;
            else if(name == "power") light_selection = TRHIP_RESTIR_LIGHT_SELECTION_POWER;
            else throw std::runtime_error("--restir-light-selection: " + name + " is neither uniform nor power");
            if(comma == std::string::npos) return;
            const std::string number = text.substr(comma + 1);
            size_t end = 0;
            float f = 0.0f;
            try { f = std::stof(number, &end); } catch(std::exception&) { end = 0; }
            if(number.empty() || end != number.size() || !(f > 0.0f) || !(f <= 1.0f))
                throw std::runtime_error("--restir-light-selection: the uniform fraction " + number + " is not a number in (0, 1]");
            uniform_fraction = f;
        }
        // --restir-bsdf-candidates=N
        void parse_bsdf_candidates(const std::string& text)
        {
            size_t end = 0;
            long n = -1;
            try { n = std::stol(text, &end); } catch(std::exception&) { end = 0; }
            if(text.empty() || end != text.size() || n < 0 || n > 8)
                throw std::runtime_error("--restir-bsdf-candidates: " + text + " is not a whole number in 0..8");
            bsdf_candidates = (uint32_t)n;
        }
        // --restir-visibility=MODE
        void parse_visibility(const std::string& text)
        {
            if(text == "per-target") visibility = TRHIP_RESTIR_VISIBILITY_PER_TARGET;
            else if(text == "shared") visibility = TRHIP_RESTIR_VISIBILITY_SHARED;
            else if(text == "sampled") visibility = TRHIP_RESTIR_VISIBILITY_SAMPLED;
            else throw std::runtime_error("--restir-visibility: " + text + " is none of per-target, shared, sampled");
        }
        // --restir=...: positional or name=value; a field left out keeps its value
        void parse(const std::string& text)
        {
            const char* const o = "--restir";
            const auto v = parse_struct_option(o, text, {"candidates", "spatial_samples", "search_radius", "max_confidence", "temporal_reuse"});
            whole(o, v, "candidates", candidates, 1, 32);
            parse_shared(o, v);
            check();
        }
        trhip_restir_di_options c_options() const { trhip_restir_di_options o = {}; o.candidates = candidates; fill_shared(o); return o; }
    };
    restir_di_stage(device& dev, uvec2 size, uint32_t layers, const options& opt): dev(&dev), size(size), layers(layers), opt(opt)
    {
        opt.check();
        const trhip_restir_di_options o = opt.c_options();
        check(trhip_restir_di_create(dev.h, &o, size.x, size.y, layers, &h));
        if((opt.visibility != TRHIP_RESTIR_VISIBILITY_PER_TARGET && trhip_restir_di_set_visibility(h, opt.visibility) != 0) ||
           (opt.light_selection != TRHIP_RESTIR_LIGHT_SELECTION_UNIFORM && trhip_restir_di_set_light_selection(h, opt.light_selection, opt.uniform_fraction) != 0) ||
           (opt.bsdf_candidates != 0 && trhip_restir_di_set_bsdf_candidates(h, opt.bsdf_candidates) != 0) ||
           (opt.sphere_lights != TRHIP_RESTIR_SPHERE_LIGHTS_POINT && trhip_restir_di_set_sphere_lights(h, opt.sphere_lights) != 0))
        {
            trhip_restir_di_destroy(h);
            check(1);
        }
    }
    restir_di_stage(const restir_di_stage&) = delete;
    ~restir_di_stage() { trhip_restir_di_destroy(h); }
    // one frame of the listed viewports into `out` (RGBA32F [viewports][h][w])
    void run(const std::vector<uint32_t>& viewports, void* out, void* stream = nullptr)
    {
        check(trhip_restir_di_render(h, opt.projection, viewports.data(), (uint32_t)viewports.size(), out, stream));
    }
    void reset() { check(trhip_restir_di_reset(h)); }
    // another mode than the history's is refused until reset()
    void set_visibility(int mode) { check(trhip_restir_di_set_visibility(h, mode)); opt.visibility = mode; }
    // "power" builds the table from the scene's lights as they are and waits for the device; a change is refused while there is history
    void set_light_selection(int mode, float uniform_fraction = 0.1f)
    {
        check(trhip_restir_di_set_light_selection(h, mode, uniform_fraction));
        opt.light_selection = mode; opt.uniform_fraction = uniform_fraction;
    }
    // a change is refused while there is history
    void set_bsdf_candidates(uint32_t n) { check(trhip_restir_di_set_bsdf_candidates(h, n)); opt.bsdf_candidates = n; }
    // another mode than the history's is refused until reset()
    void set_sphere_lights(int mode) { check(trhip_restir_di_set_sphere_lights(h, mode)); opt.sphere_lights = mode; }
    // after the scene's lights or instances changed: rebuilds the power mode's table unless the lights' weights are those it holds (then false)
    bool refresh_light_selection() { uint32_t rebuilt = 0; check(trhip_restir_di_refresh_light_selection(h, &rebuilt)); return rebuilt != 0; }
    trhip_restir_di_timings get_timings() { trhip_restir_di_timings t; check(trhip_restir_di_get_timings(h, &t)); return t; }

    device* dev;
    uvec2 size;
    uint32_t layers;
    options opt;
    trhip_restir_di* h = nullptr;
};

// --renderer=restir-di: the ReSTIR DI stage renders every viewport, the frame is tonemapped - on one stream.
class restir_di_renderer: public viewport_frame_renderer
{
public:
    struct options
    {
        restir_di_stage::options restir;
        tonemap_stage::options tonemap;
    };
    restir_di_renderer(device& dev, const scene_data& scene, uvec2 size, const options& opt_)
    : viewport_frame_renderer(dev, scene, size, checked(opt_).tonemap), opt(opt_)
    {
        stage.reset(new restir_di_stage(dev, size, viewports, opt.restir));
    }
    ~restir_di_renderer() { stage.reset(); }
    // a frame of an animated scene, ahead of render(): the lights may have moved with their nodes (nothing for the uniform selection)
    void scene_moved() { stage->refresh_light_selection(); }
    void render(void* stream = nullptr)
    {
        stage->run(viewport_list, color, stream);
        finish_frame(stream);
    }

    options opt;
    std::unique_ptr<restir_di_stage> stage;

private:
    static const options& checked(const options& o) { o.restir.check(); return o; }      // the options are refused before anything is allocated
};

// ReSTIR GI (trhip_restir_gi_*; csrc/restir_gi.h pins the rule): indirect light by reservoir resampling - per frame the initial kernel
// (first hit, one cosine-hemisphere ray, a light sample at its hit and, with bounces > 1, the path continued from there), the temporal
// kernel (the history merge) and the spatial kernel (neighbour merge, shading).  `size`, `layers`: the images of a frame.  The limits are
// listed in trhip.h and DESIGN.md sections 25 and 30.
class restir_gi_stage
{
public:
    struct options: restir_shared_options     // --restir-gi=spatial_samples,search_radius,max_confidence,temporal_reuse
    {
        uint32_t bounces = 1;                 // --restir-gi-bounces=N: the vertices of a sample's path behind the pixel (trhip_restir_gi_set_bounces)
        // what trhip_restir_gi_create and trhip_restir_gi_set_bounces refuse, said without a device
        void check() const
        {
            if(bounces < 1 || bounces > 8) throw std::runtime_error("restir-gi: bounces " + std::to_string(bounces) + " is outside 1..8");
            check_shared("restir-gi");
        }
        // --restir-gi-bounces=N
        void parse_bounces(const std::string& text)
        {
            size_t end = 0;
            unsigned long n = 0;
            try { n = std::stoul(text, &end); } catch(std::exception&) { end = 0; }
            if(text.empty() || end != text.size() || text[0] == '-' || n < 1 || n > 8)
                throw std::runtime_error("--restir-gi-bounces: " + text + " is not a whole number in 1..8");
            bounces = (uint32_t)n;
        }
        // --restir-gi=...: positional or name=value; a field left out keeps its value
        void parse(const std::string& text)
        {
            const char* const o = "--restir-gi";
            parse_shared(o, parse_struct_option(o, text, {"spatial_samples", "search_radius", "max_confidence", "temporal_reuse"}));
            check();
        }
        trhip_restir_gi_options c_options() const { trhip_restir_gi_options o = {}; fill_shared(o); return o; }
    };
    restir_gi_stage(device& dev, uvec2 size, uint32_t layers, const options& opt): dev(&dev), size(size), layers(layers), opt(opt)
    {
        opt.check();
        const trhip_restir_gi_options o = opt.c_options();
        check(trhip_restir_gi_create(dev.h, &o, size.x, size.y, layers, &h));
        if(opt.bounces != 1 && trhip_restir_gi_set_bounces(h, opt.bounces) != 0)
        {
            trhip_restir_gi_destroy(h);
            check(1);
        }
    }
    restir_gi_stage(const restir_gi_stage&) = delete;
    ~restir_gi_stage() { trhip_restir_gi_destroy(h); }
    // one frame of the listed viewports: out = in + indirect light (RGBA32F [viewports][h][w]; `in` null: (0, 0, 0, 1); `out` may be `in`)
    void run(const std::vector<uint32_t>& viewports, const void* in, void* out, void* stream = nullptr)
    {
        check(trhip_restir_gi_render(h, opt.projection, viewports.data(), (uint32_t)viewports.size(), in, out, stream));
    }
    void reset() { check(trhip_restir_gi_reset(h)); }
    trhip_restir_gi_timings get_timings() { trhip_restir_gi_timings t; check(trhip_restir_gi_get_timings(h, &t)); return t; }

    device* dev;
    uvec2 size;
    uint32_t layers;
    options opt;
    trhip_restir_gi* h = nullptr;
};

// --renderer=restir-gi: the ReSTIR DI stage renders the direct light of every viewport, the ReSTIR GI stage adds indirect light to it
// (options.restir_gi.bounces: how far a sample's path goes on), the frame is tonemapped - on one stream.
class restir_gi_renderer: public viewport_frame_renderer
{
public:
    struct options
    {
        restir_di_stage::options restir;        // the direct half (--restir)
        restir_gi_stage::options restir_gi;     // the indirect half (--restir-gi)
        tonemap_stage::options tonemap;
    };
    restir_gi_renderer(device& dev, const scene_data& scene, uvec2 size, const options& opt_)
    : viewport_frame_renderer(dev, scene, size, checked(opt_).tonemap), opt(opt_)
    {
        direct.reset(new restir_di_stage(dev, size, viewports, opt.restir));
        stage.reset(new restir_gi_stage(dev, size, viewports, opt.restir_gi));
    }
    ~restir_gi_renderer() { stage.reset(); direct.reset(); }
    void scene_moved() { direct->refresh_light_selection(); }      // as restir_di_renderer
    void render(void* stream = nullptr)
    {
        direct->run(viewport_list, color, stream);
        stage->run(viewport_list, color, color, stream);
        finish_frame(stream);
    }

    options opt;
    std::unique_ptr<restir_di_stage> direct;
    std::unique_ptr<restir_gi_stage> stage;

private:
    static const options& checked(const options& o) { o.restir.check(); o.restir_gi.check(); return o; }      // refused before anything is allocated
};

class load_balancer
{
public:
    explicit load_balancer(size_t device_count, std::vector<double> initial = {}): workloads(std::move(initial))
    {
        workloads.resize(device_count);
        double sum = 0, add = 0;
        for(double w: workloads) sum += w;
        if(sum == 0) { add = 1.0; sum = (double)workloads.size(); }
        for(double& w: workloads) w = (std::max(w, 0.0) + add) / sum;
    }
    // times[i] = "path tracing" timer of device i
    const std::vector<double>& update(const std::vector<double>& times)
    {
        double sum_speed = 0;
        for(size_t i = 0; i < workloads.size(); ++i) sum_speed += std::max(workloads[i] / times[i], 0.0);   // a zero time gives inf: no update
        if(sum_speed > 0 && std::isfinite(sum_speed))
            for(size_t i = 0; i < workloads.size(); ++i)
                workloads[i] = workloads[i] * 0.9 + (workloads[i] / times[i]) / sum_speed * 0.1;
        return workloads;
    }
    std::vector<double> workloads;
};

//==============================================================================
// post_processing_renderer (src/post_processing_renderer.{hh,cc}): the one owner of the chain behind the path tracer.  make_plan is its
// policy - which stages run and in which order, which G-buffer entries the path tracer has to write for them (set_gbuffer_spec), whether a
// history binds the chain to frame order, whether the path tracer may still write the display image itself - as a pure function that needs
// no device.  The object builds the stages of a plan and the images that belong to the chain rather than to a frame slot's path tracing
// (the TAA input, the destination G-buffer, the full and the composed images), keeps the previous-camera record and runs the chain for a
// slot on a stream.  The renderer in front of it asks four things: alloc_targets per slot, chain.frame_order, chain.fused_tonemap, run.
//==============================================================================
class post_processing_renderer
{
public:
    struct options
    {
        tonemap_stage::options tonemap;
        // --denoiser=bmfr (src/post_processing_renderer.cc:53-106): the path tracer also renders the gbuffer entries the stage reads, every
        // frame is a fresh frame (the sample counter keeps counting), the stage runs between stitch and tonemap - which is then a stage of
        // its own - and gets last frame's cameras as camera_pair.previous.  One device (or view shards): the feature targets of a pixel
        // distribution over several devices would have to be gathered and stitched like colour, which is not built.
        std::optional<bmfr_stage::options> bmfr;
        // --spatial-reprojection=i,j,... : only these viewports of active_viewport_count are path traced, as compact layers in list order
        // with their own cameras and RNG streams; the others get a first-hit G-buffer pass and are filled by spatial_reprojection_stage.
        // `display` holds every viewport in natural order; with `accumulate` the sources are the accumulators and the full image is
        // rewritten every frame.  --temporal-reprojection=r (0 = off): temporal_reprojection_stage on the path-traced layers in front of it;
        // its history is one chain in frame order, like the denoiser's.  One device, no denoiser, one frame per launch.
        std::vector<uint32_t> spatial_reprojection;
        float temporal_reprojection = 0.0f;
        // --taa=N (src/post_processing_renderer.cc:62, 99-100, 202-224): taa_stage behind the tonemap stage with alpha = 1 / N and the tonemap
        // stage's gamma; the path tracer also renders screen_motion, pos and instance_id, every frame is a fresh frame and the stage gets last
        // frame's cameras - with last frame's jitter - as camera_pair.previous.  The caller gives the scene's cameras the jitter sequence
        // (set_camera_jitter) and steps it before every frame (step_camera_jitter, then update_cameras or update_scene).  One device, no
        // reprojection stages, one frame per launch; its history is one chain in frame order, like the denoiser's.
        struct taa_options { int sequence_length = 8; bool edge_dilation = true, anti_shimmer = false; };
        std::optional<taa_options> taa;
        // --display=looking-glass: looking_glass_composition_stage at the very end, behind tonemap and taa; `size` is the size of one view,
        // active_viewport_count the rig's view count (before a viewport list compacts it) and `composed` / `composed8` the panel's image.
        // The caller sets the cameras up (looking_glass_cameras of tauray_gltf.hh).  One device - the views would have to be gathered
        // first -, one frame per launch; works with the reprojection stages, the denoiser, taa and an animated scene.
        struct looking_glass_options { looking_glass_composition_stage::options stage; uvec2 output_size{0, 0}; };
        std::optional<looking_glass_options> looking_glass;
    };
    // what the policy depends on besides the chain's own options
    struct facts
    {
        size_t device_count = 1;
        size_t viewports = 1;               // active_viewport_count, before a viewport list compacts it
        bool accumulate = false;
        uint32_t frames_per_launch = 1;
        int projection = 0;
        bool path_tracer = true;            // the pipeline is path_tracer_stage
    };
    struct plan
    {
        std::vector<std::string> stages;    // in chain order, out of: bmfr, temporal, gbuffer+spatial, tonemap, taa, looking_glass
        std::vector<std::string> targets;   // the G-buffer entries the path tracer writes besides colour
        bool frame_order = false;           // a history (or the destination G-buffer the slots share) is one chain over all frame slots
        bool fused_tonemap = false;         // nothing sits between the path tracer and the tonemap stage
        size_t output_layers = 1;           // layers of `display`
        size_t traced_viewports = 1;        // the viewports the path tracer renders (the length of a viewport list) ...
        size_t traced_layers = 1;           // ... and the layers of its targets: that times the frames per launch
        bool has(const char* stage) const { return std::find(stages.begin(), stages.end(), stage) != stages.end(); }
    };

    static plan make_plan(const options& opt, const facts& f)
    {
        const std::string count = std::to_string(f.device_count);
        const uint32_t batch = f.frames_per_launch;
        if(opt.bmfr)
        {
            if(f.device_count > 1)
                throw std::runtime_error("rt_renderer: a denoiser with a pixel distribution of count " + count + " > 1 is not built: "
                                         "the feature targets (diffuse, albedo, normal, pos, instance id, screen motion) would have to be gathered and stitched like colour");
            if(f.accumulate || batch > 1) throw std::runtime_error("rt_renderer: a denoised frame is a fresh frame: no accumulation, one frame per launch");
            if(!f.path_tracer) throw std::runtime_error("rt_renderer: the denoiser reads the path tracer's diffuse target");
        }
        const bool spatial_on = !opt.spatial_reprojection.empty();
        if(!(opt.temporal_reprojection >= 0.0f) || !(opt.temporal_reprojection < 1.0f))
            throw std::runtime_error("rt_renderer: the temporal reprojection ratio must be in [0, 1) (0 = off)");
        const bool temporal_on = opt.temporal_reprojection > 0.0f;
        if(spatial_on) check_viewport_list(opt.spatial_reprojection, f.viewports, "rt_renderer: spatial reprojection");
        if(spatial_on || temporal_on)
        {
            const std::string which = spatial_on ? "spatial reprojection" : "temporal reprojection";
            if(f.device_count > 1)
                throw std::runtime_error("rt_renderer: " + which + " with a distribution of count " + count + " > 1: the stages read the "
                                         "G-buffer of whole viewports on one device, gathering it from several is not built; use one device");
            if(opt.bmfr) throw std::runtime_error("rt_renderer: " + which + " together with a denoiser: a chain of reprojection and a denoiser is not built");
            if(batch > 1) throw std::runtime_error("rt_renderer: " + which + ": a reprojected frame is one frame, frames per launch must be 1");
            if(temporal_on && f.accumulate) throw std::runtime_error("rt_renderer: temporal reprojection blends the previous frame into a fresh frame: no accumulation");
        }
        if(opt.taa)
        {
            if(opt.taa->sequence_length < 1) throw std::runtime_error("rt_renderer: taa: the length of the jitter sequence must be positive");
            if(f.device_count > 1)
                throw std::runtime_error("rt_renderer: taa with a pixel distribution of count " + count + " > 1: the stage reads screen motion, "
                                         "pos and instance id of whole viewports on one device, gathering them from several is not built; use one device");
            if(f.accumulate) throw std::runtime_error("rt_renderer: taa blends a fresh, jittered frame into its history: no accumulation");
            if(batch > 1) throw std::runtime_error("rt_renderer: taa: an antialiased frame is one frame (the jitter steps between frames), frames per launch must be 1");
            if(spatial_on || temporal_on) throw std::runtime_error("rt_renderer: taa together with spatial / temporal reprojection: a chain of reprojection and taa is not built");
            if(f.projection == 2)
                throw std::runtime_error("rt_renderer: taa with equirectangular cameras: the stage projects a miss's ray direction with the previous camera's view_proj, "
                                         "which an equirectangular camera does not have");
            if(!f.path_tracer) throw std::runtime_error("rt_renderer: taa reads the path tracer's screen_motion target");
        }
        if(opt.looking_glass)
        {
            if(f.device_count > 1)
                throw std::runtime_error("rt_renderer: a Looking Glass output with a pixel distribution of count " + count + " > 1: the composition "
                                         "stage reads every view of the light field on one device, the views would have to be gathered first, which is not built; use one device");
            if(batch > 1) throw std::runtime_error("rt_renderer: a Looking Glass output: a composed frame is one frame, frames per launch must be 1");
            if(f.projection != 0) throw std::runtime_error("rt_renderer: a Looking Glass output: the rig's cameras are perspective cameras");
            if(opt.looking_glass->stage.viewport_count != f.viewports)
                throw std::runtime_error("rt_renderer: a Looking Glass output of " + std::to_string(opt.looking_glass->stage.viewport_count) + " views over " +
                                         std::to_string(f.viewports) + " viewports");
        }
        plan p;
        if(opt.bmfr) p.stages.push_back("bmfr");
        if(temporal_on) p.stages.push_back("temporal");
        if(spatial_on) p.stages.push_back("gbuffer+spatial");
        p.stages.push_back("tonemap");
        if(opt.taa) p.stages.push_back("taa");
        if(opt.looking_glass) p.stages.push_back("looking_glass");
        if(opt.bmfr) p.targets = {"diffuse", "albedo", "normal", "pos", "screen_motion", "instance_id"};
        else if(opt.taa) p.targets = {"screen_motion", "pos", "instance_id"};
        else if(spatial_on || temporal_on) { p.targets = {"normal", "pos", "instance_id"}; if(temporal_on) p.targets.push_back("screen_motion"); }
        p.frame_order = opt.bmfr || temporal_on || spatial_on || opt.taa;
        p.fused_tonemap = f.path_tracer && f.device_count == 1 && p.stages.size() == 1;
        p.output_layers = f.viewports * batch;
        p.traced_viewports = spatial_on ? opt.spatial_reprojection.size() : f.viewports;
        p.traced_layers = p.traced_viewports * batch;
        return p;
    }

    // `dev`: the display device; `slots`: the frame slots; `cameras`: scene_data::cameras of the scene the devices hold
    post_processing_renderer(device& dev, uvec2 size, const options& opt, const plan& chain, size_t slots, int projection, float min_ray_dist,
                             const std::vector<uint8_t>& cameras)
    : dev(&dev), size(size), chain(chain), images(slots), last_cameras(cameras), current_cameras(cameras)
    {
        const size_t layer_px = size_t(size.x) * size.y, display_bytes = layer_px * 16 * chain.output_layers;
        const uint32_t layers = (uint32_t)chain.traced_layers;
        tonemap = std::make_unique<tonemap_stage>(dev, opt.tonemap);
        if(chain.has("looking_glass"))
        {
            const uvec2 os = opt.looking_glass->output_size;
            lkg = std::make_unique<looking_glass_composition_stage>(dev, size, os, opt.looking_glass->stage);
            for(slot_images& im: images) { im.composed = dev.alloc(size_t(os.x) * os.y * 16); im.composed8 = dev.alloc(size_t(os.x) * os.y * 4); }
        }
        if(chain.has("bmfr")) bmfr = std::make_unique<bmfr_stage>(dev, trhip_bmfr_features{}, size, layers, *opt.bmfr);
        if(chain.has("temporal"))
            temporal = std::make_unique<temporal_reprojection_stage>(dev, size, layers, temporal_reprojection_stage::options{opt.temporal_reprojection});
        if(chain.has("gbuffer+spatial"))
        {
            for(slot_images& im: images) { im.full = dev.alloc(display_bytes); check(trhip_memset(dev.h, im.full, 0, display_bytes, nullptr)); }
            spatial = std::make_unique<spatial_reprojection_stage>(dev, size, (uint32_t)chain.output_layers, opt.spatial_reprojection);
            gbuffer = std::make_unique<gbuffer_stage>(dev, size, projection, min_ray_dist);
            const size_t dpx = layer_px * spatial->destinations.size();
            destination_targets.normal = dev.alloc(dpx * 8); destination_targets.pos = dev.alloc(dpx * 16); destination_targets.instance_id = dev.alloc(dpx * 4);
        }
        if(chain.has("taa"))
        {
            taa_input = dev.alloc(display_bytes);
            taa_stage::options to;
            to.blending_ratio = 1.0f / (float)opt.taa->sequence_length; to.gamma = opt.tonemap.gamma;
            to.edge_dilation = opt.taa->edge_dilation; to.anti_shimmer = opt.taa->anti_shimmer; to.projection = projection;
            taa = std::make_unique<taa_stage>(dev, size, layers, to);
        }
        dev.sync();
    }
    post_processing_renderer(const post_processing_renderer&) = delete;
    ~post_processing_renderer()
    {
        bmfr.reset(); temporal.reset(); spatial.reset(); taa.reset(); lkg.reset();
        for(void* p: {taa_input, destination_targets.normal, destination_targets.pos, destination_targets.instance_id}) if(p) dev->free(p);
        for(slot_images& im: images) for(void* p: {im.full, im.composed, im.composed8}) if(p) dev->free(p);
    }

    // "allocate these targets per slot": the G-buffer entries of the plan next to a slot's colour target, and their release
    void alloc_targets(trhip_pt_targets& t) const
    {
        const size_t px = size_t(size.x) * size.y * chain.traced_layers;
        for(const std::string& name: chain.targets) t.*target(name).member = dev->alloc(px * target(name).bytes_per_pixel);
    }
    void free_targets(trhip_pt_targets& t) const
    {
        for(const std::string& name: chain.targets) { void*& p = t.*target(name).member; if(p) dev->free(p); p = nullptr; }
    }

    // The scene's cameras changed (`s.cameras`); a whole scene update may bring its own previous cameras.
    void cameras_changed(const scene_data& s, bool whole_scene)
    {
        current_cameras = s.cameras;
        if(whole_scene && !s.previous_cameras.empty()) uploaded_previous_cameras = s.previous_cameras;
    }

    // In front of a frame's path tracing: camera_pair.previous on the device = the cameras of the frame before this one.  `wait` is called
    // before the record changes (frames in flight read the cameras they were enqueued with).
    template<typename Wait>
    void begin_frame(scene_stage& scene_update, Wait&& wait)
    {
        if(!(bmfr || temporal || taa)) return;
        if(last_cameras != uploaded_previous_cameras)
        {
            wait();
            scene_update.set_previous_cameras(last_cameras.data(), (uint32_t)(last_cameras.size() / 320));
            uploaded_previous_cameras = last_cameras;
        }
        last_cameras = current_cameras;
    }

    // The chain on slot k's images (src/post_processing_renderer.cc:53-106): `t` the slot's targets with its colour, `display` its display
    // image; `run_tonemap` false: the path tracer wrote the display image itself.
    void run(size_t k, const trhip_pt_targets& t, void* display, bool run_tonemap, uint32_t frame_index, void* stream)
    {
        slot_images& im = images[k];
        if(bmfr)
        {
            bmfr->features = trhip_bmfr_features{t.color, t.diffuse, t.albedo, t.normal, t.pos, t.screen_motion, t.instance_id};
            bmfr->run(frame_index, stream);
        }
        const void* final_color = t.color;
        if(temporal) temporal->run(trhip_reprojection_images{t.color, t.normal, t.pos, t.instance_id, t.screen_motion}, stream);
        if(spatial)
        {
            gbuffer->run(spatial->destinations, destination_targets, stream);
            spatial->run(trhip_reprojection_images{t.color, t.normal, t.pos, t.instance_id, nullptr},
                         trhip_reprojection_images{nullptr, destination_targets.normal, destination_targets.pos, destination_targets.instance_id, nullptr}, im.full, stream);
            final_color = im.full;
        }
        if(run_tonemap) tonemap->run(final_color, taa ? taa_input : display, size, (uint32_t)chain.output_layers, stream);
        if(taa) taa->run(trhip_taa_images{taa_input, display, t.screen_motion, t.pos, t.instance_id}, stream);
        if(lkg) lkg->run(display, im.composed, im.composed8, stream);
    }

    struct slot_images { void* full = nullptr; void* composed = nullptr; void* composed8 = nullptr; };   // spatial reprojection: the colour of every viewport in natural order; a Looking Glass output: the panel's image
    device* dev;
    uvec2 size;
    plan chain;
    std::vector<slot_images> images;                            // one per frame slot
    std::unique_ptr<tonemap_stage> tonemap;
    std::unique_ptr<bmfr_stage> bmfr;                           // options.bmfr
    std::unique_ptr<temporal_reprojection_stage> temporal;      // options.temporal_reprojection
    std::unique_ptr<spatial_reprojection_stage> spatial;        // options.spatial_reprojection
    std::unique_ptr<gbuffer_stage> gbuffer;
    std::unique_ptr<taa_stage> taa;                             // options.taa
    std::unique_ptr<looking_glass_composition_stage> lkg;       // options.looking_glass
    void* taa_input = nullptr;                                  // the tonemap stage's output when taa runs behind it (the stage writes `display`)
    trhip_gbuffer_targets destination_targets = {};             // the G-buffer of the viewports that are reprojected, shared by the slots
    std::vector<uint8_t> last_cameras, current_cameras, uploaded_previous_cameras;   // camera_data of the last frame rendered / of the scene as it is / camera_pair.previous on the device

private:
    struct target_info { const char* name; void* trhip_pt_targets::* member; size_t bytes_per_pixel; };
    static const target_info& target(const std::string& name)
    {
        static const target_info table[] = {{"diffuse", &trhip_pt_targets::diffuse, 16}, {"albedo", &trhip_pt_targets::albedo, 16}, {"normal", &trhip_pt_targets::normal, 8},
                                            {"pos", &trhip_pt_targets::pos, 16}, {"screen_motion", &trhip_pt_targets::screen_motion, 8}, {"instance_id", &trhip_pt_targets::instance_id, 4}};
        for(const target_info& t: table) if(name == t.name) return t;
        throw std::runtime_error("post_processing_renderer: no G-buffer entry " + name);
    }
};

//==============================================================================
// rt_renderer<Pipeline> (src/rt_renderer.hh:28-77): all devices in one process, like the reference.  Pipeline is
// path_tracer_stage or direct_stage (the reference instantiates the template for those, src/rt_renderer.cc:410-412);
// `rt_renderer` and `direct_renderer` below are the two instantiations (src/rt_renderer.hh:75-77).
//
// render() never blocks the host, like the reference's (src/rt_renderer.cc:84-133, src/stage.cc:35-76): every device has
// one stream per frame slot; a device's path tracing and the peer copy of its partial frame go onto its slot stream, the
// display device's slot stream waits for those streams (trhip_stream_wait_peer = the `dependencies` the reference hands
// from stage to stage), then stitches every partial in one launch and tonemaps.  The next frame of a slot starts on a
// non-display device only after the display device has stitched the slot's previous frame (the receive buffer is free
// again) - a stream dependency as well.  Frame slots (MAX_FRAMES_IN_FLIGHT, src/context.hh:26) work with any number of
// devices.
//==============================================================================
template<typename Pipeline>
class basic_rt_renderer
{
public:
    struct options: path_tracer_stage::options, post_processing_renderer::options     // the chain's options keep their spelling: opt.bmfr, opt.taa, ...
    {
        scene_stage::options scene;         // acceleration-structure strategy and dynamic instances of every device's scene stage
        bool accumulate = false;
        // Frame slots: frame i renders, is gathered and tonemapped on the streams of slot i % N while its predecessors are
        // still running; `display` and finish_frame() refer to the frame render() was last called for, frame_slots[k] to
        // the others.
        int max_frames_in_flight = 1;
        // Frames per launch: B > 1 makes every render() call B consecutive frames (trhip_pt_set_frame_batch): every image holds
        // B * active_viewport_count layers, frame-major, and `display` B tonemapped frames.  For frames that do not accumulate.
        // Bigger launches: less of a frame is the tail of its kernels (the pipelined figure of bench.py uses two).
        int frames_per_launch = 1;
    };

    // `devices`: HIP device index per logical device (repeat an index for --fake-devices); device 0 displays.
    basic_rt_renderer(const std::vector<int>& devices, const scene_data& scene, uvec2 size, options opt)
    : size(size), opt(opt)
    {
        if(devices.empty()) throw std::runtime_error("rt_renderer needs at least one device");
        if(devices.size() == 1) this->opt.distribution.strategy = DISTRIBUTION_DUPLICATE;   // src/tauray.cc:519-521
        const int n_slots = std::max(this->opt.max_frames_in_flight, 1);
        if(n_slots > 1 && this->opt.accumulate)
            throw std::runtime_error("rt_renderer: accumulating frames depend on each other, frames in flight must be 1");
        batch = (uint32_t)std::max(this->opt.frames_per_launch, 1);
        if(batch > 1 && this->opt.accumulate)
            throw std::runtime_error("rt_renderer: accumulating frames depend on each other, frames per launch must be 1");
        post_processing_renderer::facts facts;
        facts.device_count = devices.size(); facts.viewports = this->opt.active_viewport_count; facts.accumulate = this->opt.accumulate;
        facts.frames_per_launch = batch; facts.projection = this->opt.projection; facts.path_tracer = std::is_same<Pipeline, path_tracer_stage>::value;
        const post_processing_renderer::plan chain = post_processing_renderer::make_plan(this->opt, facts);
        per_device.resize(devices.size());
        std::vector<double> ratios(devices.size(), 1.0 / devices.size());
        double cumulative = 0;
        output_layers = chain.output_layers;                         // layers of `display`
        this->opt.active_viewport_count = chain.traced_viewports;    // the path tracer's layers: all viewports, or the active ones of a viewport list, compact
        const size_t layers = chain.traced_layers;
        display_bytes = size_t(size.x) * size.y * 16 * output_layers;
        for(size_t i = 0; i < devices.size(); ++i)
        {
            per_device_data& d = per_device[i];
            d.dev = std::make_unique<device>(devices[i]);
            d.scene_update = std::make_unique<scene_stage>(*d.dev, this->opt.scene);
            d.scene_update->set_scene(scene);               // scene replicated on every device (src/gpu_buffer.hh:63-116)
            d.dist = get_device_distribution_params(size, this->opt.distribution.strategy, cumulative, ratios[i], (unsigned)i,
                                                    (unsigned)devices.size(), i == 0);
            cumulative += ratios[i];
            // non-primary targets are allocated for the largest share set_device_workloads can hand the device
            // (get_distribution_target_max_size, src/rt_renderer.cc init_resources)
            const uvec2 ms = get_distribution_target_max_size(d.dist);
            d.max_bytes = size_t(ms.x) * ms.y * 16 * layers;
            d.slots.resize((size_t)n_slots);
            for(slot_data& sl: d.slots)
            {
                sl.stream = d.dev->create_stream();
                sl.color = d.dev->alloc(d.max_bytes);
                check(trhip_memset(d.dev->h, sl.color, 0, d.max_bytes, nullptr));
                path_tracer_stage::options po = this->opt;
                po.distribution = d.dist;
                sl.ray_tracer = std::make_unique<Pipeline>(*d.dev, *d.scene_update, sl.color, po);
                if(n_slots > 1) { sl.ray_tracer->set_frame_slots(n_slots); }   // the frames in flight fill the chip between them
                if(batch > 1) sl.ray_tracer->set_frame_batch(batch);
                if(!this->opt.spatial_reprojection.empty())
                {   // the list as arithmetic runs, one stage per run (usually one): layer l shows viewport list[l], its camera and its RNG stream
                    uint32_t first = 0;
                    for(const viewport_run& r: viewport_runs(this->opt.spatial_reprojection))
                    {
                        Pipeline* stage = sl.ray_tracer.get();
                        if(!sl.runs.empty())
                        {
                            sl.extra_tracers.push_back(std::make_unique<Pipeline>(*d.dev, *d.scene_update, sl.color, po));
                            stage = sl.extra_tracers.back().get();
                            if(n_slots > 1) stage->set_frame_slots(n_slots);
                        }
                        stage->set_shard(r.base, r.stride);
                        sl.runs.push_back({stage, first, r.count});
                        first += r.count;
                    }
                }
                if(i != 0) sl.gbuffer_copy = per_device[0].dev->alloc(d.max_bytes);   // receive buffer on the display device
            }
            d.dev->sync();
        }
        frame_slots.resize((size_t)n_slots);
        for(frame_slot& fs: frame_slots) fs.display = per_device[0].dev->alloc(display_bytes);
        display = frame_slots[0].display;
        post = std::make_unique<post_processing_renderer>(*per_device[0].dev, size, this->opt, chain, frame_slots.size(), this->opt.projection, this->opt.min_ray_dist, scene.cameras);
        tonemap = post->tonemap.get();
        composed = post->images[0].composed; composed8 = post->images[0].composed8;
        for(slot_data& sl: per_device[0].slots) { sl.targets.color = sl.color; post->alloc_targets(sl.targets); }
        // One device: nothing sits between the path tracer and the tonemap stage (no transfer, no stitch), and the stage writes the slot's
        // display image while it writes its colour target - the same bits without a second pass over the frame.  TRHIP_FUSED_TONEMAP=0: off.
        const char* fe = getenv("TRHIP_FUSED_TONEMAP");
        fused_tonemap = chain.fused_tonemap && !(fe && atoi(fe) == 0);
        fused_info.assign(frame_slots.size(), trhip_tonemap_info{-1, 0.0f, 0.0f, 0});     // what each slot's stage was last told: render() keeps it current
    }

    ~basic_rt_renderer()
    {
        finish_all();
        for(slot_data& sl: per_device[0].slots) post->free_targets(sl.targets);
        post.reset();
        for(size_t i = 0; i < per_device.size(); ++i)
            for(slot_data& sl: per_device[i].slots)
            {
                sl.ray_tracer.reset();
                sl.extra_tracers.clear();
                if(sl.gbuffer_copy) per_device[0].dev->free(sl.gbuffer_copy);
                per_device[i].dev->free(sl.color);
                per_device[i].dev->destroy_stream(sl.stream);
            }
        for(frame_slot& fs: frame_slots) per_device[0].dev->free(fs.display);
    }

    void reset_accumulation(bool reset_sample_counter = false)
    {
        for(auto& d: per_device)
            for(slot_data& sl: d.slots)
            {
                sl.ray_tracer->reset_accumulated_samples();
                if(reset_sample_counter) sl.ray_tracer->reset_sample_counter();
                for(auto& t: sl.extra_tracers) { t->reset_accumulated_samples(); if(reset_sample_counter) t->reset_sample_counter(); }
            }
        if(reset_sample_counter) frame_index = 0;
        accumulated_frames = 0;
    }

    // waits for the frame of the last render() call (all of it: path tracing, gather, stitch and tonemap end on the
    // display device's slot stream)
    void finish_frame() { if(current_slot >= 0) finish_slot(current_slot); }
    void finish_slot(int k) { per_device[0].dev->sync(per_device[0].slots[(size_t)k].stream); }
    void finish_all()
    {
        for(auto& d: per_device) { for(slot_data& sl: d.slots) d.dev->sync(sl.stream); d.dev->sync(); }
    }

    // The scene changed (an animation step): every device's copy follows (the scene is replicated, src/gpu_buffer.hh:63-116).
    // Frames in flight read the old scene: they are finished first.
    void update_scene(const scene_data& s, bool rebuild = false)
    {
        finish_all();
        for(auto& d: per_device) d.scene_update->apply(s, rebuild);
        post->cameras_changed(s, true);
    }

    // Only the cameras changed (the jitter of a still scene stepped): scene_data::cameras go to every device.
    void update_cameras(const scene_data& s)
    {
        finish_all();
        for(auto& d: per_device) d.scene_update->update_cameras(s.cameras.data(), (uint32_t)(s.cameras.size() / 320));
        post->cameras_changed(s, false);
    }

    // rt_renderer::render (src/rt_renderer.cc:84-133): ray tracers -> transfers -> stitch -> tonemap.  Enqueues only.
    void render()
    {
        const size_t k = (frame_index / batch) % frame_slots.size();
        current_slot = (int)k;
        const uint32_t layers = (uint32_t)opt.active_viewport_count * batch;
        device& display_device = *per_device[0].dev;
        void* const display_stream = per_device[0].slots[k].stream;
        if(fused_tonemap)
        {   // the stage's copy of the tonemap parameters follows tonemap->opt: an edit between frames takes effect on the next frame,
            // as it does when the tonemap stage itself runs (several devices)
            const trhip_tonemap_info ti = tonemap->info();
            if(std::memcmp(&ti, &fused_info[k], sizeof(ti)) != 0)
            {
                per_device[0].slots[k].ray_tracer->set_fused_tonemap(frame_slots[k].display, &ti);
                fused_info[k] = ti;
            }
        }
        for(size_t i = 0; i < per_device.size(); ++i)
        {
            per_device_data& d = per_device[i];
            slot_data& sl = d.slots[k];
            if(!opt.accumulate) sl.ray_tracer->reset_accumulated_samples();
            if(frame_slots.size() > 1 || batch > 1) sl.ray_tracer->set_frame_counter(frame_index);   // one stage per slot: slot k renders frames k, k + N, ... (B at a time)
            for(auto& t: sl.extra_tracers)
            {
                if(!opt.accumulate) t->reset_accumulated_samples();
                if(frame_slots.size() > 1) t->set_frame_counter(frame_index);
            }
            if(i != 0)   // the slot's previous frame has been stitched on the display device: its receive buffer is free
                check(trhip_stream_wait_peer(d.dev->h, sl.stream, display_device.h, display_stream));
            post->begin_frame(*d.scene_update, [&] { if(frame_slots.size() > 1) finish_all(); });
            const uvec2 ts = get_distribution_target_size(d.dist);
            if(!sl.runs.empty())
            {   // a viewport list: every run of it into its layers of the compact targets
                const size_t layer_px = size_t(ts.x) * ts.y;
                for(const run_data& r: sl.runs)
                {
                    trhip_pt_targets t = sl.targets;
                    auto at = [&](void* p, size_t bytes_per_pixel) { return p ? static_cast<void*>(static_cast<char*>(p) + r.first * layer_px * bytes_per_pixel) : nullptr; };
                    t.color = at(t.color, 16); t.pos = at(t.pos, 16); t.normal = at(t.normal, 8); t.instance_id = at(t.instance_id, 4); t.screen_motion = at(t.screen_motion, 8);
                    check(trhip_pt_render_targets(r.stage->pt, &t, ts.x, ts.y, r.count, sl.stream));
                }
            }
            else if(!post->chain.targets.empty()) check(trhip_pt_render_targets(sl.ray_tracer->pt, &sl.targets, ts.x, ts.y, layers, sl.stream));
            else sl.ray_tracer->run(sl.stream);
            if(i != 0) check(trhip_copy_peer(display_device.h, sl.gbuffer_copy, d.dev->h, sl.color, d.target_bytes(layers), sl.stream));
        }
        if(per_device.size() > 1)
        {
            std::vector<trhip_distribution> dists;
            std::vector<const void*> partials;
            std::vector<uint32_t> ws, hs;
            for(size_t i = 1; i < per_device.size(); ++i)
            {
                per_device_data& d = per_device[i];
                check(trhip_stream_wait_peer(display_device.h, display_stream, d.dev->h, d.slots[k].stream));
                const uvec2 ts = get_distribution_target_size(d.dist);
                dists.push_back(to_abi(d.dist)); partials.push_back(d.slots[k].gbuffer_copy); ws.push_back(ts.x); hs.push_back(ts.y);
            }
            check(trhip_stitch_batch(display_device.h, (uint32_t)dists.size(), dists.data(), partials.data(), ws.data(), hs.data(),
                                     per_device[0].slots[k].color, layers, stitch_blend_ratio, display_stream));
            stitch_blend_ratio = 1.0f;      // src/rt_renderer.cc:122
        }
        display = frame_slots[k].display;
        void* post_stream = display_stream;
        if(post->chain.frame_order && frame_slots.size() > 1)
        {   // a history is one chain over the frames of all slots: the chain runs in frame order on the display device's default stream
            check(trhip_stream_wait(display_device.h, nullptr, display_stream)); post_stream = nullptr;
        }
        post->run(k, per_device[0].slots[k].targets, display, !fused_tonemap, frame_index, post_stream);
        composed = post->images[k].composed; composed8 = post->images[k].composed8;
        if(post_stream != display_stream) check(trhip_stream_wait(display_device.h, display_stream, nullptr));
        frame_index += batch;
        accumulated_frames++;
    }

    // rt_renderer::set_device_workloads (src/rt_renderer.cc:135-183): only shuffled strips can be re-balanced
    void set_device_workloads(const std::vector<double>& ratios)
    {
        if(opt.distribution.strategy != DISTRIBUTION_SHUFFLED_STRIPS) return;
        finish_all();
        double cumulative = 0;
        for(size_t i = 0; i < per_device.size(); ++i)
        {
            double ratio = std::min(std::max(ratios[i], 0.0), 1.0 - cumulative);
            per_device[i].dist = get_device_distribution_params(size, opt.distribution.strategy, cumulative, ratio, (unsigned)i,
                                                                (unsigned)per_device.size(), i == 0);
            cumulative += ratio;
            for(slot_data& sl: per_device[i].slots)
            {
                sl.ray_tracer->reset_distribution_params(per_device[i].dist);
                if(i != 0) sl.ray_tracer->reset_accumulated_samples();
            }
        }
        // the non-primary devices start over with one sample: blend their pixels into what the display device has
        // accumulated instead of replacing it (src/rt_renderer.cc:176-181)
        if(opt.accumulate && per_device.size() > 1) stitch_blend_ratio = 1.0f / float(accumulated_frames + 1);
    }

    // "path tracing" timers of the most recent frame, one per device (waits for them)
    std::vector<double> get_path_tracing_times()
    {
        std::vector<double> t;
        const size_t k = current_slot < 0 ? 0 : (size_t)current_slot;
        for(auto& d: per_device) t.push_back(d.slots[k].ray_tracer->get_duration_ms());
        return t;
    }

    struct slot_data
    {
        void* stream = nullptr;
        std::unique_ptr<Pipeline> ray_tracer;
        void* color = nullptr;          // the device's (partial) colour target of this slot
        void* gbuffer_copy = nullptr;   // non-primary devices: where the partial lands on the display device
        trhip_pt_targets targets = {};  // denoiser / reprojection: the gbuffer entries next to `color`
        struct run { Pipeline* stage; uint32_t first, count; };
        std::vector<run> runs;          // a viewport list: one stage per arithmetic run of it (ray_tracer is the first), its first layer and layer count
        std::vector<std::unique_ptr<Pipeline>> extra_tracers;   // ... the stages of the runs after the first
    };
    using run_data = typename slot_data::run;
    struct per_device_data
    {
        std::unique_ptr<device> dev;
        std::unique_ptr<scene_stage> scene_update;
        distribution_params dist;
        size_t max_bytes = 0;
        std::vector<slot_data> slots;
        size_t target_bytes(size_t layers) const { const uvec2 ts = get_distribution_target_size(dist); return size_t(ts.x) * ts.y * 16 * layers; }
    };
    std::vector<per_device_data> per_device;
    struct frame_slot { void* display = nullptr; };   // tonemapped RGBA32F on the display device
    std::vector<frame_slot> frame_slots;   // options.max_frames_in_flight of them (at least one)
    int current_slot = -1;
    uint32_t batch = 1;                    // options.frames_per_launch
    uint32_t frame_index = 0;
    uvec2 size;
    options opt;
    void* display = nullptr;          // frame_slots[current_slot].display
    size_t display_bytes = 0;
    std::unique_ptr<post_processing_renderer> post;             // the chain behind the path tracer, on the display device
    tonemap_stage* tonemap = nullptr;                           // post->tonemap
    void* composed = nullptr;                                   // a Looking Glass output, the current slot's: RGBA32F [output_size.y][output_size.x]
    void* composed8 = nullptr;                                  // ... and the same frame as uint8 [..][..][4]
    size_t output_layers = 1;                                   // layers of `display` (every viewport; the path tracer renders opt.active_viewport_count)
    bool fused_tonemap = false;
    std::vector<trhip_tonemap_info> fused_info;
    unsigned accumulated_frames = 0;
    float stitch_blend_ratio = 1.0f;
};
using rt_renderer = basic_rt_renderer<path_tracer_stage>;       // path_tracer_renderer
using direct_renderer = basic_rt_renderer<direct_stage>;        // direct_renderer

//==============================================================================
// headless (src/headless.{hh,cc}): readback + writers.  EXR: scanline file, channels B,G,R[,A] like the reference's,
// half or float, every codec of src/headless.hh:25-32 (include/tauray_exr.hh); PIZ is the default as in the reference
// (src/headless.hh:56).
//==============================================================================
class headless
{
public:
    enum image_file_type { EXR = 0, RAW, EMPTY };
    enum pixel_format { RGB16, RGB32, RGBA16, RGBA32 };
    enum compression_type { NONE = 0, RLE = 1, ZIPS = 2, ZIP = 3, PIZ = 4 };   // values = OpenEXR compression codes (src/headless.hh:25-32)

    struct options
    {
        uvec2 size;
        std::string output_prefix = "capture";
        image_file_type output_file_type = EXR;
        pixel_format output_format = RGB16;
        compression_type output_compression = PIZ;      // src/headless.hh:56
        bool single_frame = false;
        bool skip_nan_check = false;
        unsigned first_frame_index = 0;
        unsigned display_count = 1;
        // a view shard (one process per GPU, viewport v on rank v mod N): local layer l is display display_index_base + l *
        // display_index_stride of display_count_total (0 = display_count) - what the file names are made of
        unsigned display_index_base = 0, display_index_stride = 1, display_count_total = 0;
    };

    explicit headless(const options& opt): opt(opt) {}

    static uint16_t float_to_half(float f) { return exr::float_to_half(f); }

    std::string get_filename(unsigned display_index, unsigned frame_number) const
    {
        std::string filename = opt.output_prefix;                                       // src/headless.cc:305-309
        if((opt.display_count_total ? opt.display_count_total : opt.display_count) > 1)
            filename += std::to_string(opt.display_index_base + display_index * opt.display_index_stride) + "_";
        if(!opt.single_frame) filename += std::to_string(frame_number);
        return filename + (opt.output_file_type == EXR ? ".exr" : ".raw");
    }

    // finish_image + save_image for every display layer; returns the number of NaN pixels reported
    size_t save(device& dev, const void* display_image, unsigned frame_number)
    {
        const size_t pixels = size_t(opt.size.x) * opt.size.y;
        if(opt.output_file_type == EMPTY && opt.skip_nan_check) return 0;      // nothing to look at, nothing to write: no readback
        std::vector<float> mem(pixels * 4 * opt.display_count);
        check(trhip_download(dev.h, mem.data(), display_image, mem.size() * 4, nullptr));
        size_t nan_pixels = 0;
        for(unsigned d = 0; d < opt.display_count; ++d)
        {
            const float* img = mem.data() + pixels * 4 * d;
            if(!opt.skip_nan_check)
                for(size_t j = 0; j < pixels; ++j)
                    if(std::isnan(img[4 * j]) || std::isnan(img[4 * j + 1]) || std::isnan(img[4 * j + 2]) || std::isnan(img[4 * j + 3]))
                    {
                        std::fprintf(stderr, "NaN pixel at: %zu, %zu\n", j % opt.size.x, j / opt.size.x);
                        nan_pixels++;
                    }
            if(opt.output_file_type == EMPTY) continue;
            const std::string filename = get_filename(d, frame_number);
            if(opt.output_file_type == RAW) write_raw(filename, img, pixels);
            else write_exr(filename, img);
        }
        return nan_pixels;
    }

    // writes one display layer (RGBA32F, `img`) as save() would, without a device: for tools and tests
    void write_image(const std::string& filename, const float* img) const
    {
        if(opt.output_file_type == RAW) write_raw(filename, img, size_t(opt.size.x) * opt.size.y);
        else if(opt.output_file_type == EXR) write_exr(filename, img);
    }

    options opt;

private:
    void write_raw(const std::string& filename, const float* img, size_t pixels) const
    {
        std::ofstream f(filename, std::ios::binary);
        if(!f) throw std::runtime_error("Failed to write " + filename);
        f.write(reinterpret_cast<const char*>(img), (std::streamsize)(pixels * 16));
    }

    void write_exr(const std::string& filename, const float* img) const
    {
        const bool alpha = opt.output_format == RGBA16 || opt.output_format == RGBA32;
        const bool half = opt.output_format == RGB16 || opt.output_format == RGBA16;
        const std::vector<uint8_t> out = exr::encode(img, opt.size.x, opt.size.y, alpha, half, (int)opt.output_compression);
        std::ofstream f(filename, std::ios::binary);
        if(!f) throw std::runtime_error("Failed to write " + filename);
        f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size());
    }
};

}

#endif
