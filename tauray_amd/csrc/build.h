// Host-side device scene container shared by the API and the BVH builder.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "shading.h"
#include "morph.h"

namespace tr {

int set_error(const std::string& msg);   // records trhip_last_error(); returns 1

struct DeviceScene {
    // uploaded by trhip_scene_upload
    Instance* instances = nullptr;
    MeshSpan* spans = nullptr;
    Vertex* vertices = nullptr;
    uint* indices = nullptr;
    PointLight* point_lights = nullptr;
    DirectionalLight* directional_lights = nullptr;
    TextureInfo* tex_infos = nullptr;
    uint8_t* texels = nullptr;
    f4* envmap = nullptr;
    AliasEntry* alias_table = nullptr;
    CameraData* cameras = nullptr;
    CameraData* prev_cameras = nullptr;  // defaults to a copy of `cameras`
    uint8_t* non_opaque = nullptr;
    uint* alpha_base = nullptr;          // per instance: first AlphaTri record of its triangles (non-opaque instances; 0xFFFFFFFF otherwise)
    AlphaTri* alpha_tris = nullptr;      // filled by the build and the refit (k_pretransform / k_retransform)
    uint alpha_count = 0;
    uint* tri_prefix = nullptr;          // instance_count + 1 prefix sums of triangle counts
    ShadeTri* shade_tris = nullptr;      // index_count / 3 records, or null (see common.h ShadeTri)
    f4* shade_tangents = nullptr;        // ... and their tangents, three per record, behind the records in the same allocation
    // scene_stage's pre-transformed vertex copy (shader/pre_transform.comp): one span per instance; vertices built on first use
    std::vector<MeshSpan> host_spans, host_world_spans;
    MeshSpan* world_spans = nullptr;
    Vertex* world_vertices = nullptr;
    uint world_vertex_count = 0;
    f4 environment_factor = {0, 0, 0, 0};
    int environment_proj = -1;
    uint instance_count = 0, point_light_count = 0, directional_light_count = 0, camera_count = 0, texture_count = 0;
    uint env_w = 0, env_h = 0, tri_count = 0, vertex_count = 0, index_count = 0;
    uint gather_emissive_triangles = 0, host_tri_light_count = 0;
    uint wide_textures = 0;              // some texture is RGBA16 (texture.h takes the one-dword path otherwise)
    // built by trhip_scene_build_accel
    BvhNode* nodes = nullptr;
    Bvh4Node* nodes4 = nullptr;
    TriRecord* tris = nullptr;
    TriLight* tri_lights = nullptr;
    uint node_count = 0, tri_light_count = 0;
    int builder = 1;                     // 0 = Karras LBVH, 1 = PLOC over the Morton order (TRHIP_BUILDER=lbvh|ploc)
    uint build_rounds = 0;
    int ploc_radius = 16;                // neighbour search radius of the PLOC rounds (TRHIP_PLOC_RADIUS)
    int optimise_rounds = 8;             // reinsertion rounds after the build (bvh_optimize.h; TRHIP_BVH_OPT)
    uint leaf_count = 0;                 // leaves of the tree = records in `tris`
    uint accel_tri_count = 0;            // triangle count of the scene the structure was built for
    bool collapse_by_cost = true;        // 4-wide nodes chosen by least area sum (k_collapse_cost) instead of greedily (TRHIP_COLLAPSE=greedy)
    bool fast_build = false;             // trhip_scene_set_build_mode: no optimisation rounds
    int optimise_modulus = 1;            // a node searches every optimise_modulus-th round (TRHIP_BVH_OPT_MOD)
    int dfs_layout = 1;                  // depth-first node order (TRHIP_NODE_LAYOUT=dfs|build)
    bool accel_built = false;
    uint accel_capacity = 0xFFFFFFFFu;   // leaf count the output buffers were allocated for
    void* scratch = nullptr;             // build temporaries, kept between builds
    float bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};   // centroid bounds of the last build
    // refit support (built on the first trhip_scene_refit_accel after a build): live 4-wide nodes in breadth-first order
    uint* level_nodes = nullptr;
    float* node_bounds = nullptr;        // 6 floats per node: union of its child boxes
    std::vector<uint> level_offsets;     // level l = level_nodes[level_offsets[l] .. level_offsets[l + 1])
    bool levels_valid = false;
    size_t scratch_bytes = 0;
    // ---- two-level structure (trhip_scene_set_accel_strategy)
    int accel_strategy = TRHIP_AS_ALL_MERGED;   // kept over uploads; takes effect at the next build
    std::vector<uint8_t> dynamic_marks;         // trhip_scene_set_dynamic_instances (cleared by an upload)
    std::vector<Instance> host_instances;       // what the device holds: the TLAS transforms, and which static record changed
    struct Blas {
        int root;                  // >= 0 node, < 0 ~record, in the shared arrays
        uint node_off, node_slots, tri_off, tri_count;
        uint rep;                  // an instance of the BLAS's span (object-space BLAS), whose records it rebuilds from
        bool world;                // the merged BLAS of the static instances: world-space records with their own words
    };
    std::vector<Blas> blases;
    std::vector<int> inst_blas;     // per instance: its BLAS, or -1 (no triangles)
    std::vector<uint> tlas_src;     // instance of each TLAS leaf before the TLAS sort; 0xFFFFFFFF = the merged static BLAS
    std::vector<uint8_t> blas_dirty;   // vertices changed since the BLAS was built (trhip_scene_skin)
    bool static_dirty = false;      // a static instance's record changed (trhip_scene_update_instances)
    std::vector<uint8_t> alpha_dirty;   // per instance: its AlphaTri records are stale (material changed, mesh skinned)
    uint* alpha_list = nullptr;     // device copy of the refit's list of such instances (+ prefix sums of their triangle counts)
    size_t alpha_list_words = 0;
    bool two_level = false;         // the last build was two-level
    TlasLeaf* tlas = nullptr;       // instance records in TLAS leaf order: inside the nodes4 allocation, behind the node slots
    TlasLeaf* tlas_src_leaves = nullptr;   // ... in tlas_src order (build input)
    uint tlas_leaf_count = 0, tlas_node_slots = 0, tlas_capacity = 0;
    size_t node_capacity = 0, tri_capacity = 0;   // node slots / records the two-level outputs hold
    trhip_accel_layout layout = {};
    std::vector<uint> host_alpha_base;
    std::vector<uint8_t> host_non_opaque;
    void* tl_aux = nullptr;         // TLAS build: BLAS root references and boxes, sorted instance boxes
    size_t tl_aux_bytes = 0;
    // ---- sphere-light tree (trhip_scene_set_light_accel): header and nodes behind the records in `point_lights`
    int light_accel_requested = -1;             // TRHIP_LIGHT_ACCEL_*, -1 = not set (TRHIP_LIGHT_ACCEL, else AUTO); kept over uploads
    int light_in_effect = TRHIP_LIGHT_ACCEL_LOOP;
    std::vector<PointLight> host_point_lights;  // what the device holds
    std::vector<uint> light_tree_set;           // the lights the tree was built over (radius != 0), ascending
    std::vector<Bvh4Node> light_nodes;          // host copy of the tree's nodes (the refit rewrites their boxes)
    uint light_tree_nodes = 0;
    float light_ms = 0.0f;
    int light_last_refit = -1;
    uint sphere_light_count() const { uint c = 0; for (const PointLight& pl : host_point_lights) c += pl.radius != 0.0f ? 1u : 0u; return c; }
    // ---- emitter set of the terminal query (common.h EmitterSet): behind the records in `tris`, all-merged structure only
    uint emitter_count = 0xFFFFFFFFu;           // emitter triangles of the last build or refit; 0xFFFFFFFF = no set
    // ---- motion of deforming meshes (trhip_scene_set_deformation_motion)
    bool deformation_motion = false;            // kept over uploads
    float* prev_positions = nullptr;            // float[vertex_count][3] parallel to `vertices`: the positions at the last latch; null = off
    MeshSpan* latch_spans = nullptr;            // device list for k_latch_positions: the whole vertex array (the fill), then the deforming spans
    uint latch_span_count = 0;                  // ... of the latter, each vertex range once
    uint latch_span_most = 0;                   // ... and the vertex count of the longest
    bool latch_spans_valid = false;             // false after trhip_scene_set_skin / trhip_scene_set_morph_targets

    SceneView view() const {
        SceneView v;
        v.instances = instances; v.spans = spans; v.vertices = vertices; v.indices = indices;
        v.point_lights = point_lights; v.directional_lights = directional_lights; v.tri_lights = tri_lights;
        v.tex_infos = tex_infos; v.texels = texels; v.envmap = envmap; v.alias_table = alias_table;
        v.cameras = cameras; v.prev_cameras = prev_cameras ? prev_cameras : cameras; v.obj_spans = spans; v.obj_vertices = vertices; v.shade_tris = shade_tris; v.shade_tangents = shade_tangents; v.tris = tris; v.alpha_tris = alpha_tris; v.nodes4 = nodes4;
        v.environment_factor = environment_factor; v.environment_proj = environment_proj;
        v.instance_count = instance_count; v.point_light_count = point_light_count;
        v.directional_light_count = directional_light_count; v.tri_light_count = tri_light_count;
        v.env_w = env_w; v.env_h = env_h; v.wide_textures = wide_textures; v.tri_count = accel_built ? tri_count : 0; v.node_count = node_count;
        v.prev_positions = prev_positions;
        return v;
    }
    void free_accel() {
        if (nodes) (void)hipFree(nodes);
        if (nodes4) (void)hipFree(nodes4);
        if (tris) (void)hipFree(tris);
        if (tri_lights) (void)hipFree(tri_lights);
        if (tlas_src_leaves) (void)hipFree(tlas_src_leaves);
        if (tl_aux) (void)hipFree(tl_aux);
        tl_aux = nullptr; tl_aux_bytes = 0;
        if (alpha_list) (void)hipFree(alpha_list);
        alpha_list = nullptr; alpha_list_words = 0; alpha_dirty.clear();
        tlas = nullptr; tlas_src_leaves = nullptr; tlas_capacity = 0; node_capacity = 0; tri_capacity = 0; two_level = false;
        blases.clear(); inst_blas.clear(); tlas_src.clear(); blas_dirty.clear(); static_dirty = false;
        nodes = nullptr; nodes4 = nullptr; tris = nullptr; tri_lights = nullptr; node_count = 0; tri_light_count = 0; accel_built = false;
        emitter_count = 0xFFFFFFFFu;
        accel_capacity = 0xFFFFFFFFu;
        if (level_nodes) (void)hipFree(level_nodes);
        if (node_bounds) (void)hipFree(node_bounds);
        level_nodes = nullptr; node_bounds = nullptr; level_offsets.clear(); levels_valid = false;
    }
    // skinned meshes (mesh(mesh* animation_source), src/mesh.hh:47): bind-pose vertices + skin records per instance
    struct SkinSlot { Vertex* source = nullptr; Skin* skins = nullptr; m4* joints = nullptr; uint joint_capacity = 0; uint vertex_count = 0; };
    std::vector<SkinSlot> skin_slots;
    void free_skins() {
        for (SkinSlot& k : skin_slots) { if (k.source) (void)hipFree(k.source); if (k.skins) (void)hipFree(k.skins); if (k.joints) (void)hipFree(k.joints); }
        skin_slots.clear();
    }
    // morph targets (morph.h): per instance a copy of the base vertices, the target-major delta planes (normals / tangents may be absent)
    // and the active (index, weight) list of the last trhip_scene_morph
    struct MorphSlot { Vertex* base = nullptr; float* dpos = nullptr; float* dnrm = nullptr; float* dtan = nullptr; MorphActive* active = nullptr;
                       uint active_capacity = 0; uint target_count = 0; uint vertex_count = 0; };
    std::vector<MorphSlot> morph_slots;
    static void free_morph(MorphSlot& m) {
        for (void* p : {(void*)m.base, (void*)m.dpos, (void*)m.dnrm, (void*)m.dtan, (void*)m.active}) if (p) (void)hipFree(p);
        m = MorphSlot();
    }
    void free_morphs() {
        for (MorphSlot& m : morph_slots) free_morph(m);
        morph_slots.clear();
    }
    bool has_morph(uint instance) const { return instance < morph_slots.size() && morph_slots[instance].base; }
    void free_previous_positions() {
        if (prev_positions) (void)hipFree(prev_positions);
        if (latch_spans) (void)hipFree(latch_spans);
        prev_positions = nullptr; latch_spans = nullptr; latch_span_count = 0; latch_span_most = 0; latch_spans_valid = false;
    }
    void free_all() {
        free_accel();
        free_skins();
        free_morphs();
        free_previous_positions();
        void* ptrs[] = {instances, spans, vertices, indices, point_lights, directional_lights, tex_infos, texels, envmap,
                        alias_table, cameras, prev_cameras, non_opaque, tri_prefix, world_spans, world_vertices, scratch, shade_tris, alpha_base, alpha_tris};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        const int strategy = accel_strategy, light_mode = light_accel_requested;
        const bool motion = deformation_motion;
        *this = DeviceScene();
        accel_strategy = strategy;
        deformation_motion = motion;
        light_accel_requested = light_mode;
    }
};

int build_accel(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info);
int ensure_world_vertices(DeviceScene& ds, hipStream_t stream);
int build_shade_tris(DeviceScene& ds, int instance, hipStream_t stream);   // instance < 0: every mesh (after an upload); else the mesh of that instance (after skinning)
int skin_instance(DeviceScene& ds, uint instance, const float* joint_transforms, uint joint_count, hipStream_t stream);   // skinning.comp
int refit_accel(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info);   // same tree, new boxes (after trhip_scene_update_instances)   // pre_transform.comp per instance
void mark_skinned(DeviceScene& ds, uint instance);
int morph_instance(DeviceScene& ds, uint instance, const float* weights, uint weight_count, hipStream_t stream);   // k_morph (morph.h)
// The previous-position plane: allocated and filled from every vertex of the scene (after an upload, or when the switch goes on), and
// the latch of the spans that have a skin or morph targets (k_latch_positions).  Both synchronous.
int fill_previous_positions(DeviceScene& ds, hipStream_t stream);
int latch_positions(DeviceScene& ds, hipStream_t stream);
// The sphere-light tree after an upload or trhip_scene_update_lights (`moved`: the records changed) or trhip_scene_set_light_accel: chooses
// the mode in effect, then builds, refits or drops the tree so that the device matches ds.host_point_lights.  Synchronous.
int update_light_accel(DeviceScene& ds, bool moved);
uint light_accel_auto_threshold();
int light_accel_requested(const DeviceScene& ds);   // the mode set, else TRHIP_LIGHT_ACCEL, else TRHIP_LIGHT_ACCEL_AUTO   // the BLAS of the instance's span needs a refit (two-level structure)

}  // namespace tr
