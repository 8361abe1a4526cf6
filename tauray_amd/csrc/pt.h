// Host-side path_tracer_stage object behind trhip_pt (mirrors the state kept by rt_stage /
// rt_camera_stage / path_tracer_stage: options, distribution params, frame and sample counters).
#pragma once
#include "build.h"
#include "sh_probes.h"

namespace tr {

void get_ray_count(const trhip_distribution& d, uint& w, uint& h);

// get_nee_sampling_probabilities (shader/rt.glsl:302-335): scene constants, evaluated once in fp32 on the host.  A class whose weight is
// not positive or that the scene does not have gets 0.  The path tracer, the direct stage and ReSTIR DI (restir_di.hip) share it.
inline void nee_probabilities(const DeviceScene& scene, float w_point, float w_tri, float w_dir, float w_env, float& prob_point, float& prob_tri,
                              float& prob_dir, float& prob_env) {
    float point = (w_point > 0 && scene.point_light_count > 0) ? w_point : 0.0f;
    float tri = (w_tri > 0 && scene.tri_light_count > 0) ? w_tri : 0.0f;
    float dir = (w_dir > 0 && scene.directional_light_count > 0) ? w_dir : 0.0f;
    float env = (w_env > 0 && scene.environment_proj >= 0) ? w_env : 0.0f;
    float sum = point + tri + dir + env;
    float inv_sum = sum <= 0.0f ? 0.0f : (1.0f / sum + 1e-5f);
    prob_point = point * inv_sum; prob_tri = tri * inv_sum; prob_dir = dir * inv_sum; prob_env = env * inv_sum;
}

// Streams of the current device, kept for the life of the process and classified by hardware pipe (stream_pool.hip): a new stream
// for a taker whose launches must overlap those of `overlap_with` (streams of any origin, the null stream included).
int stream_pool_acquire(hipStream_t* out, const hipStream_t* overlap_with = nullptr, int n_overlap = 0);
void stream_pool_release(hipStream_t s);
// The pipe class of any stream (-1: unknown).  A stream the pool did not create is classified by the experiment the first time it is
// seen: with `blocking` the stream is synchronised for it (trhip_stream_pipe_class: the caller asked); without, only a stream that is
// idle and not capturing is probed, anything else is -1 for now.
int stream_pool_class(hipStream_t s, int* cls, bool blocking = false);
int stream_pool_pipe_classes(int* classes_out, int* streams_out);      // distinct classes this process reaches on the current device

struct PathBuffers;
struct PtParams;

class PtStage {
public:
    PtStage(DeviceScene* scene, const trhip_pt_options& opt);
    ~PtStage();
    int render(const trhip_pt_targets& targets, uint target_w, uint target_h, uint viewports, hipStream_t stream);
    int get_counters(trhip_counters* out, hipStream_t stream);
    int reset_counters();
    int get_timings(trhip_timings* out);
    int get_phase_counters(trhip_phase_counters* out, hipStream_t stream);
    int get_light_counters(trhip_light_counters* out, hipStream_t stream);
    int get_max_stack_depth(uint32_t* out, hipStream_t stream);
    int get_terminal_counters(trhip_terminal_counters* out, hipStream_t stream);
    int get_program(trhip_program_info* out);
    int terminal_query_in_effect() const;
    int primary_start_in_effect() const;
    bool shades_with_cli_set() const;

    DeviceScene* scene;
    trhip_pt_options opt;
    trhip_distribution dist;
    uint frame_counter = 0;          // rt_stage::frame_counter (src/rt_stage.cc:81-86)
    uint accumulated_samples = 0;    // rt_camera_stage::accumulated_samples (src/rt_camera_stage.cc:100)
    int count_work = 0, detailed_timing = 0;
    // trhip_pt_set_shard: which viewports / samples of the whole job this stage renders (view and sample sharding)
    uint shard_vp_base = 0, shard_vp_stride = 1, shard_sample_base = 0, shard_sample_stride = 1;
    int frame_slots = 0;             // trhip_pt_set_frame_slots: stages rendering next to this one (0 = unknown)
    int lanes = 0;                   // trhip_pt_set_lanes: 0 = automatic
    int last_lanes = 0, last_lane_pipes[4] = {-1, -1, -1, -1};      // trhip_pt_get_lane_pipes
    hipStream_t last_main = nullptr;
    void* tm_display = nullptr;      // trhip_pt_set_fused_tonemap
    trhip_tonemap_info tm_info{};
    uint frame_batch = 1;            // trhip_pt_set_frame_batch: consecutive frames per render() call
    int ieee_shading = -1;           // trhip_pt_set_shading_arithmetic: 1 = k_shade at IEEE fp32 for every option set, 0 = Vulkan-grade arithmetic for the command-line set, -1 = TRHIP_SHADE_FAST decides
    int specialize = -1;             // trhip_pt_set_specialization: 1 = a shading program compiled for this stage's option set (hipRTC / kernel cache), 0 = the general kernels, -1 = TRHIP_SPECIALIZE decides (default on)
    int terminal_query = -1;         // trhip_pt_set_terminal_query: TRHIP_TERMINAL_QUERY_AUTO / _OFF, -1 = TRHIP_TERMINAL_QUERY decides (default auto)
    int primary_start = -1;          // trhip_pt_set_primary_start: TRHIP_PRIMARY_START_AUTO / _OFF, -1 = TRHIP_PRIMARY_START decides (default auto)
    int last_primary_start = -1;     // whether the last frame rendered started its paths that way (-1: no frame yet)
    bool direct = false;             // direct_stage instead of path_tracer_stage (trhip_direct_create)
    // sh_path_tracer_stage instead (trhip_sh_create): render() traces the batch `probes` names - k_sh_raygen instead of k_raygen, the bounce
    // loop with hidden lights and the first-bounce clamp on the general kernels, no resolve (sh_probes.hip projects the path state)
    bool probe_mode = false;
    const ShProbeBatch* probes = nullptr;
    const PathBuffers* path_buffers() const;
    hipStream_t last_stream = nullptr;

    // which kernels shade this stage (render() and get_program() decide it the same way)
    struct Program { bool cli_set, shade_fast, wide; const struct SpecKernels *shade, *raygen; };
    Program choose_program();

private:
    struct Impl;
    Impl* impl;
    bool timing_pending = false;
    // the steps of render(), in its order (path_tracer.hip)
    struct Frame;
    struct LaneCtx;
    int validate_call(uint viewports) const;
    void make_params(PtParams& P, const trhip_pt_targets& targets, uint target_w, uint target_h, uint viewports, uint launch_w, uint launch_h) const;
    void report_lane_pipes(int n_lanes, hipStream_t stream);
    int render_direct(Frame& f);
    int enqueue_item(Frame& f, const struct EnqueueItem& it);
    void enqueue_raygen(Frame& f, LaneCtx& c);
    int enqueue_bounce(Frame& f, LaneCtx& c, int bounce, int sample);
    int enqueue_finish(Frame& f, int lane, int pass);
    int ensure_buffers(size_t n, bool lobe_sums);
    int resolve_pending();
    void free_buffers();
};

}  // namespace tr
