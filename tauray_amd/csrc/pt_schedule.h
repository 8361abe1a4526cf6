// How a frame of the path tracer is cut into lanes and launches: every decision PtStage::render (path_tracer.hip) takes before it
// enqueues anything, as one pure function of the frame's numbers and the TRHIP_* scheduling switches.  Host only: no HIP header, no
// kernel header, no heap - tests/pt_schedule_check.cc compiles it alone and checks the decisions without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace tr {

#ifndef TR_PT_LANES
#define TR_PT_LANES 4           // -DTR_PT_LANES=8: an experiment (more lanes than hardware pipes, TRHIP_LANES=5 ... 8; profiles/r6/lone_frame_phase_ab.txt)
#endif
constexpr int PT_LANES = TR_PT_LANES;   // independent slices of a frame that run concurrently (plan_frame)

// The scheduling switches of the process's environment.  schedule_switches() reads them once; nothing else in the path tracer's host reads one.
struct ScheduleSwitches {
    int lanes = PT_LANES;                 // TRHIP_LANES: most lanes of a frame
    uint64_t lanes_min_paths = 100000;    // TRHIP_LANES_MIN_PATHS: below it one lane, below twice it two
    uint64_t slots2_min_paths = 50000;    // TRHIP_SLOTS2_MIN_PATHS: a stage of a two-slot renderer runs two lanes from here on
    bool sample_lanes = true;             // TRHIP_SAMPLE_LANES=0: no sample lanes
    bool fused = true;                    // TRHIP_FUSED=0: shadow(b) in a launch of its own
    bool overlap = true;                  // TRHIP_OVERLAP=0: ... and on the lane's own stream
    bool grid_blocks_set = false;         // TRHIP_GRID_BLOCKS: most blocks of a persistent trace launch; set, it overrides every cap below
    uint32_t grid_blocks = 256u * 8u;
    uint32_t fused_grid_factor = 2;       // TRHIP_FUSED_GRID_FACTOR: blocks of a fused launch per block of paths of its lane (two queues: 2 gives every chunk of both a wave)
    uint32_t shade_blocks = 0;            // TRHIP_SHADE_BLOCKS: most blocks of a k_shade launch (0: plan_frame's own)
    bool shade_last = true;               // TRHIP_SHADE_LAST=0: the last bounce shades with the general instance
    enum Order { ORDER_AUTO, ORDER_LANES, ORDER_STEP } order = ORDER_AUTO;      // TRHIP_ENQUEUE=lanes | step | skew<k> pins the enqueue order
    int skew = 0;                         // TRHIP_ENQUEUE=skew<k>: lane l runs k steps behind lane l - 1 (0 = all lanes in step)
    bool merged_raygen = true;            // TRHIP_MERGED_RAYGEN=0: a k_raygen per lane even when the lanes run in step
};

template <class Getenv> inline ScheduleSwitches parse_schedule_switches(Getenv&& get) {
    ScheduleSwitches s;
    const auto off = [&](const char* name) { const char* v = get(name); return v && atoi(v) == 0; };
    if (const char* v = get("TRHIP_LANES")) s.lanes = atoi(v);
    if (const char* v = get("TRHIP_LANES_MIN_PATHS")) s.lanes_min_paths = (uint64_t)atol(v);
    if (const char* v = get("TRHIP_SLOTS2_MIN_PATHS")) s.slots2_min_paths = (uint64_t)atol(v);
    s.sample_lanes = !off("TRHIP_SAMPLE_LANES");
    s.fused = !off("TRHIP_FUSED");
    s.overlap = !off("TRHIP_OVERLAP");
    if (const char* v = get("TRHIP_GRID_BLOCKS")) { s.grid_blocks_set = true; s.grid_blocks = (uint32_t)atoi(v); }
    if (const char* v = get("TRHIP_FUSED_GRID_FACTOR")) s.fused_grid_factor = (uint32_t)std::max(1, atoi(v));
    if (const char* v = get("TRHIP_SHADE_BLOCKS")) s.shade_blocks = (uint32_t)atoi(v);
    s.shade_last = !off("TRHIP_SHADE_LAST");
    if (const char* v = get("TRHIP_ENQUEUE")) {
        s.order = strcmp(v, "lanes") != 0 ? ScheduleSwitches::ORDER_STEP : ScheduleSwitches::ORDER_LANES;
        if (!strncmp(v, "skew", 4)) s.skew = atoi(v + 4);
    }
    s.merged_raygen = !off("TRHIP_MERGED_RAYGEN");
    return s;
}

inline const ScheduleSwitches& schedule_switches() {
    static const ScheduleSwitches s = parse_schedule_switches([](const char* name) { return (const char*)getenv(name); });
    return s;
}

// What the decisions depend on, and nothing else
struct FrameRequest {
    uint64_t n = 0;                        // paths of the launch: launch_w * launch_h * viewports
    uint32_t launch_w = 0, launch_h = 0, viewports = 1;
    int samples_per_pixel = 1, samples_per_pass = 1, max_bounces = 1;
    bool direct = false, timing = false, count = false;
    int lanes = 0;                         // trhip_pt_set_lanes: 0 = automatic
    int frame_slots = 0;                   // trhip_pt_set_frame_slots
    float prev_frame_ms = 0.0f;            // device time of the stage's previous frame (0 = unknown)
    bool primary_start = false;            // the launch of bounce 0 starts the paths: the frame has no k_raygen
    uint32_t n_cu = 256, block_size = 256; // the device's compute units; threads of a block of every kernel of the frame
    uint32_t closest_waves = 6, shadow_waves = 8;      // resident waves per SIMD (= blocks per CU) at the closest-hit and the shadow kernel's register budget
};

struct LanePlan {
    uint32_t id_offset = 0, n_ids = 0;     // the lane's launch ids
    uint32_t blocks_all = 0;               // one thread per id
    uint32_t blocks_q = 0;                 // a queue kernel: enough blocks to fill the chip, striding over the queue
    uint32_t blocks_f = 0;                 // a fused launch
    uint32_t shade_blocks = 0;             // k_shade
};

// One step of one pass of one lane, so that the steps of several lanes can be enqueued in turn
enum class Step { WholePass, Raygen, Bounce, Finish };      // Finish: the accumulation and k_resolve
struct EnqueueItem { int lane, pass; Step step; int bounce; };      // bounce: of Step::Bounce

struct FrameSchedule {
    bool sample_lanes = false;             // the lanes take turns with whole one-sample passes, each with path state of its own
    int passes = 1;
    uint64_t state_paths = 0;              // paths the state arrays hold: n per sample lane
    int n_lanes = 1;                       // streams of the frame (sample lanes: how many of them)
    int lanes_used = 1;                    // lanes that have launch ids (a tiny frame may leave the last ones none)
    bool fused = false;                    // shadow(b) rides in the launch of closest(b + 1)
    bool overlap = false;                  // one lane, shadow(b) on the side stream next to closest(b + 1)
    bool pixel_lanes = false;
    uint32_t grid_cap = 0, closest_cap = 0, shadow_cap = 0;
    uint32_t spill_regions = 1, spill_blocks = 1;      // the quad-tail spill buffer: regions, and the blocks of the largest trace launch of a lane
    uint32_t per_lane = 0, tile_lanes = 1, tiles_per_lane = 0;
    LanePlan lane[PT_LANES];
    bool shade_last = true;                // the last bounce's k_shade is the `last` instance
    bool interleave = false;               // the lanes' steps in turn, not lane after lane
    int skew = 0;
    bool merged_raygen = false;            // one k_raygen over every lane's ids on the caller's stream, ahead of the fork
    int max_bounces = 1;
};

inline FrameSchedule plan_frame(const FrameRequest& rq, const ScheduleSwitches& sw) {
    FrameSchedule s;
    const uint64_t n = rq.n;
    const uint32_t KB = rq.block_size;
    const bool timing = rq.timing;
    s.max_bounces = rq.max_bounces;
    s.passes = rq.samples_per_pixel / rq.samples_per_pass;
    // Concurrency inside a frame.  The trace kernels are persistent and leave the chip under-filled while their last
    // waves finish, the bounce loop is a chain of dependent launches, and trace (VALU-bound) and shade (latency-bound)
    // want different resources.  Ways to fill the gaps, all bit-neutral:
    //  * lanes (default, four = the HIP runtime's hardware queues): the path ids are cut into slices with their own
    //    queues and counters, and every slice runs its whole bounce loop on its own stream, so one slice's shade overlaps
    //    another's traversal;
    //  * TRHIP_LANES=1: one lane; shadow(b) shares the launch of closest(b + 1) (k_trace_fused), or - TRHIP_FUSED=0 - runs
    //    on a side stream next to it.
    // Per-kernel timing (trhip_pt_set_profiling) wants kernels that own the chip: one lane, one stream.
    //  * sample lanes (a frame of two or more one-sample passes, the offline case - BASELINE config 3 is 4096 of them): the lanes
    //    take turns with whole samples instead of sharing one, each with path state of its own (so every lane needs state for all n
    //    paths), so that up to four samples are in flight like the frames of a renderer with frame slots (3.4 instead of 4.0 ms per
    //    sample on sponza_class).  A pass ends in k_resolve, which blends into the targets and therefore runs in pass order: each one
    //    waits for the previous pass's, on whatever lane that ran.
    const int sample_lane_count = std::min(s.passes, PT_LANES);
    s.sample_lanes = sw.sample_lanes && !rq.direct && !timing && rq.lanes == 0 && rq.samples_per_pass == 1 && s.passes >= 2 &&
                     n * (uint64_t)sample_lane_count * 224u <= ((uint64_t)8 << 30);
    s.state_paths = s.sample_lanes ? n * (uint64_t)sample_lane_count : n;
    // Small frames (the shards of a multi-GPU job) are bound by the latency of one ray's dependent fetches per kernel, not by
    // throughput; extra lanes pay as long as a lane still has a few hundred blocks.  One frame at a time, sponza_teapots, lanes
    // 1 / 2 / 4 (profiles/r5/lanes_by_share.txt, every lane on a hardware pipe of its own - stream_pool.hip; round 3's
    // thresholds were measured with whatever pipes the streams had landed on): 65 k paths 0.50 / 0.52 / 0.55 ms, 130 k
    // 0.60 / 0.57 / 0.61, 261 k 0.94 / 0.79 / 0.74, 518 k 1.49 / 1.40 / 1.17, 1.04 M 2.52 / 2.30 / 2.16, 2.07 M 4.48 / 3.96 / 3.70.
    //  * a stage of a renderer with frames in flight (trhip_pt_set_frame_slots): the frames overlap each other, so one lane per frame -
    //    except with two slots, where two lanes each put the pair on all four hardware pipes (two in flight, one frame per launch:
    //    3.57 -> 3.43 ms on sponza_teapots, 3.05 -> 2.92 sponza_class, 1.80 -> 1.66 test.glb; profiles/r5/two_in_flight_lanes.txt)
    const int auto_lanes = rq.frame_slots >= 3 ? 1
                         : rq.frame_slots == 2 ? (n < sw.slots2_min_paths ? 1 : std::min(sw.lanes, 2))
                         : (n < sw.lanes_min_paths ? 1 : std::max(1, std::min(n < 2 * sw.lanes_min_paths ? std::min(sw.lanes, 2) : sw.lanes, PT_LANES)));
    const int n_lanes = s.n_lanes = s.sample_lanes ? sample_lane_count : (timing ? 1 : (rq.lanes > 0 ? std::min(rq.lanes, PT_LANES) : auto_lanes));
    // shadow(b) rides in the launch of closest(b + 1) unless kernels are being timed or counted one by one
    s.fused = sw.fused && !timing && !rq.count;
    s.overlap = sw.overlap && !timing && !s.fused && n_lanes == 1;
    // Trace launches of frames that share the chip - with the other frames in flight (frame slots, one lane each) or with the
    // other three lanes of their own frame - get four blocks per CU instead of eight, which leaves room for the launches next
    // to them (four slots: sponza_teapots 4.33 -> 4.18 ms per frame, sponza_class 3.59 -> 3.44; four lanes of a lone frame:
    // 4.78 -> 4.52 ms, profiles/r2/schedule_sweep.txt).  Only a kernel that is timed alone wants the whole chip.
    // Round 5 (profiles/r5/sync_schedule_sweep.txt, lone_frame_grids.txt): with the round's faster traversal the four pixel lanes of a lone frame want
    // smaller grids still - three blocks per CU for the trace launches and for k_shade (768 / 768 instead of 1024 / 2048): a lane's launch
    // then leaves half the chip to the other lanes' launches, which is what lanes are for; one frame at a time 4.06 -> 3.72 ms on
    // sponza_teapots.  Frame slots (one lane per frame, whole frames per launch) and sample lanes keep the larger grids: pipelined 3.29 ms
    // against 3.37 with the small ones.
    s.pixel_lanes = n_lanes >= 3 && !s.sample_lanes;
    const bool few_slots = (n_lanes == 1 && (rq.frame_slots == 2 || rq.frame_slots == 3)) || (n_lanes == 2 && rq.frame_slots == 2);      // trhip_pt_set_frame_slots: trace launches of three blocks per CU
    s.grid_cap = (!timing && !sw.grid_blocks_set) ? ((s.pixel_lanes || few_slots) ? 768u : 1024u) : sw.grid_blocks;
    // A trace kernel that is timed alone gets exactly the blocks that are resident at its register budget (persistent waves: a
    // block that has to wait for a slot only lengthens the tail): 1536 for the closest-hit kernel, 0.544 -> 0.527 ms per launch
    // on sponza_teapots against the 2048 both used to get; the shadow kernel's budget is 8 per CU, i.e. 2048.
    const bool resident = timing && !sw.grid_blocks_set;
    s.closest_cap = resident ? std::min(rq.n_cu * rq.closest_waves, sw.grid_blocks) : s.grid_cap;
    s.shadow_cap = resident ? std::min(rq.n_cu * rq.shadow_waves, sw.grid_blocks) : s.grid_cap;
    {   // spill regions: one per lane; a single lane whose shadow launches overlap the next closest-hit launch on the side stream
        // needs a second one (both kernels index their slices by block and wave)
        const uint64_t lane_paths = s.sample_lanes ? n : (n + (uint64_t)n_lanes - 1) / (uint64_t)n_lanes;
        s.spill_blocks = (uint32_t)std::min<uint64_t>(std::max(std::max(s.closest_cap, s.shadow_cap), s.grid_cap), sw.fused_grid_factor * ((lane_paths + KB - 1) / KB) + 1);
        s.spill_regions = (uint32_t)std::max(n_lanes, s.overlap ? 2 : 1);
    }
    // direct_stage renders on the caller's stream alone (its grids are still those of the lane count above)
    const int slices = rq.direct ? 1 : n_lanes;
    s.per_lane = (s.sample_lanes || rq.direct) ? (uint32_t)n : (uint32_t)((((n + slices - 1) / slices + 63) / 64) * 64);   // whole 8x8 tiles per lane
    {   // interleave the lanes' tiles when the image is whole tiles and divides evenly (always true for 1080p / 4 lanes)
        const uint64_t tiles = n / 64;
        const bool even = !s.sample_lanes && rq.viewports == 1 && (rq.launch_w & 7u) == 0 && (rq.launch_h & 7u) == 0 && slices > 1 && tiles % (uint64_t)slices == 0 &&
                          (uint64_t)s.per_lane * (uint64_t)slices == n;
        s.tile_lanes = even ? (uint32_t)slices : 1u;
        s.tiles_per_lane = even ? (uint32_t)(tiles / (uint64_t)slices) : 0u;
    }
    // k_shade holds its waves (768 resident blocks at three per SIMD) and strides over the queue; 2048 blocks since the
    // trace launches of a frame slot shrank to 1024 (round 2 sweep: profiles/r2/schedule_sweep.txt)
    const uint32_t shade_cap = sw.shade_blocks ? sw.shade_blocks : ((s.pixel_lanes || (n_lanes == 2 && rq.frame_slots == 2)) ? 768u : 2048u);
    s.lanes_used = 0;
    for (int l = 0; l < slices; ++l) {
        LanePlan& c = s.lane[l];
        c.id_offset = s.sample_lanes ? 0u : (uint32_t)l * s.per_lane;
        if (c.id_offset >= n) break;
        c.n_ids = std::min(s.per_lane, (uint32_t)n - c.id_offset);
        c.blocks_all = (c.n_ids + KB - 1) / KB;
        // persistent-style launch for the queue kernels: enough blocks to fill the chip, grid-stride over the queue
        c.blocks_q = std::min(c.blocks_all, s.grid_cap);
        // The fused launch carries two queues (closest-hit rays of this bounce, shadow rays of the last one): a small frame - a rank's share
        // of a multi-GPU job - leaves the chip room for a wave per chunk of both, and then the launch lasts as long as the longer of the two
        // traversals instead of their sum (a 1/8 strip of sponza_teapots: 165 -> 130 us per fused launch, profiles/r5/strip_timeline_1_8.txt)
        c.blocks_f = std::min(s.grid_cap, c.blocks_all * sw.fused_grid_factor);
        c.shade_blocks = timing ? c.blocks_q : std::min(c.blocks_all, shade_cap);   // alone on the chip it wants the full grid
        s.lanes_used = l + 1;
    }
    s.shade_last = sw.shade_last;
    // Enqueue order of the lanes of a one-pass frame (same bits either way; profiles/r3/enqueue_order_ab.txt).  Lane after lane leaves
    // the lanes a dozen launches (~60 us of host time) apart, so they run out of phase - one shades while another traces - which is
    // worth 3 % on a 4.2 ms frame (sponza_teapots); step by step in turn keeps them in phase, which is worth 6 % on a 2.2 ms frame
    // (test.glb) and costs 3 % on the long one; lanes one or two steps apart gain on neither.  So: in turn when the previous frame
    // of this stage took less than 3 ms, lane after lane otherwise.  TRHIP_ENQUEUE=lanes | step | skew<k> pins the order.
    const bool in_turn = sw.order != ScheduleSwitches::ORDER_AUTO ? sw.order == ScheduleSwitches::ORDER_STEP : (rq.prev_frame_ms > 0.0f && rq.prev_frame_ms < 3.0f);
    const bool one_sample = s.passes == 1 && rq.samples_per_pass == 1;
    s.interleave = in_turn && !s.sample_lanes && s.lanes_used > 1 && one_sample;
    s.skew = sw.skew;
    // Round 6: lanes in step share ONE ray-generation launch, on the caller's stream ahead of the fork.  A frame that short starts
    // host-bound - a launch costs the host ~10 us, and with a raygen per lane the first closest-hit launch was the fifth of the frame
    // (47 us after the frame's first kernel on a 1/8 strip of sponza_teapots, profiles/r6/strip_timeline_1_8_base.txt); now it is the
    // second.  Same kernel over all the lanes' path ids (the state of a path does not depend on its lane); block 0 zeroes every lane's
    // counters.  TRHIP_MERGED_RAYGEN=0 switches it off.  (Under the primary start there is no ray generation to merge.)
    s.merged_raygen = sw.merged_raygen && !rq.primary_start && s.interleave && s.lanes_used == n_lanes;
    return s;
}

// The frame's enqueue order: f(EnqueueItem) for every item in turn; a non-zero result ends the walk and is returned.
template <class F> inline int for_each_enqueue_item(const FrameSchedule& s, F&& f) {
    if (s.sample_lanes) {       // pass p on lane p mod lanes
        for (int pass = 0; pass < s.passes; ++pass) if (int rc = f(EnqueueItem{pass % s.lanes_used, pass, Step::WholePass, 0})) return rc;
    } else if (s.interleave) {  // lane l runs `skew` steps behind lane l - 1 (0 = all lanes in step)
        const int n_steps = s.max_bounces + 2;
        for (int t = 0; t < n_steps + s.skew * (s.lanes_used - 1); ++t)
            for (int lane = 0; lane < s.lanes_used; ++lane) {
                const int step = t - s.skew * lane;
                if (step < 0 || step >= n_steps) continue;
                const EnqueueItem it{lane, 0, step == 0 ? Step::Raygen : (step == n_steps - 1 ? Step::Finish : Step::Bounce), step - 1};
                if (int rc = f(it)) return rc;
            }
    } else {
        for (int lane = 0; lane < s.lanes_used; ++lane)
            for (int pass = 0; pass < s.passes; ++pass) if (int rc = f(EnqueueItem{lane, pass, Step::WholePass, 0})) return rc;
    }
    return 0;
}

// The pipe class of the caller's stream (stream_pool.hip): which class, when to look again, did it change.  A class is trusted only for the
// stream it was measured on; an unknown one is looked at again on later frames, 16 times at the most.
struct MainStreamClass {
    const void* stream = nullptr;      // the stream `cls` belongs to
    int cls = -1, tries = 0;
    // every frame: a frame on another stream forgets what was known of the last one
    void frame_on(const void* s) { if (s != stream) { stream = s; cls = -1; tries = 0; } }
    // a frame that runs lanes next to the stream: true when a class has just been learnt, i.e. the lanes in hand were chosen without it.
    // classify(stream) -> its class, or -1 when it cannot be told now
    template <class Classify> bool look(const void* s, Classify&& classify) {
        frame_on(s);
        if (cls >= 0 || tries >= 16) return false;
        cls = classify(s); ++tries;
        return cls >= 0;
    }
};

}  // namespace tr
