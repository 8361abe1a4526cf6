// The path tracer's frame schedule without a device (tauray_amd/csrc/pt_schedule.h): plan_frame, the enqueue order and the rule for the
// caller's stream class.  A stand-alone program:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o pt_schedule_check tests/pt_schedule_check.cc && ./pt_schedule_check
// The expected values are worked out by hand from the expressions render() had before the schedule became a function (the arithmetic is
// in the comments), not printed from plan_frame.  Unless a case says otherwise: default switches, 256 CUs, 6 / 8 resident waves for the
// closest-hit / shadow kernel, blocks of 256, one pass of one sample, no timing or counting, lanes = 0.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../tauray_amd/csrc/pt_schedule.h"

using namespace tr;

#define EXPECT(x) do { if (!(x)) { std::printf("pt_schedule_check: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static FrameRequest frame(uint32_t w, uint32_t h) {
    FrameRequest rq;
    rq.n = (uint64_t)w * h; rq.launch_w = w; rq.launch_h = h; rq.viewports = 1;
    rq.max_bounces = 4;
    return rq;
}

struct Item { int lane, pass; Step step; int bounce; };
static bool operator==(const Item& a, const Item& b) { return a.lane == b.lane && a.pass == b.pass && a.step == b.step && (a.step != Step::Bounce || a.bounce == b.bounce); }
static std::vector<Item> order_of(const FrameSchedule& s) {
    std::vector<Item> v;
    for_each_enqueue_item(s, [&](const EnqueueItem& it) { v.push_back(Item{it.lane, it.pass, it.step, it.bounce}); return 0; });
    return v;
}
static std::vector<Item> lane_after_lane(int lanes, int passes) {
    std::vector<Item> v;
    for (int l = 0; l < lanes; ++l) for (int p = 0; p < passes; ++p) v.push_back(Item{l, p, Step::WholePass, 0});
    return v;
}
static std::vector<Item> in_turn(int lanes, int max_bounces) {      // max_bounces + 2 steps, each over lanes 0 .. lanes - 1
    std::vector<Item> v;
    for (int l = 0; l < lanes; ++l) v.push_back(Item{l, 0, Step::Raygen, 0});
    for (int b = 0; b < max_bounces; ++b) for (int l = 0; l < lanes; ++l) v.push_back(Item{l, 0, Step::Bounce, b});
    for (int l = 0; l < lanes; ++l) v.push_back(Item{l, 0, Step::Finish, 0});
    return v;
}
static ScheduleSwitches switches(const std::map<std::string, std::string>& env) {
    return parse_schedule_switches([&](const char* name) -> const char* { auto it = env.find(name); return it == env.end() ? nullptr : it->second.c_str(); });
}

static int check_1080p() {
    const ScheduleSwitches sw;
    FrameRequest rq = frame(1920, 1080);      // 2 073 600 paths >= 2 x 100 000: four lanes
    FrameSchedule s = plan_frame(rq, sw);
    EXPECT(!s.sample_lanes && s.n_lanes == 4 && s.lanes_used == 4 && s.fused && !s.overlap && s.pixel_lanes);
    EXPECT(s.grid_cap == 768 && s.closest_cap == 768 && s.shadow_cap == 768);      // three blocks per CU
    EXPECT(s.per_lane == 518400 && s.tile_lanes == 4 && s.tiles_per_lane == 8100);   // 32 400 tiles of 64
    for (int l = 0; l < 4; ++l) {
        const LanePlan& c = s.lane[l];
        EXPECT(c.id_offset == 518400u * l && c.n_ids == 518400);
        EXPECT(c.blocks_all == 2025 && c.blocks_q == 768 && c.blocks_f == 768 && c.shade_blocks == 768);      // 518 400 / 256; min(768, 2 x 2025)
    }
    EXPECT(s.spill_regions == 4 && s.spill_blocks == 768);      // min(768, 2 x 2025 + 1)
    EXPECT(s.state_paths == rq.n && s.passes == 1);
    EXPECT(!s.interleave && !s.merged_raygen && order_of(s) == lane_after_lane(4, 1));      // previous frame unknown
    rq.prev_frame_ms = 2.5f;
    s = plan_frame(rq, sw);
    EXPECT(s.interleave && s.merged_raygen && order_of(s) == in_turn(4, 4) && order_of(s).size() == 4 * 6);
    rq.primary_start = true;
    s = plan_frame(rq, sw);
    EXPECT(s.interleave && !s.merged_raygen && order_of(s) == in_turn(4, 4));
    rq.primary_start = false; rq.prev_frame_ms = 3.0f;
    s = plan_frame(rq, sw);
    EXPECT(!s.interleave && !s.merged_raygen && order_of(s) == lane_after_lane(4, 1));
    // the order pinned either way
    rq.prev_frame_ms = 2.5f;
    EXPECT(order_of(plan_frame(rq, switches({{"TRHIP_ENQUEUE", "lanes"}}))) == lane_after_lane(4, 1));
    rq.prev_frame_ms = 0.0f;
    s = plan_frame(rq, switches({{"TRHIP_ENQUEUE", "step"}}));
    EXPECT(s.merged_raygen && order_of(s) == in_turn(4, 4));
    EXPECT(!plan_frame(rq, switches({{"TRHIP_ENQUEUE", "step"}, {"TRHIP_MERGED_RAYGEN", "0"}})).merged_raygen);
    return 0;
}

static int check_strip() {      // 1920 x 135, a 1/8 strip: 259 200 paths
    const FrameSchedule s = plan_frame(frame(1920, 135), ScheduleSwitches());
    EXPECT(s.n_lanes == 4 && s.lanes_used == 4 && s.per_lane == 64832);      // 64 800 up to whole tiles
    EXPECT(s.tile_lanes == 1 && s.tiles_per_lane == 0);                      // 135 rows are not whole tiles, the lanes unequal
    const uint32_t blocks[4] = {254, 254, 254, 253};                         // 64 832 / 256 = 253.25, 64 704 / 256 = 252.75
    for (int l = 0; l < 4; ++l) {
        EXPECT(s.lane[l].id_offset == 64832u * l && s.lane[l].n_ids == (l < 3 ? 64832u : 64704u));
        EXPECT(s.lane[l].blocks_all == blocks[l] && s.lane[l].blocks_q == blocks[l] && s.lane[l].blocks_f == 2 * blocks[l] && s.lane[l].shade_blocks == blocks[l]);
    }
    EXPECT(s.spill_regions == 4 && s.spill_blocks == 509);      // 2 x ceil(64 800 / 256) + 1
    return 0;
}

static int check_small_frames() {
    FrameSchedule s = plan_frame(frame(500, 300), ScheduleSwitches());      // 150 000 paths: between one and two times 100 000
    EXPECT(s.n_lanes == 2 && s.lanes_used == 2 && !s.pixel_lanes && s.grid_cap == 1024 && s.closest_cap == 1024 && s.shadow_cap == 1024);
    EXPECT(s.per_lane == 75008 && s.tile_lanes == 1);      // 75 000 up to whole tiles; 500 is not whole tiles
    EXPECT(s.lane[0].n_ids == 75008 && s.lane[1].n_ids == 74992 && s.lane[0].blocks_all == 293 && s.lane[1].blocks_all == 293);
    for (int l = 0; l < 2; ++l) EXPECT(s.lane[l].shade_blocks == std::min(s.lane[l].blocks_all, 2048u));
    s = plan_frame(frame(256, 256), ScheduleSwitches());        // 65 536 paths
    EXPECT(s.n_lanes == 1 && s.lanes_used == 1 && s.fused && !s.overlap && s.spill_regions == 1);
    EXPECT(s.lane[0].n_ids == 65536 && s.lane[0].blocks_all == 256 && s.lane[0].blocks_f == 512 && s.grid_cap == 1024 && s.spill_blocks == 513);
    EXPECT(order_of(s) == lane_after_lane(1, 1));
    return 0;
}

static int check_profiling() {
    FrameRequest rq = frame(1920, 1080);
    rq.timing = true;
    FrameSchedule s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.n_lanes == 1 && !s.fused && !s.overlap);
    EXPECT(s.closest_cap == 1536 && s.shadow_cap == 2048);      // 256 CUs x 6, x 8: the resident blocks
    EXPECT(s.lane[0].blocks_all == 8100 && s.lane[0].blocks_q == 2048 && s.lane[0].shade_blocks == s.lane[0].blocks_q);
    EXPECT(s.spill_regions == 1 && s.spill_blocks == 2048);
    rq.timing = false; rq.count = true; rq.lanes = 1;
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.n_lanes == 1 && !s.fused && s.overlap && s.spill_regions == 2 && s.grid_cap == 1024);
    EXPECT(!plan_frame(rq, switches({{"TRHIP_OVERLAP", "0"}})).overlap);
    rq.count = false;
    s = plan_frame(rq, switches({{"TRHIP_FUSED", "0"}}));
    EXPECT(!s.fused && s.overlap);
    return 0;
}

static int check_sample_lanes() {
    FrameRequest rq = frame(640, 360);      // 230 400 paths; 4 x 230 400 x 224 bytes of state is 206 MB
    rq.samples_per_pixel = 4;
    FrameSchedule s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.sample_lanes && s.n_lanes == 4 && s.lanes_used == 4 && s.passes == 4 && s.state_paths == 4 * rq.n && !s.pixel_lanes);
    for (int l = 0; l < 4; ++l) EXPECT(s.lane[l].id_offset == 0 && s.lane[l].n_ids == rq.n && s.lane[l].blocks_all == 900);
    EXPECT(s.grid_cap == 1024 && s.closest_cap == 1024 && s.shadow_cap == 1024 && s.tile_lanes == 1);
    EXPECT((order_of(s) == std::vector<Item>{{0, 0, Step::WholePass, 0}, {1, 1, Step::WholePass, 0}, {2, 2, Step::WholePass, 0}, {3, 3, Step::WholePass, 0}}));
    rq.samples_per_pixel = 3;
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.sample_lanes && s.n_lanes == 3 && s.state_paths == 3 * rq.n);
    rq.samples_per_pixel = 6;      // more passes than lanes: pass p on lane p mod 4
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.n_lanes == 4 && order_of(s).size() == 6 && (order_of(s)[4] == Item{0, 4, Step::WholePass, 0}) && (order_of(s)[5] == Item{1, 5, Step::WholePass, 0}));
    rq.samples_per_pixel = 4; rq.lanes = 2;
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(!s.sample_lanes && s.n_lanes == 2 && s.state_paths == rq.n);
    rq.lanes = 0;
    EXPECT(!plan_frame(rq, switches({{"TRHIP_SAMPLE_LANES", "0"}})).sample_lanes);
    rq = frame(4000, 2500);                 // 10 000 000 paths: 4 x 224 bytes each is 8.96e9 > 8 GiB
    rq.samples_per_pixel = 4;
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(!s.sample_lanes && s.n_lanes == 4 && s.pixel_lanes && s.state_paths == rq.n && s.passes == 4);
    EXPECT(order_of(s) == lane_after_lane(4, 4));      // every lane its passes one after the other
    rq.prev_frame_ms = 1.0f;
    EXPECT(!plan_frame(rq, ScheduleSwitches()).interleave);      // in turn is for one-pass frames
    return 0;
}

static int check_frame_slots() {
    FrameRequest rq = frame(1920, 1080);
    rq.frame_slots = 2;
    FrameSchedule s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.n_lanes == 2 && s.grid_cap == 768 && s.closest_cap == 768 && s.shadow_cap == 768);
    EXPECT(s.lane[0].blocks_all == 4050 && s.lane[0].shade_blocks == 768 && s.lane[1].shade_blocks == 768);
    rq.frame_slots = 3;
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.n_lanes == 1 && s.grid_cap == 768 && s.closest_cap == 768 && s.shadow_cap == 768 && s.lane[0].shade_blocks == 2048);      // min(8100, 2048)
    rq.frame_slots = 4;
    s = plan_frame(rq, ScheduleSwitches());
    EXPECT(s.n_lanes == 1 && s.grid_cap == 1024 && s.closest_cap == 1024 && s.shadow_cap == 1024);
    rq = frame(200, 200);      // 40 000 paths < 50 000
    rq.frame_slots = 2;
    EXPECT(plan_frame(rq, ScheduleSwitches()).n_lanes == 1);
    EXPECT(plan_frame(rq, switches({{"TRHIP_SLOTS2_MIN_PATHS", "30000"}})).n_lanes == 2);
    return 0;
}

static int check_switches() {
    const ScheduleSwitches d = switches({});
    EXPECT(d.lanes == PT_LANES && d.lanes_min_paths == 100000 && d.slots2_min_paths == 50000 && d.sample_lanes && d.fused && d.overlap && !d.grid_blocks_set &&
           d.grid_blocks == 2048 && d.fused_grid_factor == 2 && d.shade_blocks == 0 && d.shade_last && d.order == ScheduleSwitches::ORDER_AUTO && d.skew == 0 && d.merged_raygen);
    FrameRequest rq = frame(1920, 1080);
    const ScheduleSwitches g = switches({{"TRHIP_GRID_BLOCKS", "300"}});
    for (int timing = 0; timing < 2; ++timing) {
        rq.timing = timing != 0;
        const FrameSchedule s = plan_frame(rq, g);
        EXPECT(s.grid_cap == 300 && s.closest_cap == 300 && s.shadow_cap == 300);
    }
    rq.timing = false;
    EXPECT(plan_frame(rq, switches({{"TRHIP_LANES", "1"}})).n_lanes == 1 && plan_frame(rq, switches({{"TRHIP_LANES", "2"}})).n_lanes == 2);
    EXPECT(plan_frame(frame(320, 192), switches({{"TRHIP_LANES_MIN_PATHS", "1"}})).n_lanes == 4);
    EXPECT(plan_frame(rq, switches({{"TRHIP_SHADE_BLOCKS", "512"}})).lane[0].shade_blocks == 512);
    EXPECT(plan_frame(frame(1920, 135), switches({{"TRHIP_FUSED_GRID_FACTOR", "1"}})).lane[0].blocks_f == 254);
    EXPECT(!plan_frame(rq, switches({{"TRHIP_SHADE_LAST", "0"}})).shade_last);
    // TRHIP_ENQUEUE=skew1, four lanes, two bounces: lane l one step behind lane l - 1
    rq.max_bounces = 2;
    const FrameSchedule s = plan_frame(rq, switches({{"TRHIP_ENQUEUE", "skew1"}}));
    const Step R = Step::Raygen, B = Step::Bounce, F = Step::Finish;
    const std::vector<Item> want = {
        {0, 0, R, 0},
        {0, 0, B, 0}, {1, 0, R, 0},
        {0, 0, B, 1}, {1, 0, B, 0}, {2, 0, R, 0},
        {0, 0, F, 0}, {1, 0, B, 1}, {2, 0, B, 0}, {3, 0, R, 0},
        {1, 0, F, 0}, {2, 0, B, 1}, {3, 0, B, 0},
        {2, 0, F, 0}, {3, 0, B, 1},
        {3, 0, F, 0}};
    EXPECT(s.interleave && s.skew == 1 && order_of(s) == want);
    return 0;
}

// The rule for the caller's stream with a fake classifier: a multi-lane frame on stream A of class 2, a one-lane frame on stream B, a
// multi-lane frame on B of class 0
static int check_main_stream_class() {
    const int A = 0, B = 0;      // two addresses
    std::vector<const void*> asked;
    const auto classify = [&](const void* s) { asked.push_back(s); return s == &A ? 2 : 0; };
    MainStreamClass m;
    m.frame_on(&A);
    EXPECT(m.look(&A, classify) && m.cls == 2 && m.stream == &A && asked.size() == 1);
    m.frame_on(&A);
    EXPECT(!m.look(&A, classify) && m.cls == 2 && asked.size() == 1);      // a known class on an unchanged stream is not asked for again
    m.frame_on(&B);                                                          // the one-lane frame: nobody looks
    EXPECT(m.cls == -1 && m.tries == 0 && m.stream == &B && asked.size() == 1);
    m.frame_on(&B);
    EXPECT(m.look(&B, classify) && m.cls == 0 && asked.size() == 2 && asked.back() == &B);
    EXPECT(!m.look(&B, classify) && asked.size() == 2);
    EXPECT(m.look(&A, classify) && m.cls == 2 && asked.size() == 3);       // look() alone moves too
    int calls = 0;
    const auto unknown = [&](const void*) { ++calls; return -1; };
    MainStreamClass u;
    for (int i = 0; i < 40; ++i) EXPECT(!u.look(&B, unknown) && u.cls == -1);
    EXPECT(calls == 16);
    return 0;
}

int main() {
    if (check_1080p() || check_strip() || check_small_frames() || check_profiling() || check_sample_lanes() || check_frame_slots() || check_switches() ||
        check_main_stream_class())
        return 1;
    std::printf("ok\n");
    return 0;
}
