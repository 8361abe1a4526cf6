// The host skeleton of the stage objects (tauray_amd/csrc/stage_host.h) on a machine without a device, for a run under the host sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o stage_host_check tests/stage_host_check.cc && ./stage_host_check
// A derived stage is built and destroyed, create's failure tail releases it and reports "<fn>: <hip error>", a stage that has run no frame
// gives zero timings without touching the device, and a download of the wrong size is refused with both sizes.  The host side of a
// viewport frame: the list check and the scene check say each of their refusals and accept what is valid, and a list is walked in chunks of
// 64 with every entry in order.  Prints "ok" and returns 0.
#include "../tauray_amd/csrc/stage_host.h"

#include <cstdio>
#include <utility>

static std::string last_error;
namespace tr {
int set_error(const std::string& msg) { last_error = msg; return 1; }
int device_index(const trhip_device*) { return 0; }
DeviceScene* device_scene(trhip_device*) { return nullptr; }
}  // namespace tr

struct two_event_stage : tr::StageHost<> { float* image = nullptr; uint8_t* bytes = nullptr; };
struct five_event_stage : tr::StageHost<5> { float* image[2] = {}; };
struct timings { float total_ms; uint32_t frames; };
struct list64 { uint32_t v[64]; };      // the shape of ViewportList (first_hit.h), which needs the device headers

// The chunks of a list of `count` viewports 1000, 1001, ...; empty when an entry is out of place or a chunk's tail is not zero.
static std::vector<std::pair<uint32_t, uint32_t>> chunks_of(uint32_t count)
{
    std::vector<uint32_t> viewports(count);
    for(uint32_t i = 0; i < count; ++i) viewports[i] = 1000 + i;
    std::vector<std::pair<uint32_t, uint32_t>> seen;
    bool in_order = true;
    tr::for_each_viewport_chunk<list64>(viewports.data(), count, [&](uint32_t first, uint32_t n, const list64& list) {
        for(uint32_t i = 0; i < 64; ++i) in_order = in_order && list.v[i] == (i < n ? 1000 + first + i : 0);
        seen.push_back({first, n});
    });
    if(!in_order) seen.clear();
    return seen;
}

#define EXPECT(x) do { if(!(x)) { std::printf("stage_host_check: %s failed (line %d; last error: %s)\n", #x, __LINE__, last_error.c_str()); return 1; } } while(0)

int main()
{
    // the viewport list of a frame: every refusal verbatim, the layer bound only where there is one, a valid list
    {
        const uint32_t list[3] = {0, 4, 2};
        EXPECT(tr::check_viewport_list("check_render", nullptr, 3, 3, 5) == 1 && last_error == "check_render: null argument");
        EXPECT(tr::check_viewport_list("check_render", list, 3, 2, 5) == 1 && last_error == "check_render: 3 viewports, the stage has 2 layers");
        EXPECT(tr::check_viewport_list("check_render", list, 0, 2, 5) == 1 && last_error == "check_render: 0 viewports, the stage has 2 layers");
        EXPECT(tr::check_viewport_list("check_render", list, 3, 3, 4) == 1 && last_error == "check_render: viewport 4 out of range");
        EXPECT(tr::check_viewport_list("check_render", list, 3, 0, 4) == 1 && last_error == "check_render: viewport 4 out of range");
        last_error.clear();
        EXPECT(tr::check_viewport_list("check_render", list, 3, 3, 5) == 0 && tr::check_viewport_list("check_render", list, 3, 0, 5) == 0);
        EXPECT(tr::check_viewport_list("check_render", list, 3, 64, 5) == 0 && tr::check_viewport_list("check_render", list, 0, 0, 5) == 0 && last_error.empty());
    }
    {
        EXPECT(tr::check_scene_ready("check_render", 0, false) == 1 && last_error == "check_render: no scene (trhip_scene_upload)");
        EXPECT(tr::check_scene_ready("check_render", 0, true) == 1 && last_error == "check_render: no scene (trhip_scene_upload)");
        EXPECT(tr::check_scene_ready("check_render", 6, false) == 1 && last_error == "check_render: no acceleration structure: call trhip_scene_build_accel first");
        last_error.clear();
        EXPECT(tr::check_scene_ready("check_render", 6, true) == 0 && last_error.empty());
    }
    // a list in chunks of one launch
    {
        using seq = std::vector<std::pair<uint32_t, uint32_t>>;
        EXPECT(chunks_of(0) == seq{});
        EXPECT(chunks_of(1) == (seq{{0, 1}}));
        EXPECT(chunks_of(63) == (seq{{0, 63}}));
        EXPECT(chunks_of(64) == (seq{{0, 64}}));
        EXPECT(chunks_of(65) == (seq{{0, 64}, {64, 1}}));
        EXPECT(chunks_of(128) == (seq{{0, 64}, {64, 64}}));
        EXPECT(chunks_of(129) == (seq{{0, 64}, {64, 64}, {128, 1}}));
    }

    // from here on: what happens without a device
    int devices = 0;
    if(hipGetDeviceCount(&devices) == hipSuccess && devices > 0) { std::printf("stage_host_check: this check is for a machine without a device\n"); return 2; }

    // a derived stage lives and dies, through delete and through the shared destroy
    delete new two_event_stage;
    tr::stage_destroy(new five_event_stage);
    tr::stage_destroy((two_event_stage*)nullptr);

    // create's tail: the first error is kept, nothing after it is tried, the stage is released and the text names the function
    {
        two_event_stage* s = new two_event_stage;
        s->alloc_zeroed(s->image, 1024);
        const hipError_t first = s->err;
        s->alloc_zeroed(s->bytes, 16);
        EXPECT(first != hipSuccess && s->err == first && !s->image && !s->bytes && s->allocations.empty());
        two_event_stage* out = nullptr;
        EXPECT(tr::stage_finish_create("check_create", s, &out) == 1 && out == nullptr);
        EXPECT(last_error == std::string("check_create: ") + hipGetErrorString(first));
    }
    {
        five_event_stage* s = new five_event_stage;      // no allocation at all: the events are the first thing to fail
        five_event_stage* out = nullptr;
        EXPECT(tr::stage_finish_create("check_create5", s, &out) == 1 && out == nullptr && last_error.rfind("check_create5: ", 0) == 0);
    }

    // no frame yet: zeros, and the device is not asked
    {
        five_event_stage s;
        timings t = {1.0f, 7};
        last_error.clear();
        EXPECT(tr::stage_total_ms("check_timings", &s, &t) == 0 && t.total_ms == 0.0f && t.frames == 0 && last_error.empty());
        EXPECT(tr::stage_total_ms("check_timings", (five_event_stage*)nullptr, &t) == 1 && last_error == "check_timings: null argument");
        EXPECT(tr::stage_total_ms("check_timings", &s, (timings*)nullptr) == 1);
        s.frames = 1;      // a frame has run: now the device is asked, and there is none
        EXPECT(tr::stage_total_ms("check_timings", &s, &t) == 1 && t.frames == 1 && last_error.rfind("hipSetDevice: ", 0) == 0);
    }

    // download: null arguments, the stage's own refusal, the two sizes
    {
        two_event_stage s;
        char host[8] = {};
        int asked = 0;
        auto find = [&](const void*& src, size_t& size) { ++asked; src = host; size = 8; return 0; };
        EXPECT(tr::stage_download("check_download", (two_event_stage*)nullptr, host, 8, find) == 1 && last_error == "check_download: null argument" && asked == 0);
        EXPECT(tr::stage_download("check_download", &s, nullptr, 8, find) == 1 && asked == 0);
        EXPECT(tr::stage_download("check_download", &s, host, 3, find) == 1 && last_error == "check_download: 3 bytes asked, the buffer has 8" && asked == 1);
        EXPECT(tr::stage_download("check_download", &s, host, 8, [&](const void*&, size_t&) { return tr::set_error("check_download: unknown buffer"); }) == 1);
        EXPECT(last_error == "check_download: unknown buffer");
        EXPECT(tr::stage_download("check_download", &s, host, 8, find) == 1 && last_error.rfind("hipSetDevice: ", 0) == 0);      // the right size: on to the device
    }

    std::printf("ok\n");
    return 0;
}
