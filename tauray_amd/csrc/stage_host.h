// The host skeleton of the post-processing stage objects (bmfr.hip, reprojection.hip, taa.hip, looking_glass.hip): what every stage owns
// (its HIP device, its events, its frame counter, its device allocations) and the tails every entry point shares (finishing create,
// destroy, the total time, a size-checked download).  Host only: nothing here is seen by a kernel.  A stage struct derives from StageHost
// and keeps its own fields; argument validation, parameter packing and kernel launches stay in the stage's file.  The entry points that
// render a list of viewports (gbuffer, dshgi, restir_di, restir_gi) share the checks and the chunk walk at the end of the file.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

struct trhip_device;

namespace tr {

struct DeviceScene;
int set_error(const std::string& msg);                 // api.hip: records trhip_last_error(); returns 1
int device_index(const trhip_device* dev);             // api.hip: the HIP device of a handle, -1 for null
DeviceScene* device_scene(trhip_device* dev);          // api.hip: the scene of a handle

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return set_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define DEVCHK(idx) do { hipError_t e_ = hipSetDevice(idx); if (e_ != hipSuccess) return set_error(std::string("hipSetDevice: ") + hipGetErrorString(e_)); } while (0)

// EVENTS: ev[0] is recorded before a frame's first kernel, ev[EVENTS - 1] behind its last (BMFR has one between its passes as well).
template <int EVENTS = 2>
struct StageHost {
    int hip_device = 0;
    hipEvent_t ev[EVENTS] = {};
    uint32_t frames = 0;
    hipError_t err = hipSuccess;           // the first error of create's allocations, copies and events
    std::vector<void*> allocations;

    StageHost() = default;
    StageHost(const StageHost&) = delete;
    StageHost& operator=(const StageHost&) = delete;
    ~StageHost() {
        for (void* p : allocations) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    // After a first error nothing more is tried; p stays null unless the allocation is the stage's.
    template <class T>
    void alloc_zeroed(T*& p, size_t bytes) {
        if (err != hipSuccess) return;
        void* q = nullptr;
        err = hipMalloc(&q, bytes);
        if (err != hipSuccess) return;
        allocations.push_back(q);
        p = (T*)q;
        err = hipMemset(q, 0, bytes);
    }
    hipEvent_t last_event() const { return ev[EVENTS - 1]; }
};

// The tail of <fn> = trhip_*_create, behind the stage's alloc_zeroed calls: the events, a sync, then the stage or "<fn>: <hip error>".
template <class Stage>
int stage_finish_create(const char* fn, Stage* s, Stage** out) {
    for (hipEvent_t& e : s->ev) if (s->err == hipSuccess) s->err = hipEventCreate(&e);
    if (s->err == hipSuccess) s->err = hipDeviceSynchronize();
    if (s->err != hipSuccess) {
        const hipError_t e = s->err;
        delete s;
        return set_error(std::string(fn) + ": " + hipGetErrorString(e));
    }
    *out = s;
    return 0;
}

template <class Stage>
void stage_destroy(Stage* s) {
    if (!s) return;
    (void)hipSetDevice(s->hip_device);
    (void)hipDeviceSynchronize();
    delete s;
}

// Zeroes *out and fills frames and total_ms (every trhip_*_timings has them).  A stage that has run no frame does not touch the device.
template <class Stage, class Timings>
int stage_total_ms(const char* fn, Stage* s, Timings* out) {
    if (!s || !out) return set_error(std::string(fn) + ": null argument");
    memset(out, 0, sizeof(*out));
    out->frames = s->frames;
    if (s->frames == 0) return 0;
    DEVCHK(s->hip_device);
    HIPCHK(hipEventSynchronize(s->last_event()));
    HIPCHK(hipEventElapsedTime(&out->total_ms, s->ev[0], s->last_event()));
    return 0;
}

// find(src, size) names the buffer asked for (or refuses with the stage's own text); it runs only for a non-null stage.
template <class Stage, class Find>
int stage_download(const char* fn, Stage* s, void* host, size_t bytes, Find find) {
    if (!s || !host) return set_error(std::string(fn) + ": null argument");
    const void* src = nullptr;
    size_t size = 0;
    if (int r = find(src, size)) return r;
    if (bytes != size) return set_error(std::string(fn) + ": " + std::to_string(bytes) + " bytes asked, the buffer has " + std::to_string(size));
    DEVCHK(s->hip_device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host, src, size, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The host side of a viewport frame: what the entry points that trace the first hit of every pixel of a list of viewports share
// (trhip_gbuffer_render, trhip_dshgi_render, trhip_restir_di_render; the kernels' side is first_hit.h).  The checks take plain numbers.

// `layers`: what the stage's images hold, 0 = no bound.  trhip_gbuffer_render refuses a null list in words of its own before it asks.
inline int check_viewport_list(const char* fn, const uint32_t* viewports, uint32_t count, uint32_t layers, uint32_t camera_count) {
    if (!viewports) return set_error(std::string(fn) + ": null argument");
    if (layers && (count == 0 || count > layers))
        return set_error(std::string(fn) + ": " + std::to_string(count) + " viewports, the stage has " + std::to_string(layers) + " layers");
    for (uint32_t i = 0; i < count; ++i)
        if (viewports[i] >= camera_count) return set_error(std::string(fn) + ": viewport " + std::to_string(viewports[i]) + " out of range");
    return 0;
}

inline int check_scene_ready(const char* fn, size_t instance_count, bool accel_built) {
    if (instance_count == 0) return set_error(std::string(fn) + ": no scene (trhip_scene_upload)");
    if (!accel_built) return set_error(std::string(fn) + ": no acceleration structure: call trhip_scene_build_accel first");
    return 0;
}

// body(first, n, list) for every chunk of the list: List is what one launch takes in its arguments (ViewportList of first_hit.h),
// list.v[0 .. n) = viewports[first .. first + n).
template <class List, class Body>
void for_each_viewport_chunk(const uint32_t* viewports, uint32_t count, Body body) {
    constexpr uint32_t chunk = sizeof(List::v) / sizeof(List::v[0]);
    for (uint32_t first = 0; first < count; first += chunk) {
        const uint32_t n = count - first < chunk ? count - first : chunk;
        List list{};
        for (uint32_t i = 0; i < n; ++i) list.v[i] = viewports[first + i];
        body(first, n, list);
    }
}

}  // namespace tr
