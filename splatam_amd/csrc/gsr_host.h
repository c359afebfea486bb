// gsr_host.h -- host-only helpers of the C entry points: shared by gsr_capi.hip (orchestration) and
// gsr_timing.hip (stage timing), included by nothing else.
#pragma once
#include "gsr_layout.h"

namespace gsr {

// Host-side state is kept per device (the device of the launch stream), so one process (or one
// thread) may serve several GPUs: the pinned counter staging + its event (per thread and device),
// the binning-capacity hint (per device) and the stage timing (per device).
constexpr int kMaxDevices = 64;
int stream_device(hipStream_t s);
int current_device();
int device_cus(int dev);  // CU count (render schedule round size), cached per device

// zero-fill as a kernel (a memset node in a captured graph was not re-executed on replay)
hipError_t zero_async(void* p, size_t bytes, hipStream_t s);

struct Timing;
struct TimedRec {
    int stage;
    long long units;
    hipEvent_t a, b;
};
struct StageTimer {  // brackets the launches of one stage
    TimedRec rec{};
    hipStream_t s;
    bool on;
    unsigned long long* dc = nullptr;
    unsigned long long* kc = nullptr;  // in-kernel clock slot (stages whose kernel stamps itself)
    // in_kernel: the stage is one launch that takes kclock() and stamps itself
    // (kclock_begin / kclock_end), so no stamp kernels are added around it
    Timing& T;
    StageTimer(int stage, long long units, hipStream_t s_, bool in_kernel = false);
    unsigned long long* kclock() const { return kc; }
    ~StageTimer();
};
// The speculative launches learn their work units only after the host sync.
void g_timing_units(int dev, int stage, long long units);

struct ImgPtrs {
    float* final_T;
    uint32_t* n_contrib;
    uint2* ranges;
    uint32_t* tile_count;
    uint32_t* order;
    uint32_t* rowmax;
    static ImgPtrs at(void* image_buffer, const ImgLayout& L) {
        char* b = (char*)image_buffer;
        return {(float*)(b + L.final_T), (uint32_t*)(b + L.n_contrib), (uint2*)(b + L.ranges),
                (uint32_t*)(b + L.tile_count), (uint32_t*)(b + L.order), (uint32_t*)(b + L.rowmax)};
    }
};

struct BinPtrs {
    uint64_t* point_list;
    uint64_t* keys[2];
    uint32_t* vals[2];
    uint32_t* gid;
    uint32_t* hist;
    static BinPtrs at(void* binning_buffer, const BinLayout& L) {
        char* b = (char*)binning_buffer;
        return {(uint64_t*)(b + L.point_list), {(uint64_t*)(b + L.keys[0]), (uint64_t*)(b + L.keys[1])},
                {(uint32_t*)(b + L.vals[0]), (uint32_t*)(b + L.vals[1])}, (uint32_t*)(b + L.gid),
                (uint32_t*)(b + L.hist)};
    }
};

// the render schedule of an image buffer (a permutation of the tiles: tile_plan in the bucketed duplicate,
// else row-major; any order gives the same results) and the device's round size, bound into a launch's camera
inline void bind_schedule(Camera& cam, const ImgPtrs& img, int dev) {
    cam.tile_order = img.order;
    cam.rowmax = img.rowmax;
    cam.sched_cus = device_cus(dev);  // (wave priority levels: one or several dispatch rounds)
}

}  // namespace gsr
