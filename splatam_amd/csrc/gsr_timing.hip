// gsr_timing.hip -- optional per-stage timing of the launches gsr_capi.hip brackets with a StageTimer
// (gsr_host.h): hipEvents on the launch stream, or device clocks accumulated by stamp kernels
// (graph-capturable); gsr_timing_enable / gsr_timing_read of include/gsr.h.
#include <mutex>
#include <vector>

#include "../../include/gsr.h"
#include "gsr_clock.h"
#include "gsr_errors.h"
#include "gsr_host.h"

namespace {
__global__ void stamp_begin_kernel(unsigned long long* c) { c[0] = wall_clock64(); }
__global__ void stamp_end_kernel(unsigned long long* c) {
    c[1] += wall_clock64() - c[0];
    c[2] += 1;
}
}  // namespace

namespace gsr {

struct Timing {
    bool on = false;
    // device-clock mode (graph-capturable): stamp kernels around the stages in `mask`
    // accumulate wall_clock64() ticks on the device: [start, sum, count, -] per stage
    bool clock = false;
    unsigned mask = 0;
    unsigned long long* dclock = nullptr;
    std::vector<TimedRec> recs;
    std::vector<hipEvent_t> pool;
    double ms[GSR_NUM_STAGES] = {};
    long long launches[GSR_NUM_STAGES] = {};
    long long units[GSR_NUM_STAGES] = {};
    ~Timing() {
        for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
    hipEvent_t take() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};

namespace {

// Per device, not thread-local: torch runs autograd backward on its own thread.
Timing g_timing[kMaxDevices];
std::mutex g_timing_mu;

size_t kclock_bytes() { return (size_t)KCLOCK_WORDS * sizeof(unsigned long long) * GSR_NUM_STAGES; }

// Inside a stream capture an event record is only an internal dependency unless
// it is external: then it becomes a graph node re-recorded at every replay, so the
// stage times read after replays are those of the last replay.
hipError_t record_event(hipEvent_t e, hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive)
        return hipEventRecordWithFlags(e, s, hipEventRecordExternal);
    return hipEventRecord(e, s);
}

void timing_drain(Timing& T) {  // caller holds g_timing_mu
    for (auto& r : T.recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            T.ms[r.stage] += ms;
            T.launches[r.stage] += 1;
            T.units[r.stage] += r.units;
        }
        T.pool.push_back(r.a);
        T.pool.push_back(r.b);
    }
    T.recs.clear();
    (void)hipGetLastError();  // an event that was never recorded must not leave a sticky error for torch
}

}  // namespace

StageTimer::StageTimer(int stage, long long units, hipStream_t s_, bool in_kernel)
    : s(s_), on(false), T(g_timing[stream_device(s_)]) {
    on = T.on;
    if (!on) return;
    if (T.clock) {
        on = false;
        if ((T.mask >> stage) & 1u) {
            if (in_kernel) {
                kc = T.dclock + (size_t)KCLOCK_WORDS * stage;
            } else {
                dc = T.dclock + (size_t)KCLOCK_WORDS * stage;
                hipLaunchKernelGGL(stamp_begin_kernel, dim3(1), dim3(1), 0, s, dc);
            }
        }
        return;
    }
    rec.stage = stage; rec.units = units;
    {
        std::lock_guard<std::mutex> lk(g_timing_mu);
        rec.a = T.take(); rec.b = T.take();
    }
    (void)record_event(rec.a, s);
}

StageTimer::~StageTimer() {
    if (dc) hipLaunchKernelGGL(stamp_end_kernel, dim3(1), dim3(1), 0, s, dc);
    if (!on) return;
    (void)record_event(rec.b, s);
    std::lock_guard<std::mutex> lk(g_timing_mu);
    T.recs.push_back(rec);
}

void g_timing_units(int dev, int stage, long long units) {
    std::lock_guard<std::mutex> lk(g_timing_mu);
    Timing& T = g_timing[dev];
    for (auto it = T.recs.rbegin(); it != T.recs.rend(); ++it)
        if (it->stage == stage) { it->units = units; break; }
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_timing_enable(int on) {
    std::lock_guard<std::mutex> lk(g_timing_mu);
    Timing& T = g_timing[current_device()];
    timing_drain(T);
    T.on = on != 0;
    T.clock = on >= GSR_TIMING_CLOCK;
    T.mask = (unsigned)on & 0xFFu;
    for (int i = 0; i < GSR_NUM_STAGES; i++) { T.ms[i] = 0.0; T.launches[i] = 0; T.units[i] = 0; }
    if (T.clock) {
        hipError_t e;
        if (!T.dclock && (e = hipMalloc((void**)&T.dclock, kclock_bytes())) != hipSuccess)
            return hip_fail(e, "timing clock buffer");
        if ((e = hipMemset(T.dclock, 0, kclock_bytes())) != hipSuccess) return hip_fail(e, "timing clock reset");
    }
    return GSR_OK;
}

int gsr_timing_read(double* ms, long long* launches, long long* units, int n) {
    std::lock_guard<std::mutex> lk(g_timing_mu);
    Timing& T = g_timing[current_device()];
    timing_drain(T);
    if (T.clock && T.dclock) {
        std::vector<unsigned long long> h((size_t)KCLOCK_WORDS * GSR_NUM_STAGES);
        int dev = 0, khz = 0;
        hipError_t e;
        if ((e = hipMemcpy(h.data(), T.dclock, kclock_bytes(), hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail(e, "timing clock read");
        if ((e = hipGetDevice(&dev)) != hipSuccess ||
            (e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev)) != hipSuccess || khz <= 0)
            return fail(GSR_ERR_HIP, "wall clock rate unavailable");
        for (int i = 0; i < GSR_NUM_STAGES; i++) {
            T.ms[i] = (double)h[(size_t)KCLOCK_WORDS * i + 1] / (double)khz;
            T.launches[i] = (long long)h[(size_t)KCLOCK_WORDS * i + 2];
        }
    }
    for (int i = 0; i < n && i < GSR_NUM_STAGES; i++) {
        if (ms) ms[i] = T.ms[i];
        if (launches) launches[i] = T.launches[i];
        if (units) units[i] = T.units[i];
    }
    return GSR_NUM_STAGES;
}

}  // extern "C"
