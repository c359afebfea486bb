// gsr_clock.h -- the in-kernel stage clock (kclock_begin / kclock_end) and the GSR_WGTIME per-workgroup
// timeline macros that gsr_diag.h expands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

// In-kernel device-clock timing of one launch (graph-capturable, no extra
// kernels): clk = [start, sum of durations, launches, groups done, then 16 group
// counters KCLOCK_GROUP_STRIDE words apart].  The first workgroup stamps the
// start; workgroups count themselves done in 16 counters on separate cache lines
// (one counter for all 1200 workgroups serialised ~10 us of same-address
// atomics at the end of the launch), the last of each group counts the group,
// and the last group adds (now - start) and resets the counters for the next
// launch.  wall_clock64 runs at 100 MHz.
constexpr int KCLOCK_GROUP_STRIDE = 32;  // u64 words (256 B)
constexpr int KCLOCK_WORDS = 4 + 16 * KCLOCK_GROUP_STRIDE;
// Diagnostics build only (-DGSR_WGTIME=1, tools/wgtime.py; never in libgsr.so): every render
// workgroup records [start, end, HW_ID, XCC_ID] in its translation unit's g_wgtime table.
#ifndef GSR_WGTIME
#define GSR_WGTIME 0
#endif
#define GSR_WGTIME_MAX 16384
#if GSR_WGTIME
#define GSR_WGTIME_TABLE static __device__ unsigned long long g_wgtime[GSR_WGTIME_MAX][4];
#define GSR_WGTIME_MARK(end_)                                                                              \
    do {                                                                                                   \
        if (end_) __syncthreads();                                                                         \
        const unsigned b_ = blockIdx.y * gridDim.x + blockIdx.x;                                           \
        if (threadIdx.x == 0 && b_ < GSR_WGTIME_MAX) {                                                     \
            g_wgtime[b_][(end_) ? 1 : 0] = wall_clock64();                                                 \
            if (!(end_)) {                                                                                 \
                g_wgtime[b_][2] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);                     \
                g_wgtime[b_][3] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);                    \
            }                                                                                              \
        }                                                                                                  \
    } while (0)
#else
#define GSR_WGTIME_TABLE
#define GSR_WGTIME_MARK(end_) do {} while (0)
#endif

__device__ __forceinline__ void kclock_begin(unsigned long long* clk) {
    if (clk && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        __hip_atomic_store(&clk[0], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Relaxed agent-scope atomics throughout: a release/acquire fence per workgroup
// costs an L2 writeback each on this multi-XCD part (~4% of the tracking step).
// Only workgroup 0 (the one that stamped the start) releases, and only the last
// one acquires.
__device__ __forceinline__ void kclock_end(unsigned long long* clk) {  // every thread of the block calls this
    if (!clk) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned nb = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x, g = b & 15u;
        const unsigned ngroups = nb < 16u ? nb : 16u;
        const unsigned gsize = nb / 16u + (g < nb % 16u ? 1u : 0u);
        unsigned long long* gc = clk + 4 + g * KCLOCK_GROUP_STRIDE;
        if (b == 0) __atomic_thread_fence(__ATOMIC_RELEASE);
        if (__hip_atomic_fetch_add(gc, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1) {
            __hip_atomic_store(gc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(&clk[3], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1) {
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                const unsigned long long t0 = __hip_atomic_load(&clk[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                clk[1] += wall_clock64() - t0;
                clk[2] += 1;
                __hip_atomic_store(&clk[3], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

}  // namespace gsr
