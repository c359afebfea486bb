// gsr_seq_common.h -- device helpers shared by the SLAM sequence steps (gsr_keyframe.hip,
// gsr_densify.hip), all for workgroups of SEQ_BLOCK threads: the inclusive scan, the last
// workgroup's exclusive scan of per-workgroup counts, the workgroup count from wave popcounts and
// the back-projection of a pixel through the rigid inverse of w2c.
#pragma once
#include "gsr_wave.h"

namespace gsr {
namespace {

constexpr int SEQ_BLOCK = 256;
constexpr int SEQ_WAVES = SEQ_BLOCK / 64;

// Inclusive scan (Hillis-Steele) of one value per thread, every thread calling.  s_scan: SEQ_BLOCK
// words, holding the result on return (the last thread's is the total).
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* s_scan) {
    const int tid = threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < SEQ_BLOCK; d <<= 1) {
        const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    return s_scan[tid];
}

// The last workgroup's exclusive scan of n counts published with st_agent: thread t owns
// [t * per, (t + 1) * per) clamped to n, per = ceil(n / SEQ_BLOCK) (the trailing threads own
// nothing).  Writes excl[0 .. n); the last thread returns the total.
__device__ __forceinline__ uint32_t last_block_scan_excl(const uint32_t* cnt, int n, uint32_t* excl,
                                                         uint32_t* s_scan) {
    const int per = (n + SEQ_BLOCK - 1) / SEQ_BLOCK;
    const int i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
    uint32_t sum = 0;
    for (int i = i0; i < i1; i++) sum += ld_agent(cnt + i);
    const uint32_t incl = block_scan_incl(sum, s_scan);
    uint32_t run = incl - sum;
    for (int i = i0; i < i1; i++) {
        excl[i] = run;
        run += ld_agent(cnt + i);
    }
    return incl;
}

// The workgroup's count, the sum of its waves' (wave-uniform: each lane holds its wave's ballot
// popcounts), published to *dst with st_agent.  s_wave: SEQ_WAVES words.
__device__ __forceinline__ void block_count_publish(uint32_t wave_count, uint32_t* s_wave, uint32_t* dst) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) s_wave[tid >> 6] = wave_count;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (int w = 0; w < SEQ_WAVES; w++) total += s_wave[w];
        st_agent(dst, total);
    }
}

// The rigid inverse [R^T, -R^T t] of w2c (row-major, 12 floats read) and the world point of pixel
// (col, row) at depth z through it: every operation rounded on its own, every sum left to right --
// the order include/gsr_glue.h states (gsr_keyframe_select step 2, gsr_densify_frame).  A kernel
// with a pixel loop forms the inverse once, before the loop.
struct RigidInverse {
    float r[3][3], t[3];
};
__device__ __forceinline__ RigidInverse rigid_inverse(const float* w2c) {
#pragma clang fp contract(off)
    RigidInverse c;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c.r[a][0] = w2c[a]; c.r[a][1] = w2c[4 + a]; c.r[a][2] = w2c[8 + a];
        c.t[a] = -(c.r[a][0] * w2c[3] + c.r[a][1] * w2c[7] + c.r[a][2] * w2c[11]);
    }
    return c;
}
__device__ __forceinline__ float3 backproject(int col, int row, float z, float fx, float fy, float cx, float cy,
                                              const RigidInverse& c) {
#pragma clang fp contract(off)
    const float x = ((float)col - cx) / fx * z;
    const float y = ((float)row - cy) / fy * z;
    return make_float3(c.r[0][0] * x + c.r[0][1] * y + c.r[0][2] * z + c.t[0],
                       c.r[1][0] * x + c.r[1][1] * y + c.r[1][2] * z + c.t[1],
                       c.r[2][0] * x + c.r[2][1] * y + c.r[2][2] * z + c.t[2]);
}

}  // namespace
}  // namespace gsr
