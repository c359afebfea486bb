// gsr_reuse.hip -- geometry reuse: the forward of a call whose geometry and camera equal the previous call's
// (the second of SplaTAM's two Renderer calls) skips preprocess and the binning.  The kernels here copy the
// previous call's state with this call's colours and compare two calls' inputs bitwise; the C entry points
// (gsr_forward_reuse, gsr_forward_reuse_if_equal, gsr_bitwise_equal: gsr_capi.hip) decide and render.
#include "gsr_launch.h"
#include "gsr_layout.h"

namespace gsr {

// gsr_forward_reuse: the copied render records get this call's colours (preprocess writes the
// colours only for Gaussians that touch a tile: the same condition here, tiles[i] != 0)
__global__ void recolour_kernel(int P, const float* __restrict__ colors, float4* __restrict__ rr,
                                const uint32_t* __restrict__ tiles, Gate gate) {
    if (gate.off()) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P || tiles[i] == 0u) return;
    float4* q2 = rr + (size_t)RR_F4 * i + 2;
    const float4 old = *q2;
    *q2 = make_float4(colors[3 * i], colors[3 * i + 1], colors[3 * i + 2], old.w);
}
hipError_t launch_recolour(int P, const float* colors, GeomPtrs geo, hipStream_t s, Gate gate) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(recolour_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, colors, geo.rr, geo.tiles, gate);
    return hipGetLastError();
}
// gsr_forward_reuse_if_equal's copy of the previous call's state (runs only when the gate says "equal"): the
// geometry buffer up to its counters block plus counters[0..3] (num_rendered, prefiltered flag, longest list,
// sort cap: counters[4..7] stay this call's -- [5] holds the gate itself) and the radii; the render records'
// colour quarter (rr[i][2].xyz) of every Gaussian that touches a tile gets this call's colours on the way
// (recolour_kernel's condition and values, fused into the copy).  (The image and binning buffers are the
// previous call's, as in gsr_forward_reuse: the render writes the same final_T / n_contrib into them.)
// 16-B grid-stride streams (the geometry layout is 256-B aligned, the records at offset 0).
__global__ void __launch_bounds__(256) reuse_copy_kernel(Gate gate, const uint4* __restrict__ pg, uint4* __restrict__ g,
                                                         size_t ng16, const uint32_t* __restrict__ ptiles,
                                                         const float* __restrict__ colors, const int* __restrict__ prad,
                                                         int* __restrict__ rad, int P) {
    if (gate.off()) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nrr = (size_t)RR_F4 * P;
    for (size_t k = t0; k <= ng16; k += stride) {  // (k == ng16: counters[0..3])
        uint4 v = pg[k];
        if (k < nrr && (k % RR_F4) == 2) {
            const size_t i = k / RR_F4;
            if (ptiles[i] != 0u) {
                v.x = __float_as_uint(colors[3 * i]);
                v.y = __float_as_uint(colors[3 * i + 1]);
                v.z = __float_as_uint(colors[3 * i + 2]);
            }
        }
        g[k] = v;
    }
    for (size_t k = t0; k < (size_t)P; k += stride) rad[k] = prad[k];
}
hipError_t launch_reuse_copy(Gate gate, const void* prev_geom, void* geom, size_t geom_bytes, size_t tiles_offset,
                             const float* colors, const int* prev_radii, int* radii, int P, hipStream_t s) {
    if (geom_bytes & 15) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reuse_copy_kernel, dim3(2048), dim3(256), 0, s, gate, (const uint4*)prev_geom, (uint4*)geom,
                       geom_bytes / 16, (const uint32_t*)((const char*)prev_geom + tiles_offset), colors, prev_radii,
                       radii, P);
    return hipGetLastError();
}
// *word = e when a[k] and b[k] differ bitwise anywhere (16-B loads where both arrays allow them)
__global__ void __launch_bounds__(256) epoch_mismatch_kernel(EqualPairs q, uint32_t* word, uint32_t e) {
    bool diff = false;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    for (int k = 0; k < q.npairs; k++) {
        const float* a = q.a[k];
        const float* b = q.b[k];
        long long head = 0;
        if ((((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0)) {
            const uint4* a4 = reinterpret_cast<const uint4*>(a);
            const uint4* b4 = reinterpret_cast<const uint4*>(b);
            const long long n4 = q.n[k] / 4;
            for (long long i = t0; i < n4; i += stride) {
                const uint4 x = a4[i], y = b4[i];
                diff = diff || x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
            }
            head = 4 * n4;
        }
        const uint32_t* au = reinterpret_cast<const uint32_t*>(a);
        const uint32_t* bu = reinterpret_cast<const uint32_t*>(b);
        for (long long i = head + t0; i < q.n[k]; i += stride) diff = diff || au[i] != bu[i];
    }
    if (__ballot(diff) != 0ull && __lane_id() == 0) atomicExch(word, e);
}
hipError_t launch_epoch_mismatch(const EqualPairs& q, uint32_t* word, uint32_t e, hipStream_t s) {
    hipLaunchKernelGGL(epoch_mismatch_kernel, dim3(1024), dim3(256), 0, s, q, word, e);
    return hipGetLastError();
}
// flag |= 1 when a[k][i] != b[k][i] bitwise for any pair k (grid-stride over the pairs' elements)
__global__ void bitwise_equal_kernel(EqualPairs q, int* flag) {
    bool diff = false;
    for (int k = 0; k < q.npairs; k++) {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(q.a[k]);
        const uint32_t* b = reinterpret_cast<const uint32_t*>(q.b[k]);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < q.n[k];
             i += (long long)gridDim.x * blockDim.x)
            diff = diff || a[i] != b[i];
    }
    if (__ballot(diff) != 0ull && __lane_id() == 0) atomicOr(flag, 1);
}
hipError_t launch_bitwise_equal(const EqualPairs& q, int* flag, hipStream_t s) {
    if (q.npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(bitwise_equal_kernel, dim3(1024), dim3(256), 0, s, q, flag);
    return hipGetLastError();
}

}  // namespace gsr
