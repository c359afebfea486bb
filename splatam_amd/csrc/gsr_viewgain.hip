// gsr_viewgain.hip -- the silhouette half of the fork's mixed view gain (scripts/ros_handler.py:251-359,
// send_gains) on a finished forward's buffers (include/gsr_glue.h: gsr_silhouette_count): the number of
// pixels whose silhouette -- the forward's image of a colour channel whose per-Gaussian value is 1,
// SplaTAM's [z, 1, z^2] render, channel 1 -- is below a threshold, one unsigned word per image.
//
//   silhouette_count_kernel  one 256-thread workgroup per 16x16 tile.  The tile's list is already sorted
//                            and every entry the forward staged carries its 4x4-block mask (gsr_render_fwd.h
//                            fwd_tile), so there is no sort and no mask evaluation: the entries and the first
//                            half of their render records (q0, q1: 32 of the 64 bytes) are staged through LDS a
//                            batch at a time, the four 16-lane rows of a wave walk their compacted lists as
//                            the forward does, and only alpha, T and one accumulator are kept per pixel.
//
// Exactness: a pixel takes the forward's own decisions (eval_p2 without contraction, alpha = min(0.99,
// opacity * exp2(p2)), pairs with p2 > 0 or alpha < 1/255 skipped, the walk ends at T (1 - alpha) < 1e-4),
// its accumulator is C += alpha * T with the product and the sum each rounded (the forward's fma(1, w, C)),
// and the final value is C + T * bg[1] as fwd_epilogue forms it.
//
// Early exit: w = alpha * T > 0, so the rounded sums never decrease, and with bg[1] >= 0 neither does the
// background term lower the final value: once C >= sil_thres the pixel's final value is >= sil_thres
// whatever follows, it is not counted, and its walk ends there (at about half opacity for 0.5; the forward
// goes on to T < 1e-4).  A wave whose 64 pixels are all decided skips its lists; a tile ends when every
// pixel is.  With bg[1] < 0 (or NaN) the background term could lower the value again, so the kernel walks
// to the forward's own termination.  Either way a pixel is done no later than in the forward, so no batch
// is read that the forward did not stage (the entries of such batches carry no mask).
//
// Counting: a wave's ballot of the counted pixels, its popcount through LDS, one integer atomic per
// workgroup: the same word whatever the arrival order.
//
// The EIG half (compute_eig_score, :832-836) of one pose in one launch (include/gsr_glue.h: gsr_fisher_score):
//
//   fisher_score_kernel      at most FS_MAX_BLOCKS workgroups of 256 threads stride over the rows (a 300 k-row
//                            map is 10 MB of reads: the launch is bound by latency, not by bandwidth, so one
//                            workgroup per CU and a single arrival counter).  A row's four products are rounded
//                            to float32 (no contraction) and added to the thread's float64 sum in column order;
//                            a dead row is skipped, its values never enter an operation.  The workgroup's sum
//                            (lane tree, then the four waves) goes to the workspace; the last workgroup to arrive
//                            adds the partials in workgroup order and writes the score.  No float atomics: the
//                            same inputs give the same bits.
#include <stdint.h>

#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_errors.h"
#include "gsr_layout.h"
#include "gsr_math.h"
#include "gsr_wave.h"

namespace gsr {
namespace {

constexpr int VG_LS = RENDER_BATCH + 4;  // row-list stride (u16), as the forward's

__global__ void set_word_kernel(unsigned* __restrict__ p, unsigned v) { *p = v; }

__global__ void __launch_bounds__(TILE_PIX)
silhouette_count_kernel(Camera cam, const uint2* __restrict__ ranges, const PointEntry* __restrict__ point_list,
                        const float4* __restrict__ rr, BwdGuard guard, float thres, unsigned* __restrict__ count) {
    if (guard.overflow()) return;  // invalid forward state (static-mode overflow): the lists are not walked
    // entry RENDER_BATCH is a dummy (opacity 0, never blends) that pads the row lists
    __shared__ float4 s_a[RENDER_BATCH + 1];
    __shared__ float4 s_b[RENDER_BATCH + 1];
    __shared__ __attribute__((aligned(16))) uint16_t s_list[16 * VG_LS];
    __shared__ uint16_t s_mask[RENDER_BATCH];
    __shared__ uint32_t s_cnt[TILE_PIX / 64];
    const int tid = threadIdx.x, w = tid >> 6, row = (tid >> 4) & 3;
    const int tile = sched_tile(cam);
    if ((uint32_t)tile >= (uint32_t)(cam.gx * cam.gy)) return;  // (workgroup-uniform; a schedule is a permutation)
    const int tx = tile % cam.gx, ty = tile / cam.gx;
    const int px = tx * TILE_X + tile_px(tid);
    const int py = ty * TILE_Y + tile_py(tid);
    const bool inside = px < cam.W && py < cam.H;
    const v2f pix = v2f{(float)px, (float)py};
    const uint2 range = ranges[tile];
    const float bg1 = cam.bg[1];
    const bool early = bg1 >= 0.f;  // the background term cannot lower the value: a pixel is decided at C >= thres
    float T = 1.f, C = 0.f;
    bool done = !inside || (early && C >= thres);
    if (tid == 0) {
        s_a[RENDER_BATCH] = make_float4(0.f, 0.f, 0.f, 0.f);
        s_b[RENDER_BATCH] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // staging pipelined two deep, as the forward's: an entry is loaded a batch before its record
    PointEntry pe = 0, pen = 0;
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pb = pa;
    auto fetch_ent = [&](uint32_t s0) {
        if (s0 + tid < range.y) pen = point_list[s0 + tid];
    };
    auto fetch_rec = [&](uint32_t s0) {
        if (s0 + tid < range.y) {
            pe = pen;
            const float4* r = rr + (size_t)RR_F4 * pe_id(pe);
            pa = r[0];
            pb = r[1];
        }
    };
    fetch_ent(range.x);
    fetch_rec(range.x);
    fetch_ent(range.x + RENDER_BATCH);
    for (uint32_t start = range.x; start < range.y; start += RENDER_BATCH) {
        // (also the barrier between the last batch's walk and this batch's staging)
        if (__syncthreads_and(done)) break;
        const int cnt = (int)min((uint32_t)RENDER_BATCH, range.y - start);
        if (tid < cnt) {
            s_a[tid] = pa;
            s_b[tid] = pb;
            s_mask[tid] = (uint16_t)pe_mask(pe);
        }
        __syncthreads();
        fetch_rec(start + RENDER_BATCH);
        fetch_ent(start + 2 * RENDER_BATCH);
        if (__ballot(!done) == 0ull) continue;  // every pixel of this wave is decided: no lists, no walk
        const int jmin0[4] = {0, 0, 0, 0};
        static_assert(16 * RENDER_BATCH < 65536, "16-bit byte offsets");
        const int n = build_row_lists(s_mask, cnt, w, jmin0, s_list + 4 * w * VG_LS, VG_LS,
                                      (uint16_t)(16 * RENDER_BATCH), 16u);
        const uint16_t* my_list = s_list + (4 * w + row) * VG_LS;
        for (int i = 0; i < n; i += 4) {
            if (done) break;  // a decided lane leaves the walk; the wave's loop ends when every lane has
            int jb[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                jb[k] = (int)((const volatile __attribute__((address_space(3))) uint16_t*)my_list)[i + k];
            float alpha[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_a) + jb[k]);
                const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_b) + jb[k]);
                const float p2 = eval_p2(a, b, pix_delta(a, pix));
                alpha[k] = fminf(0.99f, b.y * __builtin_amdgcn_exp2f(p2));
                ok[k] = p2 <= 0.0f && alpha[k] >= 1.0f / 255.0f;  // the pad entry has alpha 0
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
#pragma clang fp contract(off)
                const bool okk = ok[k] && !done;
                const float test_T = T * (1.f - alpha[k]);
                const bool term = okk && test_T < 0.0001f;
                if (okk && !term) {
                    const float wgt = alpha[k] * T;
                    C = C + wgt;
                    T = test_T;
                }
                done = done || term || (early && C >= thres);
            }
        }
    }
    const float sil = C + T * bg1;  // fwd_epilogue's C1 + T * cam.bg[1]
    const uint64_t bal = __ballot(inside && sil < thres);
    if ((tid & 63) == 0) s_cnt[w] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (tid == 0) {
        const uint32_t n = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (n) atomicAdd(count, n);
    }
}

constexpr int FS_BLOCK = 256;
constexpr int FS_MAX_BLOCKS = 256;      // one workgroup per CU; each thread of the last one gathers one partial
constexpr size_t FS_HEAD_BYTES = 128;   // the arrival counter (word 0; zero between calls), nothing else

// Sums v over the workgroup in a fixed order (the wave's lane tree, then the four waves); every thread
// returns with the sum.
__device__ __forceinline__ double fs_block_sum(double v, double* s_red /*FS_BLOCK / 64*/) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();  // (an earlier call's readers are done with s_red)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ void __launch_bounds__(FS_BLOCK)
fisher_score_kernel(int P, const float* __restrict__ dmeans, const float* __restrict__ dopac,
                    const float4* __restrict__ hinv, const uint8_t* __restrict__ alive, uint32_t* counter,
                    double* part, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_red[FS_BLOCK / 64];
    const int tid = threadIdx.x;
    double acc = 0.;
    for (long long i = (long long)blockIdx.x * FS_BLOCK + tid; i < P; i += (long long)gridDim.x * FS_BLOCK) {
        if (alive != nullptr && alive[i] == 0) continue;  // selected out: a dead row's values are never read
        const float4 hi = hinv[i];
        const float h0 = dmeans[3 * i], h1 = dmeans[3 * i + 1], h2 = dmeans[3 * i + 2], h3 = dopac[i];
        const float p0 = h0 * hi.x, p1 = h1 * hi.y, p2 = h2 * hi.z, p3 = h3 * hi.w;
        acc += (double)p0;
        acc += (double)p1;
        acc += (double)p2;
        acc += (double)p3;
    }
    acc = fs_block_sum(acc, s_red);
    if (tid == 0) st_agent(part + blockIdx.x, acc);
    if (!last_block_arrive(counter)) return;
    const int nb = gridDim.x;  // <= FS_MAX_BLOCKS == FS_BLOCK: thread b holds workgroup b's partial
    acc = tid < nb ? ld_agent(part + tid) : 0.;
    acc = fs_block_sum(acc, s_red);
    if (tid == 0) *out = acc;
}

__global__ void set_double_kernel(double* __restrict__ p, double v) { *p = v; }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_silhouette_count(const gsr_settings* settings, int P, int num_rendered, const void* geom_buffer,
                         const void* binning_buffer, const void* image_buffer, float sil_thres, unsigned* count,
                         void* stream_) {
    if (!settings) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: null settings");
    if (!count) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: null count pointer");
    const int W = settings->image_width, H = settings->image_height;
    if (W <= 0 || H <= 0) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: image size must be positive");
    if (W > 16 * 65535 || H > 16 * 65535 || (unsigned long long)W * (unsigned long long)H > 0xFFFFFFFFull)
        return fail(GSR_ERR_INVALID_ARG, "silhouette_count: image too large (16-bit tile coordinates, 32-bit count)");
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: P must be >= 0");
    if (num_rendered < 0) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: num_rendered must be >= 0");
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e;
    if (P == 0) {
        // the forward of an empty map writes zero images and runs nothing (rasterize_points.cu:67-81):
        // every pixel's silhouette is 0
        hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(1), 0, stream, count,
                           0.f < sil_thres ? (unsigned)((unsigned long long)W * H) : 0u);
        e = hipGetLastError();
        return e == hipSuccess ? GSR_OK : hip_fail(e, "silhouette_count");
    }
    if (!geom_buffer || !image_buffer) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: missing forward state");
    if (num_rendered > 0 && !binning_buffer) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: missing binning buffer");
    if (!settings->bg) return fail(GSR_ERR_INVALID_ARG, "silhouette_count: bg missing");
    Camera cam{};
    cam.W = W;
    cam.H = H;
    cam.gx = (W + TILE_X - 1) / TILE_X;
    cam.gy = (H + TILE_Y - 1) / TILE_Y;
    cam.bg = settings->bg;
    const GeomLayout GL = GeomLayout::make(P);
    const ImgLayout IL = ImgLayout::make(W, H);
    const BinLayout BL = BinLayout::make(num_rendered, W, H);
    const GeomPtrs geo = GeomPtrs::at(const_cast<void*>(geom_buffer), GL);
    const char* ib = (const char*)image_buffer;
    // the forward's render schedule (a permutation of the tiles; any order gives the same count)
    cam.tile_order = (const uint32_t*)(ib + IL.order);
    const uint2* ranges = (const uint2*)(ib + IL.ranges);
    const PointEntry* point_list =
        binning_buffer ? (const PointEntry*)((const char*)binning_buffer + BL.point_list) : nullptr;
    hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(1), 0, stream, count, 0u);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "silhouette_count (zero)");
    hipLaunchKernelGGL(silhouette_count_kernel, dim3(cam.gx * cam.gy), dim3(TILE_PIX), 0, stream, cam, ranges,
                       point_list, geo.rr, BwdGuard{geo.counters, (uint32_t)num_rendered}, sil_thres, count);
    e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, "silhouette_count");
}

size_t gsr_fisher_score_workspace_bytes(void) { return FS_HEAD_BYTES + 8 * (size_t)FS_MAX_BLOCKS; }

int gsr_fisher_score(int P, const float* dmeans3D, const float* dopacity, const float* H_inv,
                     const unsigned char* alive, void* workspace, double* out, void* stream_) {
    static_assert(FS_MAX_BLOCKS <= FS_BLOCK, "the last workgroup gathers one partial per thread");
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "fisher_score: P must be >= 0");
    if (!out) return fail(GSR_ERR_INVALID_ARG, "fisher_score: null out pointer");
    if (((uintptr_t)out & 7u) != 0) return fail(GSR_ERR_INVALID_ARG, "fisher_score: out must be 8-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e;
    if (P == 0) {  // the empty sum (no pointer but out is read)
        hipLaunchKernelGGL(set_double_kernel, dim3(1), dim3(1), 0, stream, out, 0.0);
        e = hipGetLastError();
        return e == hipSuccess ? GSR_OK : hip_fail(e, "fisher_score");
    }
    if (!dmeans3D || !dopacity || !H_inv || !workspace) return fail(GSR_ERR_INVALID_ARG, "fisher_score: null pointer");
    if (((uintptr_t)H_inv & 15u) != 0 || ((uintptr_t)workspace & 15u) != 0)
        return fail(GSR_ERR_INVALID_ARG, "fisher_score: H_inv and workspace must be 16-byte aligned");
    const int need = (int)(((long long)P + FS_BLOCK - 1) / FS_BLOCK);
    const int nb = need < FS_MAX_BLOCKS ? need : FS_MAX_BLOCKS;
    hipLaunchKernelGGL(fisher_score_kernel, dim3(nb), dim3(FS_BLOCK), 0, stream, P, dmeans3D, dopacity,
                       (const float4*)H_inv, alive, (uint32_t*)workspace, (double*)((char*)workspace + FS_HEAD_BYTES),
                       out);
    e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, "fisher_score");
}

}  // extern "C"
