// gsr_keyframe.hip -- SplaTAM's overlap keyframe selection (utils/keyframe_selection.py,
// scripts/splatam.py:820-837) on the device, without a host read (include/gsr_glue.h:
// gsr_keyframe_select).  Three launches on the caller's stream:
//
//   kf_rows_kernel     one workgroup per image row counts its pixels with depth > 0 (ballot +
//                      popcount); the last workgroup to arrive scans the H counts into the
//                      exclusive row prefix and n_valid.
//   kf_sample_kernel   one wave per sample: rank r = (u_pix * n_valid) >> 32, the duplicate
//                      test against the other samples' ranks (recomputed from their words), a
//                      binary search over the row prefix, a ballot / popcount walk along the row
//                      to the pixel of that rank, the back-projection and the origin test.
//   kf_select_kernel   one workgroup per candidate keyframe projects the kept points and counts
//                      the ones inside; the last workgroup to arrive counts n_points, orders the
//                      eligible keyframes by (perm_key, index), writes the window and the draws.
//
// Latency-bound work (a 640x480 depth image, 1600 samples, tens of keyframes): the aim is few
// launches.  All counts are integers (LDS integer adds, agent-scope arrival counters); no float
// is ever accumulated, so the results do not depend on the arrival order.  Every float operation
// is rounded on its own (no contraction) in the order include/gsr_glue.h states, so
// splatam_amd.keyframes.select_literal's elementwise torch ops form the same bits.
#include <math.h>

#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_errors.h"
#include "gsr_layout.h"
#include "gsr_seq_common.h"
#include "gsr_wave.h"

namespace gsr {
namespace {

constexpr int KF_BLOCK = SEQ_BLOCK;
constexpr int KF_WAVES = SEQ_WAVES;
constexpr int KF_MAX_ROWS = 4096;     // the row scan's LDS prefix
constexpr int KF_MAX_WINDOW = 1024;   // k_select + 2 (the window's LDS copy)
// workspace words: [0] kf_rows_kernel's arrival counter, [1] kf_select_kernel's (both zero between
// calls), [KF_NVALID] n_valid, then rowcnt [H], rowpre [H + 1] and the samples' float4 points
constexpr int KF_NVALID = 16;
constexpr int KF_HEAD_WORDS = 32;

struct KfLayout {
    size_t rowcnt, rowpre, pts, total;  // 32-bit word offsets; total in bytes
    __host__ __device__ static KfLayout make(int H, int S) {
        KfLayout l;
        l.rowcnt = KF_HEAD_WORDS;
        l.rowpre = l.rowcnt + (size_t)H;
        l.pts = align_up(l.rowpre + (size_t)H + 1, 4);
        l.total = 4 * (l.pts + 4 * (size_t)S);
        return l;
    }
};

struct KfCam {
    float fx, fy, cx, cy;
};

__device__ __forceinline__ uint32_t kf_rank(uint32_t word, uint32_t n) {
    return (uint32_t)(((uint64_t)word * (uint64_t)n) >> 32);
}

__global__ void __launch_bounds__(KF_BLOCK)
kf_rows_kernel(int H, int W, const float* __restrict__ depth, uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_wave[KF_WAVES];
    __shared__ uint32_t s_scan[KF_BLOCK];
    const KfLayout lay = KfLayout::make(H, 0);
    uint32_t* const rowcnt = ws + lay.rowcnt;
    uint32_t* const rowpre = ws + lay.rowpre;
    const int row = blockIdx.x, tid = threadIdx.x;
    uint32_t cnt = 0;  // (wave-uniform: every lane adds the wave's popcount)
    for (int c0 = 0; c0 < W; c0 += KF_BLOCK) {
        const int c = c0 + tid;
        const bool v = c < W && depth[(size_t)row * W + c] > 0.f;
        cnt += (uint32_t)__popcll(__ballot(v));
    }
    block_count_publish(cnt, s_wave, rowcnt + row);
    if (!last_block_arrive(ws + 0)) return;
    // last workgroup: the exclusive scan of the H row counts
    const uint32_t total = last_block_scan_excl(rowcnt, H, rowpre, s_scan);
    if (tid == KF_BLOCK - 1) {
        rowpre[H] = total;
        ws[KF_NVALID] = total;
    }
}

__global__ void __launch_bounds__(KF_BLOCK)
kf_sample_kernel(int H, int W, const float* __restrict__ depth, KfCam cam, const float* __restrict__ w2c, int S,
                 const uint32_t* __restrict__ u_pix, const uint32_t* __restrict__ ws, float4* __restrict__ pts,
                 int* __restrict__ sampled) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);
    if (j >= S) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const KfLayout lay = KfLayout::make(H, S);
    const uint32_t* const rowpre = ws + lay.rowpre;
    const uint32_t n_valid = ws[KF_NVALID];
    int pix = -1;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n_valid > 0) {
        const uint32_t r = kf_rank(u_pix[j], n_valid);
        bool dup = false;
        for (int i0 = 0; i0 < S; i0 += 64) {
            const int i = i0 + lane;
            dup = dup || (i < S && i != j && kf_rank(u_pix[i], n_valid) == r);
        }
        const bool drawn_twice = __ballot(dup) != 0ull;
        int lo = 0, hi = H;  // rowpre[lo] <= r < rowpre[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rowpre[mid] <= r) lo = mid; else hi = mid;
        }
        uint32_t k = r - rowpre[lo];
        int col = -1;
        for (int c0 = 0; c0 < W; c0 += 64) {
            const int c = c0 + lane;
            const bool v = c < W && depth[(size_t)lo * W + c] > 0.f;
            const unsigned long long m = __ballot(v);
            const uint32_t n = (uint32_t)__popcll(m);
            if (k < n) {
                const bool hit = v && (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) == k;
                col = c0 + __ffsll((long long)__ballot(hit)) - 1;
                break;
            }
            k -= n;
        }
        if (col >= 0 && col < W) {
            pix = lo * W + col;
            const float3 w = backproject(col, lo, depth[pix], cam.fx, cam.fy, cam.cx, cam.cy,
                                          rigid_inverse(w2c));
            const bool origin = rintf(w.x * 10000.f) == 0.f && rintf(w.y * 10000.f) == 0.f &&
                                rintf(w.z * 10000.f) == 0.f;
            out = make_float4(w.x, w.y, w.z, (!drawn_twice && !origin) ? 1.f : 0.f);
        }
    }
    if (lane == 0) {
        pts[j] = out;
        if (sampled) sampled[j] = pix;
    }
}

__global__ void __launch_bounds__(KF_BLOCK)
kf_select_kernel(int H, int W, KfCam cam, const float* __restrict__ kf_w2c, int n_kf, int k_select, int S,
                 const float4* __restrict__ pts, const uint32_t* __restrict__ perm_key, int n_draws,
                 const uint32_t* __restrict__ u_draw, const long long* __restrict__ kf_time, long long time_idx,
                 int cur_row, uint32_t* __restrict__ ws, uint32_t* overlap, int* __restrict__ n_points,
                 int* __restrict__ window, int* __restrict__ n_window, long long* __restrict__ draw_rows,
                 long long* __restrict__ draw_times) {
#pragma clang fp contract(off)
    __shared__ int s_cnt, s_elig, s_nwin;
    __shared__ uint32_t s_key[KF_BLOCK];
    __shared__ uint32_t s_ov[KF_BLOCK];
    __shared__ int s_win[KF_MAX_WINDOW];
    const int tid = threadIdx.x;
    const int n_cand = n_kf > 0 ? n_kf - 1 : 0;  // every keyframe but the last
    const int k = blockIdx.x;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (k < n_cand) {
        float m[12];
#pragma unroll
        for (int a = 0; a < 12; a++) m[a] = kf_w2c[16 * (size_t)k + a];
        const float umax = (float)(W - 20), vmax = (float)(H - 20);
        int cnt = 0;
        for (int j = tid; j < S; j += KF_BLOCK) {
            const float4 p = pts[j];
            if (p.w == 0.f) continue;
            const float px = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
            const float py = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
            const float pz = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
            const float zz = pz + 1e-5f;
            const float u = (cam.fx * px + cam.cx * pz) / zz;
            const float v = (cam.fy * py + cam.cy * pz) / zz;
            cnt += (u > 20.f && u < umax && v > 20.f && v < vmax && zz > 0.f) ? 1 : 0;
        }
        if (cnt) atomicAdd(&s_cnt, cnt);  // (LDS, integer)
        __syncthreads();
        if (tid == 0) st_agent(overlap + k, (uint32_t)s_cnt);
    }
    if (!last_block_arrive(ws + 1)) return;
    // ---- last workgroup: n_points, the window, the draws
    if (tid == 0) { s_cnt = 0; s_elig = 0; }
    for (int i = tid; i < KF_MAX_WINDOW; i += KF_BLOCK) s_win[i] = -1;
    __syncthreads();
    {
        int kept = 0;
        for (int j = tid; j < S; j += KF_BLOCK) kept += pts[j].w != 0.f ? 1 : 0;
        if (kept) atomicAdd(&s_cnt, kept);
    }
    // rank of every eligible candidate among the eligible ones, ordered by (perm_key, index): candidate
    // i = q * 256 + tid against tiles of 256 candidates staged in LDS
    for (int q0 = 0; q0 < n_cand; q0 += KF_BLOCK) {
        const int i = q0 + tid;
        const bool mine = i < n_cand && ld_agent(overlap + i) > 0u;
        const uint32_t key = i < n_cand ? perm_key[i] : 0u;
        int rank = 0;
        for (int t0 = 0; t0 < n_cand; t0 += KF_BLOCK) {
            const int j = t0 + tid;
            __syncthreads();
            s_key[tid] = j < n_cand ? perm_key[j] : 0u;
            s_ov[tid] = j < n_cand ? ld_agent(overlap + j) : 0u;
            __syncthreads();
            const int nt = min(KF_BLOCK, n_cand - t0);
            if (mine)
                for (int e = 0; e < nt; e++)
                    rank += (s_ov[e] > 0u && (s_key[e] < key || (s_key[e] == key && t0 + e < i))) ? 1 : 0;
        }
        if (mine) {
            atomicAdd(&s_elig, 1);
            if (rank < k_select) s_win[rank] = i;  // (ranks are distinct: one writer per slot)
        }
    }
    __syncthreads();
    if (tid == 0) {
        int n = min(k_select, s_elig);
        if (n_kf > 0) s_win[n++] = n_kf - 1;
        s_win[n++] = cur_row;
        s_nwin = n;
        n_window[0] = n;
        n_points[0] = s_cnt;
    }
    __syncthreads();
    const int nw = s_nwin;
    for (int i = tid; i < k_select + 2; i += KF_BLOCK) window[i] = s_win[i];
    for (int i = tid; i < n_draws; i += KF_BLOCK) {
        const int w = s_win[kf_rank(u_draw[i], (uint32_t)nw)];
        draw_rows[i] = w;
        draw_times[i] = w == cur_row ? time_idx : kf_time[w];
    }
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_keyframe_workspace_bytes(int H, int S) {
    if (H < 0 || S < 0) return 0;
    return KfLayout::make(H, S).total;
}

int gsr_keyframe_select(int H, int W, const float* depth, float fx, float fy, float cx, float cy, const float* w2c,
                        const float* kf_w2c, int n_kf, int k_select, int S, const unsigned* u_pix,
                        const unsigned* perm_key, int n_draws, const unsigned* u_draw, const long long* kf_time,
                        long long time_idx, int cur_row, void* workspace, int* overlap, int* n_points, int* window,
                        int* n_window, long long* draw_rows, long long* draw_times, int* sampled_pixels,
                        void* stream) {
    if (!image_size_ok(H, W) || H > KF_MAX_ROWS)
        return fail(GSR_ERR_INVALID_ARG, "keyframe_select: bad image size (at most 4096 rows)");
    if (n_kf < 0 || k_select < 0 || k_select + 2 > KF_MAX_WINDOW || S < 0 || n_draws < 0 || cur_row < n_kf)
        return fail(GSR_ERR_INVALID_ARG, "keyframe_select: bad sizes (k_select <= 1022, cur_row >= n_kf)");
    if (!depth || !w2c || !workspace || !n_points || !window || !n_window || (S > 0 && !u_pix) ||
        (n_kf > 0 && (!kf_w2c || !kf_time)) || (n_kf > 1 && (!perm_key || !overlap)) ||
        (n_draws > 0 && (!u_draw || !draw_rows || !draw_times)))
        return fail(GSR_ERR_INVALID_ARG, "keyframe_select: null pointer");
    if (!aligned16(workspace)) return fail(GSR_ERR_INVALID_ARG, "keyframe_select: workspace must be 16-byte aligned");
    const KfLayout lay = KfLayout::make(H, S);
    uint32_t* const ws = (uint32_t*)workspace;
    float4* const pts = (float4*)(ws + lay.pts);
    const KfCam cam{fx, fy, cx, cy};
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kf_rows_kernel, dim3(H), dim3(KF_BLOCK), 0, st, H, W, depth, ws);
    if (S > 0)
        hipLaunchKernelGGL(kf_sample_kernel, dim3((S + KF_WAVES - 1) / KF_WAVES), dim3(KF_BLOCK), 0, st, H, W, depth,
                           cam, w2c, S, u_pix, ws, pts, sampled_pixels);
    hipLaunchKernelGGL(kf_select_kernel, dim3(n_kf > 1 ? n_kf - 1 : 1), dim3(KF_BLOCK), 0, st, H, W, cam, kf_w2c, n_kf,
                       k_select, S, pts, perm_key, n_draws, u_draw, kf_time, time_idx, cur_row, ws,
                       (uint32_t*)overlap, n_points, window, n_window, draw_rows, draw_times);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, "keyframe_select");
}

}  // extern "C"
