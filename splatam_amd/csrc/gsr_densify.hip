// gsr_densify.hip -- SplaTAM's add_new_gaussians (scripts/splatam.py:384-426) on a capacity-padded
// map, on the device, without a host read (include/gsr_glue.h: gsr_densify_frame).  Six launches
// on the caller's stream:
//
//   dn_zero_kernel      the three selection histograms (a kernel, not a memset node: a captured call
//                       must zero them on every replay)
//   dn_select_kernel x3 the lower median of err by selection on its bit patterns: pass p builds the
//                       histogram of one 11 / 11 / 10-bit digit (most significant first) over the
//                       pixels whose higher digits equal the ones already chosen -- LDS integer adds,
//                       the non-zero bins flushed with global integer adds -- and the last workgroup
//                       to arrive walks the 2048 bins to the one that holds the wanted rank.
//   dn_count_kernel     the selection mask (one ballot word per 64 pixels) and a count per
//                       workgroup; the last workgroup to arrive scans the counts (exclusive), reads
//                       the old n_live, and writes n_added, the new n_live and overflow.
//   dn_scatter_kernel   row = old n_live + workgroup prefix + the popcount rank inside the workgroup;
//                       the selected pixels' Gaussians, alive, dest.
//
// gsr_densify_frame_capped is the same six launches with the realtime loop's threshold
// (median_thr / median_scale, scripts/splatam_realtime.py:444-453), decided where dn_count_kernel
// already reads the median.  gsr_init_frame (initialize_first_timestep's point cloud, :229-237) is the
// last two launches alone: dn_count_kernel<true> selects every pixel with a measured depth and reads
// neither depth_sil nor the median, dn_scatter_kernel is the same kernel.
//
// Latency-bound work (640x480: 307 k pixels, 150 workgroups of 2048 pixels): the aim is few launches
// and no wasted bytes -- err is recomputed from the two depth images in every pass (2.4 MB, cache
// resident) rather than stored, only selected pixels write anything but dest.  All counts are
// integers; no float is accumulated and nothing is sorted, so the results do not depend on the
// arrival order.  Every float operation is rounded on its own (no contraction) in the order
// include/gsr_glue.h states, so splatam_amd.densify.densify_literal's elementwise torch ops form the
// same bits (log_scales up to logf's rounding).
//
// One value shared by most of the image (err == 0 wherever the map explains the frame) would put
// every lane of every wave on one LDS word: dn_hist_add first counts, with two ballots, the lanes
// that share the first active lane's bin and adds them at once (twice), then the rest one by one.
#include <math.h>

#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_errors.h"
#include "gsr_layout.h"
#include "gsr_seq_common.h"
#include "gsr_wave.h"

namespace gsr {
namespace {

constexpr int DN_BLOCK = SEQ_BLOCK;
constexpr int DN_WAVES = SEQ_WAVES;
constexpr int DN_ITEMS = 8;                       // pixels per thread
constexpr int DN_TILE = DN_BLOCK * DN_ITEMS;      // pixels per workgroup
constexpr int DN_CHUNKS = DN_TILE / 64;           // ballot words per workgroup
constexpr int DN_BINS = 2048;                     // 11-bit digits (the last one 10 bits: the upper half stays 0)
// workspace words: [0 .. 2] dn_select_kernel's arrival counters, one per pass, [3] dn_count_kernel's
// (all zero between calls); then the values one kernel hands to the next
constexpr int DN_PREFIX = 16;   // [2]: the digits chosen by pass 0, by passes 0 and 1
constexpr int DN_RANK = 18;     // [2]: the wanted rank inside that prefix
constexpr int DN_MED = 20;      // the median's bits
constexpr int DN_NAN = 21;      // != 0: some err is NaN
constexpr int DN_BASE = 22;     // [2]: the old n_live (int64, 8-byte aligned)
constexpr int DN_HEAD_WORDS = 32;
constexpr uint32_t DN_QNAN = 0x7fc00000u;

struct DnLayout {
    size_t hist, cnt, excl, mask, total;  // 32-bit word offsets; total in bytes
    int nb;                               // workgroups
    __host__ __device__ static DnLayout make(long long N) {
        DnLayout l;
        l.nb = (int)((N + DN_TILE - 1) / DN_TILE);
        l.hist = DN_HEAD_WORDS;
        l.cnt = l.hist + 3 * (size_t)DN_BINS;
        l.excl = l.cnt + (size_t)l.nb;
        l.mask = align_up(l.excl + (size_t)l.nb, 2);
        l.total = 4 * (l.mask + 2 * (size_t)DN_CHUNKS * (size_t)l.nb);
        return l;
    }
};

struct DnCam {
    float fx, fy, cx, cy, f;  // f: the mean focal length
};

// err's bit pattern as the selection key: non-negative floats order as unsigned integers; every NaN
// (whatever its sign) becomes the largest key, in the top bin of pass 0
__device__ __forceinline__ uint32_t dn_key(float gt, float rd) {
#pragma clang fp contract(off)
    const float valid = gt > 0.f ? 1.f : 0.f;
    const float err = fabsf(gt - rd) * valid;
    return err != err ? 0xffffffffu : __float_as_uint(err);
}

// One histogram add per active lane, every lane of the wave calling: the lanes sharing the first active
// lane's bin are counted with a ballot and added at once, twice; the others add one by one.
__device__ __forceinline__ void dn_hist_add(uint32_t* s_hist, uint32_t bin, bool active, int lane) {
    unsigned long long todo = __ballot(active);
    for (int round = 0; round < 2 && todo != 0ull; round++) {  // (todo is wave-uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lb = (uint32_t)__shfl((int)bin, leader);
        const unsigned long long same = __ballot(active && bin == lb);
        if (lane == leader) atomicAdd(&s_hist[lb], (uint32_t)__popcll(same));
        active = active && bin != lb;
        todo &= ~same;
    }
    if (active) atomicAdd(&s_hist[bin], 1u);
}

__global__ void __launch_bounds__(DN_BLOCK)
dn_zero_kernel(uint32_t* __restrict__ hist) {
    hist[blockIdx.x * DN_BLOCK + threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(DN_BLOCK)
dn_select_kernel(int pass, int N, const float* __restrict__ depth_sil, const float* __restrict__ gt_depth,
                 uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_hist[DN_BINS];
    __shared__ uint32_t s_scan[DN_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63;
    const DnLayout lay = DnLayout::make(N);
    uint32_t* const hist = ws + lay.hist + (size_t)pass * DN_BINS;
    for (int i = tid; i < DN_BINS; i += DN_BLOCK) s_hist[i] = 0u;
    __syncthreads();
    // pass 0: digit bits 31..21 of every key; pass 1: bits 20..10 of the keys whose bits 31..21 are the
    // chosen ones; pass 2: bits 9..0 of the keys whose bits 31..10 are
    const int hi_shift = pass == 0 ? 32 : (pass == 1 ? 21 : 10);
    const int lo_shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const uint32_t digit_mask = (1u << (hi_shift - lo_shift)) - 1u;
    const uint32_t prefix = pass == 0 ? 0u : ws[DN_PREFIX + pass - 1];
    const size_t p0 = (size_t)blockIdx.x * DN_TILE;
#pragma unroll
    for (int i = 0; i < DN_ITEMS; i++) {
        const size_t p = p0 + (size_t)i * DN_BLOCK + tid;
        const bool in = p < (size_t)N;
        const uint32_t key = in ? dn_key(gt_depth[p], depth_sil[p]) : 0u;
        const bool match = in && (pass == 0 || (key >> hi_shift) == prefix);
        dn_hist_add(s_hist, (key >> lo_shift) & digit_mask, match, lane);
    }
    __syncthreads();
    for (int i = tid; i < DN_BINS; i += DN_BLOCK) {
        const uint32_t c = s_hist[i];
        if (c) __hip_atomic_fetch_add(hist + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_block_arrive(ws + pass)) return;
    // ---- last workgroup: the bin that holds the wanted rank (thread t owns bins [8 t, 8 t + 8))
    const uint32_t want = pass == 0 ? (uint32_t)((N - 1) / 2) : ws[DN_RANK + pass - 1];
    uint32_t c[DN_BINS / DN_BLOCK], sum = 0;
#pragma unroll
    for (int j = 0; j < DN_BINS / DN_BLOCK; j++) {
        c[j] = ld_agent(hist + tid * (DN_BINS / DN_BLOCK) + j);
        sum += c[j];
    }
    uint32_t below = block_scan_incl(sum, s_scan) - sum;
    if (pass == 0 && tid == DN_BLOCK - 1) ws[DN_NAN] = c[DN_BINS / DN_BLOCK - 1];  // bin 2047: the NaN keys
    if (want >= below && want < below + sum) {  // (one thread: the bins' total exceeds the rank)
        int j = 0;
#pragma unroll
        for (int u = 0; u < DN_BINS / DN_BLOCK - 1; u++)
            if (j == u && want >= below + c[u]) {
                below += c[u];
                j = u + 1;
            }
        const uint32_t chosen = (prefix << (hi_shift - lo_shift)) | (uint32_t)(tid * (DN_BINS / DN_BLOCK) + j);
        if (pass < 2) {
            ws[DN_PREFIX + pass] = chosen;
            ws[DN_RANK + pass] = want - below;
        } else {
            ws[DN_MED] = chosen;
        }
    }
}

__device__ __forceinline__ bool dn_selected(float sil, float rd, float gt, float sil_thres, float thr) {
#pragma clang fp contract(off)
    const bool valid = gt > 0.f;
    const float err = fabsf(gt - rd) * (valid ? 1.f : 0.f);
    return ((sil < sil_thres) || ((rd > gt) && (err > thr))) && valid;
}

// Step 3's threshold from the median (include/gsr_glue.h: gsr_densify_frame_capped).  capped: the host's
// (float)((double)median_scale * (double)median_thr).  A NaN med fails the comparison and stays a NaN.
struct DnThr {
    int use_median_thr;
    float median_thr, median_scale, capped;
};
__device__ __forceinline__ float dn_threshold(const DnThr& t, float med) {
#pragma clang fp contract(off)
    if (!t.use_median_thr) return t.median_scale * med;
    return med > t.median_thr ? t.capped : 50.f * med;
}

// INIT (gsr_init_frame): every pixel with a measured depth is selected; depth_sil, the median and the
// threshold are not read.
template <bool INIT>
__global__ void __launch_bounds__(DN_BLOCK)
dn_count_kernel(int N, const float* __restrict__ depth_sil, const float* __restrict__ gt_depth, float sil_thres,
                DnThr tcfg, int capacity, uint32_t* __restrict__ ws, long long* __restrict__ n_live,
                unsigned char* __restrict__ overflow, long long* __restrict__ n_added) {
#pragma clang fp contract(off)
    __shared__ uint32_t s_wave[DN_WAVES];
    __shared__ uint32_t s_scan[DN_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DnLayout lay = DnLayout::make(N);
    uint32_t* const cnt = ws + lay.cnt;
    uint32_t* const excl = ws + lay.excl;
    unsigned long long* const mask = (unsigned long long*)(ws + lay.mask) + (size_t)blockIdx.x * DN_CHUNKS;
    float thr = 0.f;
    if (!INIT) thr = dn_threshold(tcfg, __uint_as_float(ws[DN_NAN] != 0u ? DN_QNAN : ws[DN_MED]));
    const size_t p0 = (size_t)blockIdx.x * DN_TILE;
    uint32_t count = 0;  // (wave-uniform: every lane adds the wave's popcount)
#pragma unroll
    for (int i = 0; i < DN_ITEMS; i++) {
        const size_t p = p0 + (size_t)i * DN_BLOCK + tid;
        bool sel = false;
        if (p < (size_t)N)
            sel = INIT ? gt_depth[p] > 0.f
                       : dn_selected(depth_sil[(size_t)N + p], depth_sil[p], gt_depth[p], sil_thres, thr);
        const unsigned long long m = __ballot(sel);
        if (lane == 0) mask[i * DN_WAVES + wave] = m;
        count += (uint32_t)__popcll(m);
    }
    block_count_publish(count, s_wave, cnt + blockIdx.x);
    if (!last_block_arrive(ws + 3)) return;
    // ---- last workgroup: the exclusive scan of the workgroups' counts
    const uint32_t total_added = last_block_scan_excl(cnt, lay.nb, excl, s_scan);
    if (tid == DN_BLOCK - 1) {
        const long long added = (long long)total_added;
        const long long old = n_live[0];  // (read before the new value is written)
        *(long long*)(ws + DN_BASE) = old;
        const long long total = old + added;
        n_added[0] = added;
        n_live[0] = total < (long long)capacity ? total : (long long)capacity;
        if (total > (long long)capacity) overflow[0] = 1;
    }
}

__global__ void __launch_bounds__(DN_BLOCK)
dn_scatter_kernel(int H, int W, const float* __restrict__ gt_im, const float* __restrict__ gt_depth, DnCam cam,
                  const float* __restrict__ w2c, int capacity, const uint32_t* __restrict__ ws,
                  float* __restrict__ means3D, float* __restrict__ rgb, float* __restrict__ rot,
                  float* __restrict__ logit_opac, float* __restrict__ log_scales, unsigned char* __restrict__ alive,
                  int* __restrict__ dest) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_mask[DN_CHUNKS];
    __shared__ uint32_t s_pre[DN_CHUNKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t N = (size_t)H * W;
    const DnLayout lay = DnLayout::make((long long)N);
    const unsigned long long* const mask =
        (const unsigned long long*)(ws + lay.mask) + (size_t)blockIdx.x * DN_CHUNKS;
    if (tid < DN_CHUNKS) s_mask[tid] = mask[tid];
    __syncthreads();
    if (tid == 0) {  // the chunks' exclusive popcount prefix, in pixel order
        uint32_t run = 0;
        for (int k = 0; k < DN_CHUNKS; k++) {
            s_pre[k] = run;
            run += (uint32_t)__popcll(s_mask[k]);
        }
    }
    __syncthreads();
    const long long base = *(const long long*)(ws + DN_BASE) + (long long)ws[lay.excl + blockIdx.x];
    const size_t p0 = (size_t)blockIdx.x * DN_TILE;
    const RigidInverse c2w = rigid_inverse(w2c);
#pragma unroll
    for (int i = 0; i < DN_ITEMS; i++) {
        const size_t p = p0 + (size_t)i * DN_BLOCK + tid;
        if (p >= N) continue;
        const int k = i * DN_WAVES + wave;
        const unsigned long long m = s_mask[k];
        long long row = -1;
        if ((m >> lane) & 1ull) {
            row = base + (long long)(s_pre[k] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
            if (row < 0 || row >= (long long)capacity) row = -1;
        }
        if (dest) dest[p] = (int)row;
        if (row < 0) continue;
        const int py = (int)(p / (size_t)W), px = (int)(p - (size_t)py * W);
        const float z = gt_depth[p];
        const float3 w = backproject(px, py, z, cam.fx, cam.fy, cam.cx, cam.cy, c2w);
        const size_t o = (size_t)row;
        means3D[3 * o + 0] = w.x; means3D[3 * o + 1] = w.y; means3D[3 * o + 2] = w.z;
#pragma unroll
        for (int a = 0; a < 3; a++) rgb[3 * o + a] = gt_im[(size_t)a * N + p];
        rot[4 * o + 0] = 1.f; rot[4 * o + 1] = 0.f; rot[4 * o + 2] = 0.f; rot[4 * o + 3] = 0.f;
        logit_opac[o] = 0.f;
        const float q = z / cam.f;
        log_scales[o] = logf(sqrtf(q * q));
        alive[o] = 1;
    }
}

}  // namespace
}  // namespace gsr

using namespace gsr;

// What the three entries share: the argument checks (`who` names the entry in gsr_last_error()), then the
// count and scatter launches; !INIT: the histogram zeroing and the three selection passes before them.
template <bool INIT>
static int dn_enqueue(const char* who, int H, int W, const float* depth_sil, const float* gt_im,
                      const float* gt_depth, float fx, float fy, float cx, float cy, const float* w2c, float sil_thres,
                      DnThr tcfg, int capacity, float* means3D, float* rgb_colors, float* unnorm_rotations,
                      float* logit_opacities, float* log_scales, unsigned char* alive, long long* n_live,
                      unsigned char* overflow, long long* n_added, int* dest, void* workspace, void* stream) {
    auto refuse = [&](const char* what) { return fail(GSR_ERR_INVALID_ARG, std::string(who) + ": " + what); };
    if (!image_size_ok(H, W)) return refuse("bad image size");
    if (capacity < 0) return refuse("negative capacity");
    if ((!INIT && !depth_sil) || !gt_im || !gt_depth || !w2c || !means3D || !rgb_colors || !unnorm_rotations ||
        !logit_opacities || !log_scales || !alive || !n_live || !overflow || !n_added || !workspace)
        return refuse("null pointer");
    if (!aligned16(workspace)) return refuse("workspace must be 16-byte aligned");
    const int N = H * W;
    const DnLayout lay = DnLayout::make(N);
    uint32_t* const ws = (uint32_t*)workspace;
    const DnCam cam{fx, fy, cx, cy, (float)(((double)fx + (double)fy) / 2.0)};
    const hipStream_t st = (hipStream_t)stream;
    if (!INIT) {
        hipLaunchKernelGGL(dn_zero_kernel, dim3(3 * DN_BINS / DN_BLOCK), dim3(DN_BLOCK), 0, st, ws + lay.hist);
        for (int pass = 0; pass < 3; pass++)
            hipLaunchKernelGGL(dn_select_kernel, dim3(lay.nb), dim3(DN_BLOCK), 0, st, pass, N, depth_sil, gt_depth,
                               ws);
    }
    hipLaunchKernelGGL(dn_count_kernel<INIT>, dim3(lay.nb), dim3(DN_BLOCK), 0, st, N, depth_sil, gt_depth, sil_thres,
                       tcfg, capacity, ws, n_live, overflow, n_added);
    hipLaunchKernelGGL(dn_scatter_kernel, dim3(lay.nb), dim3(DN_BLOCK), 0, st, H, W, gt_im, gt_depth, cam, w2c,
                       capacity, (const uint32_t*)ws, means3D, rgb_colors, unnorm_rotations, logit_opacities,
                       log_scales, alive, dest);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, who);
}

extern "C" {

size_t gsr_densify_workspace_bytes(int H, int W) {
    if (!image_size_ok(H, W)) return 0;
    return DnLayout::make((long long)H * W).total;
}

int gsr_densify_frame(int H, int W, const float* depth_sil, const float* gt_im, const float* gt_depth, float fx,
                      float fy, float cx, float cy, const float* w2c, float sil_thres, int capacity, float* means3D,
                      float* rgb_colors, float* unnorm_rotations, float* logit_opacities, float* log_scales,
                      unsigned char* alive, long long* n_live, unsigned char* overflow, long long* n_added, int* dest,
                      void* workspace, void* stream) {
    return dn_enqueue<false>("densify_frame", H, W, depth_sil, gt_im, gt_depth, fx, fy, cx, cy, w2c, sil_thres,
                             DnThr{0, 0.f, 50.f, 0.f}, capacity, means3D, rgb_colors, unnorm_rotations,
                             logit_opacities, log_scales, alive, n_live, overflow, n_added, dest, workspace, stream);
}

int gsr_densify_frame_capped(int H, int W, const float* depth_sil, const float* gt_im, const float* gt_depth,
                             float fx, float fy, float cx, float cy, const float* w2c, float sil_thres, int capacity,
                             float* means3D, float* rgb_colors, float* unnorm_rotations, float* logit_opacities,
                             float* log_scales, unsigned char* alive, long long* n_live, unsigned char* overflow,
                             long long* n_added, int* dest, void* workspace, void* stream, int use_median_thr,
                             float median_thr, float median_scale) {
    const DnThr tcfg{use_median_thr != 0, median_thr, median_scale,
                     (float)((double)median_scale * (double)median_thr)};
    return dn_enqueue<false>("densify_frame_capped", H, W, depth_sil, gt_im, gt_depth, fx, fy, cx, cy, w2c,
                             sil_thres, tcfg, capacity, means3D, rgb_colors, unnorm_rotations, logit_opacities,
                             log_scales, alive, n_live, overflow, n_added, dest, workspace, stream);
}

int gsr_init_frame(int H, int W, const float* gt_im, const float* gt_depth, float fx, float fy, float cx, float cy,
                   const float* w2c, int capacity, float* means3D, float* rgb_colors, float* unnorm_rotations,
                   float* logit_opacities, float* log_scales, unsigned char* alive, long long* n_live,
                   unsigned char* overflow, long long* n_added, int* dest, void* workspace, void* stream) {
    return dn_enqueue<true>("init_frame", H, W, nullptr, gt_im, gt_depth, fx, fy, cx, cy, w2c, 0.f,
                            DnThr{0, 0.f, 50.f, 0.f}, capacity, means3D, rgb_colors, unnorm_rotations,
                            logit_opacities, log_scales, alive, n_live, overflow, n_added, dest, workspace, stream);
}

}  // extern "C"
