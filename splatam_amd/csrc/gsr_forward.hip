// gsr_forward.hip -- the forward render kernel of the MI355X-native Gaussian rasterizer, and the map of the
// forward pipeline it ends.  One launch per stage, in this order (gsr_capi.hip, Forward):
//
//   preprocess  gsr_preprocess.hip  (forward.cu:155-256)  one lane per Gaussian: 64-B render records, rects,
//               live-tile masks, and the per-tile instance counts as one row per workgroup of the
//               [workgroup x tile] count matrix (LDS histogram; global atomics beyond MAX_LDS_TILES tiles)
//   colscan     gsr_binning.hip     (rasterizer_impl.cu:277, InclusiveSum)  column scan of the count matrix:
//               every workgroup's offset inside every tile's bucket, and the tile totals
//   duplicate   gsr_binning.hip     (rasterizer_impl.cu:70-111 duplicateWithKeys, 116-138 identifyTileRanges)
//               bucketed: every workgroup scans the workgroup and tile totals itself (ranges, counters), then
//               puts each instance straight into its tile's bucket, keyed (depth << 32 | id); workgroup 0
//               also deals the tiles to render workgroups by list length (tile_plan, the render schedule)
//   render      here, gsr_render_fwd.h  (rasterizer_impl.cu:301-309 the sort, forward.cu:261-393 the render)
//               one 16x16 tile per 256-lane workgroup: sorts its bucket in the prologue (tile_sort_bucket),
//               then 256-entry LDS batches with block masks and block-wide early exit
// A tile list longer than TILE_SORT_CAP, or GSR_FORCE_RADIX, takes the fallback instead of the bucketed
// duplicate: a global stable radix sort (gsr_radix.hip); the render then skips its sort.  The geometry-reuse
// forms that skip the binning altogether are gsr_reuse.hip.
#include "gsr_clock.h"
#include "gsr_diag.h"
#include "gsr_launch.h"
#include "gsr_layout.h"
#include "gsr_render_fwd.h"
#include "gsr_wave.h"

namespace gsr {

// ----------------------------------------------------------- render (fwd) --
// Per 256-entry batch every Gaussian gets a 16-bit mask of the 4x4-pixel blocks
// its contribution ellipse reaches (block_mask); each 16-lane row (one block)
// then walks only its own compacted list, 4 entries per step (the four rows of
// a wave walk different lists in lockstep): the LDS reads and exp/alpha of the 4
// entries are independent (ILP), the transmittance chain is then applied in
// order with predicated (branch-free) updates.  The next batch's global
// gathers are issued before the current batch is rasterised.
// DUAL: a second colour set (colors2, e.g. SplaTAM's [z, 1, z^2]) is composited
// in the same pass -- same alpha / T / termination, so each output is bitwise
// the image a separate call would produce.
// L1 (with DUAL): the tracking loss epilogue of TrackL1 (gsr_launch.h).
template <bool DUAL, bool L1 = false>
__global__ void __launch_bounds__(TILE_PIX, 5)
render_fwd_kernel(Camera cam, const uint2* __restrict__ ranges, PointEntry* __restrict__ point_list,
                  uint64_t* __restrict__ keys, const float4* __restrict__ rr, float* __restrict__ final_T, uint32_t* __restrict__ n_contrib,
                  float* __restrict__ out_color, float* __restrict__ out_color2, float* __restrict__ out_depth,
                  SpecGuard guard, unsigned long long* clk, TrackL1 l1) {
    static_assert(DUAL || !L1, "the tracking loss needs the depth / silhouette colour set");
    if (cam.gate.off()) return;
    kclock_begin(clk);
    RenderDiag dg;  // (diagnostics builds only, gsr_diag.h): phases 0 sort, 1 staging, 2 lists, 3 walk, 4 barrier,
    dg.begin();     // 5 epilogue
    if (guard.overflow()) {
        kclock_end(clk);
        return;
    }
    __shared__ __attribute__((aligned(16))) char smem[FwdShape<DUAL>::bytes];
    const int tile = sched_tile(cam);
    dg.tile(tile);
    const FwdPix f = fwd_tile<DUAL>(cam, tile, ranges, point_list, keys, rr, guard, smem, dg);
    float g[4];
    fwd_epilogue<DUAL, L1, true>(cam, tile, f, final_T, n_contrib, out_color, out_color2, out_depth, l1, g);
    dg.phase(5);
    dg.end();
    kclock_end(clk);
}

#if GSR_PHASE
extern "C" int gsr_diag_phase_fwd(unsigned long long* host) {  // copies and clears the phase cycles
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase), sizeof(g_phase), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#endif
#if GSR_WGTIME
extern "C" int gsr_diag_wgtime_fwd(unsigned long long* host, int n) {
    const size_t bytes = sizeof(unsigned long long) * 4 * (size_t)(n < GSR_WGTIME_MAX ? n : GSR_WGTIME_MAX);
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wgtime), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

int track_l1_fused_scratch_floats(int ntiles) { return 2 * ntiles + ARRIVE_GROUPED_WORDS; }

hipError_t launch_render_fwd(const Camera& cam, const uint2* ranges, uint64_t* point_list,
                             uint64_t* keys, GeomPtrs geo,
                             const float* colors2, float* final_T, uint32_t* n_contrib, float* out_color,
                             float* out_color2, float* out_depth, SpecGuard guard, hipStream_t s,
                             unsigned long long* clk, const TrackL1* l1) {
    auto k = colors2 ? (l1 ? render_fwd_kernel<true, true> : render_fwd_kernel<true, false>)
                     : render_fwd_kernel<false, false>;
    hipLaunchKernelGGL(k, dim3(cam.gx * cam.gy), dim3(TILE_PIX), 0, s, cam, ranges, point_list, keys,
                       geo.rr, final_T,
                       n_contrib, out_color, out_color2, out_depth, guard, clk, l1 ? *l1 : TrackL1{});
    return hipGetLastError();
}

}  // namespace gsr
