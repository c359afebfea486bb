// gsr_backward.hip -- backward pipeline of the MI355X-native Gaussian rasterizer.
//
// power == 1 (the standard 3DGS backward; SplaTAM's tracking/mapping path):
//   render_bwd  (backward.cu:586-748 semantics) one 16x16 tile per workgroup,
//               back-to-front over LDS batches; each 16-lane row walks the list
//               of its 4x4-pixel block.  The per-pair 2D gradient terms are
//               summed across the row with a transposed DPP reduction, the 16
//               block partials are added through LDS in a fixed order, and ONE
//               plain 48-B record per (tile, Gaussian) instance is stored at
//               its unsorted position.
//               No global atomics at all: the reference issues ~25 float
//               atomics per contributing pair (backward.cu:1093-1137).
//   gauss_bwd   one lane per Gaussian: sums its instance records in a fixed
//               order (deterministic, bitwise reproducible) and applies the
//               per-Gaussian chain rule (backward.cu:144-274 cov2D,
//               412-475 cov3D, 480-530 projection, 20-139 SH).
// Here: the kernels around the tile backward (the M2D1 and the fused tracking render), gauss_bwd and the
// launchers.  The tile backward itself (bwd_tile, its variants and render_bwd_kernel) is gsr_render_bwd.h;
// the backward_power == 2 route through second moments is gsr_backward_power.hip.
#include <cstdlib>

#include "gsr_chain.h"
#include "gsr_clock.h"
#include "gsr_diag.h"
#include "gsr_dispatch.h"
#include "gsr_glue_common.h"
#include "gsr_launch.h"
#include "gsr_layout.h"
#include "gsr_math.h"
#include "gsr_render_bwd.h"
#include "gsr_render_fwd.h"
#include "gsr_wave.h"

namespace gsr {

// The mapping form with the first colour set's own (hx, hy) sums (MapM2dVariant): a kernel of its own, so that
// no existing instantiation's name, arguments or code change.  4 waves per SIMD: the mapping variant sits at 94 of
// the 96 VGPRs that 5 waves allow, and the second accumulator with its four per-pair products spilled there (44 B
// of scratch per lane with the pair as its own pass, 68 B riding with the colour sums: tools/kernel_resources.py).
__global__ void __launch_bounds__(TILE_PIX, GSR_BWD_M2D_WAVES)
render_bwd_m2d_kernel(Camera cam, const uint2* __restrict__ ranges, const PointEntry* __restrict__ point_list,
                      const float4* __restrict__ rr, const uint32_t* __restrict__ blocksums,
                      const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                      const float* __restrict__ dL_dpix, const float* __restrict__ dL_dpix2, float* __restrict__ inst,
                      BwdGuard guard, unsigned long long* clk) {
    using V = MapM2dVariant;
    kclock_begin(clk);
    RenderDiag dg;
    dg.begin();
    if (guard.overflow()) {
        kclock_end(clk);
        return;
    }
    __shared__ __attribute__((aligned(16))) char smem[BwdShape<V>::bytes];
    const int tid = threadIdx.x;
    const int tile = sched_tile(cam), tx = tile % cam.gx, ty = tile / cam.gx;
    dg.tile(tile);
    const int px = tx * TILE_X + tile_px(tid);
    const int py = ty * TILE_Y + tile_py(tid);
    BwdPix pin{0.f, 0u, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    load_bwd_pix<V::DUAL, V::Q2>(pin, cam, px, py, final_T, n_contrib, dL_dpix, dL_dpix2);
    bwd_tile<V>(cam, tile, pin, ranges, point_list, rr, blocksums, inst, guard, smem, dg);
    dg.end();
    kclock_end(clk);
}

// The tracking iteration's render in one launch per tile (SplaTAM get_loss(tracking=True) with a static
// loss seed, scripts/splatam.py:220-353): the dual forward with the L1 loss epilogue, then -- in the same
// workgroup, its LDS reused -- the back-to-front walk of the depth-channel / geometric backward
// (TrackVariant, render_bwd_kernel's tracking form) from the pixel state still in registers.  The loss
// gradient is per pixel, so a tile's backward needs nothing from other tiles.  Saves the second launch
// (dispatch, drain, the end-of-kernel writeback), the backward's per-pixel reads (T, n_contrib, dL/dpix)
// and the forward's gradient-image stores.  Results are bitwise those of render_fwd + render_bwd.
constexpr size_t track_lds_bytes() {
    return FwdShape<true>::bytes > BwdShape<TrackVariant>::bytes ? FwdShape<true>::bytes : BwdShape<TrackVariant>::bytes;
}
// IMAGES = false: the images (and final_T / n_contrib / the block maxima) are not stored -- a separate
// instantiation, so that no store (and no wait the compiler places for one) is left in the code
template <bool IMAGES>
__global__ void __launch_bounds__(TILE_PIX, 5)
render_track_kernel(Camera cam, const uint2* __restrict__ ranges, PointEntry* __restrict__ point_list,
                    uint64_t* __restrict__ keys, const float4* __restrict__ rr, const uint32_t* __restrict__ blocksums,
                    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, float* __restrict__ out_color,
                    float* __restrict__ out_color2, float* __restrict__ out_depth, SpecGuard guard,
                    unsigned long long* clk, TrackL1 l1, float* __restrict__ inst) {
    kclock_begin(clk);
    RenderDiag dg;
    dg.begin();
    if (guard.overflow()) {
        kclock_end(clk);
        return;
    }
    __shared__ __attribute__((aligned(16))) char smem[track_lds_bytes()];
    if constexpr (!IMAGES) {  // (fwd_epilogue stores nothing for a null final_T)
        final_T = nullptr;
        cam.rowmax = nullptr;
    }
    const int tile = sched_tile(cam);
    dg.tile(tile);
    const FwdPix f = fwd_tile<true>(cam, tile, ranges, point_list, keys, rr, guard, smem, dg);
    float grad[4];
    // (the loss arrival stays here: moved after the backward it put the last workgroup's sum at the kernel's
    // end, within noise or 0.5 us slower: profiles/r4o_ab_l1_defer.txt)
    // STORE_GRADS = false: the gradient images are not formed here, and the C entry passes l1.dL_dim /
    // l1.dL_dds as NULL (a variant that stores them needs real image pointers from gsr_capi.hip)
    constexpr bool kStoreGrads = false;
    static_assert(!kStoreGrads, "render_track_kernel's callers pass no gradient images");
    fwd_epilogue<true, true, kStoreGrads>(cam, tile, f, final_T, n_contrib, out_color, out_color2, out_depth, l1,
                                          grad);
    __syncthreads();  // the forward's LDS (and its sorted point_list stores) before the backward reuses them
    const BwdPix pin{f.T, f.last16 >> 4, grad[0], grad[1], grad[2], grad[3], 0.f, 0.f};
    Camera cb = cam;
    cb.rowmax = nullptr;  // the block maxima from the registers
    bwd_tile<TrackVariant>(cb, tile, pin, ranges, point_list, rr, blocksums, inst,
                           BwdGuard{guard.counters, guard.cap_inst}, smem, dg);
    dg.end();
    kclock_end(clk);
}

int track_records_stride() { return BwdShape<TrackVariant>::RS; }

hipError_t launch_render_track(const Camera& cam, const uint2* ranges, uint64_t* point_list, uint64_t* keys,
                               GeomPtrs geo, float* final_T, uint32_t* n_contrib, float* out_color,
                               float* out_color2, float* out_depth, SpecGuard guard, const TrackL1& l1, float* inst,
                               hipStream_t s, unsigned long long* clk) {
    auto k = final_T != nullptr ? render_track_kernel<true> : render_track_kernel<false>;
    hipLaunchKernelGGL(k, dim3(cam.gx * cam.gy), dim3(TILE_PIX), 0, s, cam, ranges, point_list,
                       keys, geo.rr, geo.blocksums, final_T, n_contrib, out_color, out_color2, out_depth, guard, clk,
                       l1, inst);
    return hipGetLastError();
}

// (need, dual) decoded into the optional per-pair sums of the variant: opacity, colours, second colours and
// the second image's gradient channels (1 or 3; 3 without a second image)
struct BwdTerms {
    bool op, c1, c2;
    int q2;
};
static BwdTerms bwd_terms(unsigned need, bool dual) {
    return {(need & NEED_OPACITY) != 0, (need & NEED_COLORS) != 0, dual && (need & NEED_COLORS2),
            (dual && (need & NEED_DL2_CH0_ONLY)) ? 1 : 3};
}

// The variant launch_render_bwd picks for (need, dual) and its record layout.
RecLayout bwd_rec_layout(unsigned need, bool dual) {
    const auto [op, c1, c2, q2] = bwd_terms(need, dual);
    return rec_sums(op, c1, c2, q2).rec;
}

// The 20 forms bwd_terms() can ask for: without a second image neither its colour sums nor its channel promise
using RenderBwdFn = decltype(render_bwd_of<TrackVariant>());  // (every form has the one argument list)
struct PickRenderBwd {
    template <bool DUAL, bool OP, bool C1, bool C2, bool Q1>
    RenderBwdFn operator()() const {
        if constexpr (!DUAL && (C2 || Q1)) return nullptr;
        else return render_bwd_of<BwdVariant<DUAL, OP, C1, C2, Q1 ? 1 : 3>>();
    }
};

hipError_t launch_render_bwd(const Camera& cam, const uint2* ranges, const uint64_t* point_list, GeomPtrs geo,
                             const float* final_T, const uint32_t* n_contrib, const float* dL_dpix,
                             const float* colors2, const float* dL_dpix2, unsigned need, float* inst,
                             BwdGuard guard, hipStream_t s, unsigned long long* clk) {
    const auto [op, c1, c2, q2] = bwd_terms(need, colors2 != nullptr);
    // (c2 and q2 == 1 only with a second image; SplaTAM tracking is <dual, c2, q1>, mapping every sum with q1)
    const auto k = dispatch_bools(PickRenderBwd{}, colors2 != nullptr, op, c1, c2, q2 == 1);
    hipLaunchKernelGGL(k, dim3(cam.gx * cam.gy), dim3(TILE_PIX), 0, s, cam, ranges, point_list, geo.rr, geo.blocksums,
                       final_T, n_contrib, dL_dpix, dL_dpix2, inst, guard, clk);
    return hipGetLastError();
}

int m2d_record_stride() { return BwdShape<MapM2dVariant>::RS; }
static_assert(BwdShape<MapM2dVariant>::O_M1 == M2D_REC_PAIR && BwdShape<MapM2dVariant>::NV == M2D_REC_PAIR + 2 &&
                  BwdShape<MapM2dVariant>::RS <= INST_REC_MAX,
              "the M2D1 record: the mapping variant's ten sums, then the pair");

hipError_t launch_render_bwd_m2d(const Camera& cam, const uint2* ranges, const uint64_t* point_list, GeomPtrs geo,
                                 const float* final_T, const uint32_t* n_contrib, const float* dL_dpix,
                                 const float* dL_dpix2, float* inst, BwdGuard guard, hipStream_t s,
                                 unsigned long long* clk) {
    hipLaunchKernelGGL(render_bwd_m2d_kernel, dim3(cam.gx * cam.gy), dim3(TILE_PIX), 0, s, cam, ranges, point_list,
                       geo.rr, geo.blocksums, final_T, n_contrib, dL_dpix, dL_dpix2, inst, guard, clk);
    return hipGetLastError();
}

// SHL: per-lane SH chain (g.shs may be set).  Without it (colours precomputed, or SH handled by
// the staged sh_bwd_kernel) g.shs is NULL at compile time, and the 48-float dsh array and the SH
// chain drop out of the kernel (mapping variant: 142 -> fewer VGPRs, more waves per SIMD).
// at most 5 waves per SIMD: at 78-80 VGPRs the kernel would run 6, and the sixth wave measured slower for the
// mapping variant (1 M anisotropic Gaussians: 65.0 -> 64.0 us capped) and no faster for tracking
// (profiles/r5z_ab_gauss_bwd_waves.txt)
// M2D1 (m1.dmeans2D_c1 set): the records carry the first colour set's own (hx, hy) at m1.o_m1; its means2D
// gradient -ddel (Q [hx1, hy1]) -- the expression that forms g2[0..1] -- goes to m1.dmeans2D_c1, z as 0.
template <bool POSE, bool SHL, bool M2D1 = false>
__device__ __forceinline__ void gauss_bwd_body(Camera cam, GaussIn g, GeomPtrs geo, const int* __restrict__ radii,
                                               const float* __restrict__ inst, RecLayout rec, GradsOut out,
                                               BwdGuard guard, PoseFuse pf, M2dOut m1 = M2dOut{}) {
    static_assert(!M2D1 || !POSE, "M2D1: the mapping backward only");
    if constexpr (!SHL) {
        g.shs = nullptr;
        g.M = 0;
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!POSE && i >= g.P) return;  // (POSE: every lane takes part in the workgroup sum)
    const bool live = i < g.P;
    const int nsh = g.shs ? (cam.sh_degree + 1) * (cam.sh_degree + 1) : 0;
    float g2[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dcol2[3] = {0.f, 0.f, 0.f};
    [[maybe_unused]] float m2d1[2] = {0.f, 0.f};
    float dmean[3] = {0.f, 0.f, 0.f}, dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dscale[3] = {0.f, 0.f, 0.f},
          drot[4] = {0.f, 0.f, 0.f, 0.f};
    float dsh[48];
#pragma unroll
    for (int k = 0; k < 48; k++) dsh[k] = 0.f;
    // the Gaussian's geometry: recomputed from the world-frame map and the pre-step pose (tracking
    // forward that did not store its rendervars, PoseFuse::ls) or read from GaussIn
    GaussGeom gg;
    gg.m = make_float3(0.f, 0.f, 0.f);
    gg.s = make_float3(0.f, 0.f, 0.f);
    gg.q = make_float4(0.f, 0.f, 0.f, 0.f);
    // POSE: the frame's (pre-step) pose is workgroup-uniform: formed once by thread 0 (8 IEEE divisions and 2
    // square roots per lane otherwise) and read from LDS -- the same bits.  The Gaussian's own inputs (radius,
    // record range, the world-frame transform inputs) are loaded ahead of that barrier: loads issued after a
    // __syncthreads would wait for thread 0's pose chain (its loads and the make_pose arithmetic)
    const int rad = live ? radii[i] : 0;
    const bool xf_geom = POSE && pf.ls;
    TrackXf x;
    x.mw = pf.means_world; x.ur = pf.unnorm_rot; x.ls = pf.ls; x.scols = pf.scols;
    XfRaw xr{};
    if (xf_geom && live) xr = track_xform_load(x, i, false);
    uint32_t off = 0, cnt = 0, tl = 0xFFFFFFFFu;  // tl: live-tile mask (Camera::cull: culled slots are unwritten)
    if (POSE && live && rad > 0) {
        off = geo.offsets[i];
        cnt = geo.tiles[i];
        tl = reinterpret_cast<const uint32_t*>(geo.bin)[4 * (size_t)i + 3];
    }
    __shared__ Pose s_pose;
    if constexpr (POSE) {
        if (pf.ls || pf.scols != 1) {
            if (threadIdx.x == 0) s_pose = make_pose(pf.cam_q, pf.cam_t, pf.qs);
            __syncthreads();
        }
    }
    if (live && (POSE || rad > 0)) {  // (the pose sums need every live Gaussian's mean)
        if (xf_geom) {
            const Pose ps = s_pose;
            float m[3], sv[3];
            track_xform_geom_raw(xr, x.scols, ps, m, gg.q, sv);
            gg.m = make_float3(m[0], m[1], m[2]);
            gg.s = make_float3(sv[0], sv[1], sv[2]);
        } else {
            gg = load_geom(g, i);
        }
    }
    if (live && rad > 0 && !guard.overflow()) {  // overflow: zero gradients, no record reads
        if (!POSE) {
            off = geo.offsets[i];
            cnt = geo.tiles[i];
            tl = reinterpret_cast<const uint32_t*>(geo.bin)[4 * (size_t)i + 3];
        }
        // fixed-order sum of the Gaussian's instance records (deterministic)
        float acc[INST_REC_MAX];
#pragma unroll
        for (int m = 0; m < INST_REC_MAX; m++) acc[m] = 0.f;
        const int np = rec.stride / 2;
        // RU records' loads issued together (one memory round trip per RU instances instead of
        // per instance), then added in instance order: the same sums, bit for bit
        constexpr int RU = 4;
        for (uint32_t e0 = 0; e0 < cnt; e0 += RU) {
            float2 v[RU][INST_REC_MAX / 2];
#pragma unroll
            for (int k = 0; k < RU; k++) {
                const float2* r = reinterpret_cast<const float2*>(inst + (size_t)rec.stride * (off + e0 + k));
#pragma unroll
                for (int m = 0; m < INST_REC_MAX / 2; m++)
                    v[k][m] = (m < np && e0 + k < cnt && tile_live(tl, e0 + k)) ? r[m] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int k = 0; k < RU; k++)
                if (e0 + k < cnt && tile_live(tl, e0 + k)) {  // (a culled slot's record would be +0: skipped exactly)
#pragma unroll
                    for (int m = 0; m < INST_REC_MAX / 2; m++)
                        if (m < np) {
                            acc[2 * m] += v[k][m].x;
                            acc[2 * m + 1] += v[k][m].y;
                        }
                }
        }
#pragma unroll
        for (int m = 0; m < 5; m++) g2[m] = acc[m];
#pragma unroll
        for (int m = 0; m < INST_REC_MAX; m++) {  // constant-index selects (no dynamic register indexing)
            if (m == rec.o_op) g2[5] = acc[m];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (rec.o_c1 >= 0 && m == rec.o_c1 + k) g2[6 + k] = acc[m];
                if (rec.o_c2 >= 0 && k < rec.n_c2 && m == rec.o_c2 + k) dcol2[k] = acc[m];
            }
        }
        // instance records hold (hx, hy, hxx, hxy, hyy, dopacity, dcolor) sums (render_bwd_kernel);
        // the conic is recomputed exactly as preprocess computed it (the render record keeps
        // only its exp2-scaled form)
        float ca, cb, cc, c3[6];
        Proj pj;
        gaussian_conic(cam, g, gg, i, ca, cb, cc, &pj, c3);
        const float ddelx = (float)(0.5 * cam.W), ddely = (float)(0.5 * cam.H);  // backward.cu:935-936
        const float hx = g2[0], hy = g2[1];
        g2[0] = -(ca * hx + cb * hy) * ddelx;
        g2[1] = -(cc * hy + cb * hx) * ddely;
        if constexpr (M2D1) {
            float hx1 = 0.f, hy1 = 0.f;
#pragma unroll
            for (int m = 0; m + 1 < INST_REC_MAX; m++)
                if (m == m1.o_m1) {
                    hx1 = acc[m];
                    hy1 = acc[m + 1];
                }
            m2d1[0] = -(ca * hx1 + cb * hy1) * ddelx;
            m2d1[1] = -(cc * hy1 + cb * hx1) * ddely;
        }
        g2[2] *= -0.5f;
        g2[3] *= -0.5f;
        g2[4] *= -0.5f;
        const unsigned clamped = g.shs ? geo.clamp[i] : 0u;  // (SH colour clamping; not stored without SH)
        gauss_chain(cam, g, gg, i, g2, clamped, dmean, dcov, dscale, drot, dsh, nsh, !POSE || pf.scols != 1, &pj, c3);
    }
    if constexpr (POSE) {
        // tracking: the pose sums of this Gaussian (track_transform_bwd_kernel's, gsr_glue.hip), then
        // one fixed-order workgroup sum, published; the last workgroup finishes the pose chain / Adam
        __shared__ float s_red[4 * POSE_PARTS];
        __shared__ float s_tot[POSE_PARTS];
        float v[POSE_PARTS];
#pragma unroll
        for (int k = 0; k < POSE_PARTS; k++) v[k] = 0.f;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        if (pf.scols != 1) {
            const Pose ps = s_pose;  // (c only: the same normalised quaternion)
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = ps.c[k];
        }
        if (live) {
            const float mci[3] = {gg.m.x, gg.m.y, gg.m.z};
            pose_partials_m(v, i, dmean, dcol2, pf.scols != 1 ? drot : nullptr, pf.means_world, pf.unnorm_rot, mci,
                            pf.w2c, c);
        }
        block_sum<POSE_PARTS>(v, s_red, s_tot);
        __syncthreads();
        float* const part = scratch_partials(pf.scratch);
        if (threadIdx.x < POSE_PARTS) st_agent(part + POSE_PARTS * blockIdx.x + threadIdx.x, s_tot[threadIdx.x]);
        if constexpr (kAblate == 3) return;  // timing ablation: no pose tail (invalid pose update)
        // Two-level fixed-order sum of the ~1200 workgroup partials: the last workgroup of each
        // of the 16 arrival groups (b = g mod 16) adds its group's partials (one per thread)
        // and publishes the group sum; the last group then adds the 16 group sums.  (One
        // workgroup reading all partials serially cost ~18 us more than the separate pose kernel.  A one-level
        // tail -- the last workgroup gathers all partials as one coalesced stream, 40 agent loads in flight per
        // thread: three serial memory round trips instead of six -- measured no faster, 6350-6367 against
        // 6379-6397 frames/s, and its other sum order put the config-5 trajectory at 5.3e-4 against the 5e-4
        // bound: profiles/r7k_ab_pose_finish_kernel.txt.)
        const int nb = gridDim.x;
        uint32_t* ctr = scratch_counters(pf.scratch);
        float* gsum = part + POSE_PARTS * nb;
        __shared__ uint32_t s_flag;
        const uint32_t g = (uint32_t)blockIdx.x & 15u;
        const uint32_t ngroups = nb < 16 ? (uint32_t)nb : 16u;
        __builtin_amdgcn_s_waitcnt(0x0F70);  // s_waitcnt vmcnt(0): the partial stores have landed
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t gsize = (uint32_t)nb / 16u + (g < (uint32_t)nb % 16u ? 1u : 0u);
            uint32_t* gc = ctr + ARRIVE_STRIDE * (1 + g);
            const bool last = __hip_atomic_fetch_add(gc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1;
            if (last) __hip_atomic_store(gc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_flag = last;
        }
        __syncthreads();
        if (!s_flag) return;
#pragma unroll
        for (int k = 0; k < POSE_PARTS; k++) v[k] = 0.f;
        for (int b = (int)g + 16 * threadIdx.x; b < nb; b += 16 * 256)
#pragma unroll
            for (int k = 0; k < POSE_PARTS; k++) v[k] += ld_agent(part + POSE_PARTS * b + k);
        __syncthreads();
        block_sum<POSE_PARTS>(v, s_red, s_tot);
        __syncthreads();
        if (threadIdx.x < POSE_PARTS) st_agent(gsum + POSE_PARTS * g + threadIdx.x, s_tot[threadIdx.x]);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (threadIdx.x == 0) {
            const bool last = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1;
            if (last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_flag = last;
        }
        __syncthreads();
        if (!s_flag) return;
#pragma unroll
        for (int k = 0; k < POSE_PARTS; k++) v[k] = threadIdx.x < ngroups ? ld_agent(gsum + POSE_PARTS * threadIdx.x + k) : 0.f;
        __syncthreads();
        block_sum<POSE_PARTS>(v, s_red, s_tot);
        __syncthreads();
        if (threadIdx.x == 0) {
            const PoseAdam adam{pf.lr_q, pf.lr_t, pf.beta1, pf.beta2, (float)(1.0 - pf.beta1),
                                (float)(1.0 - pf.beta2), (float)pf.eps, pf.adam_state, pf.cam_q, pf.cam_t,
                                pf.guard, pf.cap, pf.loss, pf.best};
            pose_fin(s_tot, pf.cam_q, pf.qs, pf.dq, pf.dt, adam);
        }
        return;
    }
    if (out.dmeans2D) {
        out.dmeans2D[3 * i] = g2[0];
        out.dmeans2D[3 * i + 1] = g2[1];
        out.dmeans2D[3 * i + 2] = 0.f;
    }
    if constexpr (M2D1) {
        m1.dmeans2D_c1[3 * i] = m2d1[0];
        m1.dmeans2D_c1[3 * i + 1] = m2d1[1];
        m1.dmeans2D_c1[3 * i + 2] = 0.f;
    }
    if (out.dcolors) {
        out.dcolors[3 * i] = g2[6];
        out.dcolors[3 * i + 1] = g2[7];
        out.dcolors[3 * i + 2] = g2[8];
    }
    if (out.dopacity) out.dopacity[i] = g2[5];
    if (out.dcolors2) {
        out.dcolors2[3 * i] = dcol2[0];
        out.dcolors2[3 * i + 1] = dcol2[1];
        out.dcolors2[3 * i + 2] = dcol2[2];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) out.dmeans3D[3 * i + k] = dmean[k];
    if (out.dcov3D)
#pragma unroll
        for (int k = 0; k < 6; k++) out.dcov3D[6 * i + k] = dcov[k];
    if (out.dscales)
#pragma unroll
        for (int k = 0; k < 3; k++) out.dscales[3 * i + k] = dscale[k];
    if (out.drot)
#pragma unroll
        for (int k = 0; k < 4; k++) out.drot[4 * i + k] = drot[k];
    if (SHL && out.dsh && g.M > 0) {
        float* d = out.dsh + (size_t)3 * g.M * i;
#pragma unroll
        for (int k = 0; k < 48; k++)
            if (k < 3 * g.M) d[k] = (k < 3 * nsh) ? dsh[k] : 0.f;
        for (int k = 48; k < 3 * g.M; k++) d[k] = 0.f;
    }
}
template <bool POSE, bool SHL, bool CLK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 5)))
gauss_bwd_kernel(Camera cam, GaussIn g, GeomPtrs geo, const int* __restrict__ radii, const float* __restrict__ inst,
                 RecLayout rec, GradsOut out, BwdGuard guard, PoseFuse pf, unsigned long long* clk) {
    if constexpr (CLK) kclock_begin(clk);
    gauss_bwd_body<POSE, SHL>(cam, g, geo, radii, inst, rec, out, guard, pf);
    if constexpr (CLK) kclock_end(clk);
}

template <bool SHL, bool CLK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 5)))
gauss_bwd_m2d_kernel(Camera cam, GaussIn g, GeomPtrs geo, const int* __restrict__ radii, const float* __restrict__ inst,
                     RecLayout rec, GradsOut out, M2dOut m1, BwdGuard guard, unsigned long long* clk) {
    if constexpr (CLK) kclock_begin(clk);
    gauss_bwd_body<false, SHL, true>(cam, g, geo, radii, inst, rec, out, guard, PoseFuse{}, m1);
    if constexpr (CLK) kclock_end(clk);
}

struct PickGaussBwd {
    template <bool POSE, bool SHL, bool CLK>
    auto operator()() const { return &gauss_bwd_kernel<POSE, SHL, CLK>; }
};
struct PickGaussBwdM2d {
    template <bool SHL, bool CLK>
    auto operator()() const { return &gauss_bwd_m2d_kernel<SHL, CLK>; }
};

// arrival counters, workgroup partials, the 16 group sums
int pose_fuse_scratch_floats(int P) { return POSE_PARTS * ((P + 255) / 256) + ARRIVE_GROUPED_WORDS + 16 * POSE_PARTS; }

hipError_t launch_gauss_bwd(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii, const float* inst,
                            RecLayout rec, const GradsOut& out, BwdGuard guard, hipStream_t s, const PoseFuse* pose,
                            unsigned long long* clk) {
    if (g.P == 0) return hipSuccess;
    const auto k = dispatch_bools(PickGaussBwd{}, pose != nullptr, g.shs != nullptr, clk != nullptr);
    hipLaunchKernelGGL(k, dim3((g.P + 255) / 256), dim3(256), 0, s, cam, g, geo, radii, inst, rec, out, guard,
                       pose ? *pose : PoseFuse{}, clk);
    return hipGetLastError();
}

hipError_t launch_gauss_bwd_m2d(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii, const float* inst,
                                RecLayout rec, const GradsOut& out, M2dOut m1, BwdGuard guard, hipStream_t s,
                                unsigned long long* clk) {
    if (g.P == 0) return hipSuccess;
    const auto k = dispatch_bools(PickGaussBwdM2d{}, g.shs != nullptr, clk != nullptr);
    hipLaunchKernelGGL(k, dim3((g.P + 255) / 256), dim3(256), 0, s, cam, g, geo, radii, inst, rec, out, m1, guard, clk);
    return hipGetLastError();
}

// ------------------------------------------------------------- self-test --
// Checks the permlane/DPP row mapping of wave_reduce9 on the hardware:
// in[64*9] (lane-major) -> out[9] wave totals.
__global__ void selftest_reduce9_kernel(const float* in, float* out) {
    const int lane = threadIdx.x;
    float v[9];
#pragma unroll
    for (int q = 0; q < 9; q++) v[q] = in[lane * 9 + q];
    float r0, r1, r8;
    wave_reduce9(v, r0, r1, r8);
    if ((lane & 15) == 0) {
        const int row = lane >> 4, sl = reduce9_slot_r0(row);
        out[sl] = r0;
        out[4 + sl] = r1;
        if (row == 0) out[8] = r8;
    }
}

hipError_t launch_selftest_reduce9(const float* in, float* out, hipStream_t s) {
    hipLaunchKernelGGL(selftest_reduce9_kernel, dim3(1), dim3(64), 0, s, in, out);
    return hipGetLastError();
}

#if GSR_STEPSTAT
extern "C" int gsr_diag_stepstat_bwd(unsigned long long* host) {  // copies and clears the counters
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stepstat), sizeof(g_stepstat), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stepstat), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#endif
#if GSR_PHASE
extern "C" int gsr_diag_phase_bwd(unsigned long long* host) {  // copies and clears the phase cycles
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase), sizeof(g_phase), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#endif
#if GSR_WGTIME
extern "C" int gsr_diag_wgtime_bwd(unsigned long long* host, int n) {
    const size_t bytes = sizeof(unsigned long long) * 4 * (size_t)(n < GSR_WGTIME_MAX ? n : GSR_WGTIME_MAX);
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wgtime), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace gsr
