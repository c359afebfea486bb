// gsr_preprocess.hip -- the forward's first stage (preprocessCUDA, forward.cu:155-256): one lane per Gaussian
// projects it, writes its render record, rect and live-tile mask, and counts its instances per tile; and
// markVisible's frustum test (checkFrustum, rasterizer_impl.cu:54-66).  The pipeline's map is at the top of gsr_forward.hip.
#include "gsr_clock.h"
#include "gsr_dispatch.h"
#include "gsr_glue_common.h"  // track_xform_compute / _store: the transform-fused preprocess
#include "gsr_launch.h"
#include "gsr_layout.h"
#include "gsr_math.h"
#include "gsr_wave.h"

namespace gsr {

// ------------------------------------------------------------- preprocess --
// LDS_HIST: per-tile instance counts go to a workgroup histogram in LDS and
// leave as one row of the [workgroup x tile] matrix `counts` (no global
// atomics: ~680k scattered global atomics cost ~30 us on MI355X whatever their
// contention, tools/micro/atomics.hip).  Otherwise: global atomics on padded
// per-tile counters (fallback for > MAX_LDS_TILES tiles).
// XF: SplaTAM's tracking transform fused in (g.xf, TrackXf): the camera-frame rendervars are
// formed here from the world-frame map and the pose, and stored to g's arrays for the backward.
// CLK: the in-kernel stage clock (a separate instantiation: the production launches carry none of it)
// EXACT: the per-workgroup culled-instance counts of the dynamic forward's exact list tail (Camera::tail_exact);
// a separate instantiation because the bookkeeping, even skipped at run time, cost the static mapping
// preprocess 45 -> 58 us in code generation (profiles/r9y_ab_preprocess_tail.txt)
template <bool LDS_HIST, bool XF, bool CLK, bool EXACT>
__global__ void __launch_bounds__(PRE_BLOCK)
preprocess_kernel(Camera cam, GaussIn g, GeomPtrs geo, int* radii, uint32_t* __restrict__ counts, int ntiles,
                  unsigned long long* clk) {
#pragma clang fp contract(off)
    if (cam.gate.off()) return;
    if constexpr (CLK) kclock_begin(clk);  // (stage clock: first workgroup's start to the last one's end)
    extern __shared__ uint32_t s_hist[];
    __shared__ float s_pose[16];  // XF: the frame's pose (R 9, t 3, F.normalize(q) 4), formed once by wave 0
    const int i = (blockIdx.x << cam.pre_shift) + threadIdx.x;  // blockDim.x = 1 << pre_shift
    XfRaw xr{};  // XF: the Gaussian's transform inputs, in flight while wave 0 forms the pose
    if (XF && i < g.P) xr = track_xform_load(g.xf, i, true);
    // the per-Gaussian inputs used only once the rect is known (colour, opacity, second colour set)
    // are loaded here too, not after the projection: one memory round trip fewer per workgroup
    // (not in the transform-fused tracking form, where the early loads measured 0.6 us slower)
    float pre_rgb[3] = {0.f, 0.f, 0.f}, pre_c2[3] = {0.f, 0.f, 0.f}, pre_op = 0.f;
    if (!XF && i < g.P) {
        if (g.colors) {
            pre_rgb[0] = g.colors[3 * i]; pre_rgb[1] = g.colors[3 * i + 1]; pre_rgb[2] = g.colors[3 * i + 2];
        } else if (g.sh_staged) {  // sh_eval_kernel wrote rgb (in bin[i], overwritten below) and the clamp bits
            const uint4 c = geo.bin[i];
            pre_rgb[0] = __uint_as_float(c.x); pre_rgb[1] = __uint_as_float(c.y); pre_rgb[2] = __uint_as_float(c.z);
        }
        pre_op = g.opacities[i];
        if (g.colors2) {
            pre_c2[0] = g.colors2[3 * i]; pre_c2[1] = g.colors2[3 * i + 1]; pre_c2[2] = g.colors2[3 * i + 2];
        }
    }
    if (XF && threadIdx.x < 64) {
        const Pose ps = make_pose(g.xf.cq, g.xf.ct, g.xf.qs);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) s_pose[k] = ps.R[k / 3][k % 3];
#pragma unroll
            for (int k = 0; k < 3; k++) s_pose[9 + k] = ps.t[k];
#pragma unroll
            for (int k = 0; k < 4; k++) s_pose[12 + k] = ps.c[k];
        }
    }
    if (LDS_HIST)
        for (int t = threadIdx.x; t < ntiles; t += blockDim.x) s_hist[t] = 0u;
    if (LDS_HIST || XF) __syncthreads();
    if (i == 0) geo.counters[4] = 0u;  // tile_colscan_kernel's arrival counter (next launch)
    uint32_t tiles = 0, culled = 0;  // culled: rect tiles left out of the lists (Camera::cull)
    bool violation = false;  // prefiltered set but the point is culled (auxiliary.h:154-160)
    float4 q0, q1, q2, q3;
    if (i < g.P) {
        int radius = 0;
        float3 p;
        float xs[3], xc2[3], xop = 0.f;
        float4 xq;
        if (XF) {  // gsr_track_transform_fwd's outputs, formed in registers (and stored for the backward)
            Pose ps;  // (track_xform_compute reads R, t and c)
#pragma unroll
            for (int k = 0; k < 9; k++) ps.R[k / 3][k % 3] = s_pose[k];
#pragma unroll
            for (int k = 0; k < 3; k++) ps.t[k] = s_pose[9 + k];
#pragma unroll
            for (int k = 0; k < 4; k++) ps.c[k] = s_pose[12 + k];
            float m[3];
            track_xform_compute_raw(g.xf, xr, ps, m, xq, xc2, xop, xs);  // (stored below, after every load)
            p = make_float3(m[0], m[1], m[2]);
        } else {
            p = make_float3(g.means3D[3 * i], g.means3D[3 * i + 1], g.means3D[3 * i + 2]);
        }
        float4 hom = xform4x4(p, cam.proj);
        float pw = 1.0f / (hom.w + 0.0000001f);
        float3 pv = xform4x3(p, cam.view);
        bool ok = pv.z > 0.001f;  // auxiliary.h:154 (the 1.3 NDC test is commented out)
        if (!ok && cam.prefiltered) violation = true;
        // a pruned Gaussian (alive mask, prune_gaussians inside a captured mapping frame) is culled like one
        // behind the camera: radius 0, no instances, zero gradients -- the survivors render and
        // differentiate exactly as after remove_points (utils/slam_external.py:141-163)
        if (g.alive != nullptr && g.alive[i] == 0) ok = false;
        float cov3[6];
        Proj pj;
        float det = 0.f, ca = 0.f, cb = 0.f, cc = 0.f;
        if (ok) {
            if (g.cov3D) {
#pragma unroll
                for (int k = 0; k < 6; k++) cov3[k] = g.cov3D[6 * i + k];
            } else {
                float3 s = XF ? make_float3(xs[0], xs[1], xs[2])
                              : make_float3(g.scales[3 * i], g.scales[3 * i + 1], g.scales[3 * i + 2]);
                float4 q = XF ? xq : make_float4(g.rotations[4 * i], g.rotations[4 * i + 1], g.rotations[4 * i + 2],
                                                 g.rotations[4 * i + 3]);
                cov3d_fwd(s, cam.scale_modifier, q, cov3);
            }
            cov2d_fwd(p, cam.focal_x, cam.focal_y, cam.tan_fovx, cam.tan_fovy, cov3, cam.view, pj);
            det = conic_of(pj, ca, cb, cc);
            ok = det != 0.0f;
        }
        if (ok) {
            float mid = 0.5f * (pj.a + pj.c);
            float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
            float l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
            float rad = ceilf(3.f * sqrtf(fmaxf(l1, l2)));
            float px = ndc2pix(hom.x * pw, cam.W), py = ndc2pix(hom.y * pw, cam.H);
            int x0, y0, x1, y1;
            get_rect(px, py, (int)rad, cam.gx, cam.gy, x0, y0, x1, y1);
            tiles = (uint32_t)((x1 - x0) * (y1 - y0));
            if (tiles != 0) {
                float rgb[3] = {pre_rgb[0], pre_rgb[1], pre_rgb[2]};
                unsigned clamped = 0;
                if (XF && g.colors) {
                    rgb[0] = g.colors[3 * i]; rgb[1] = g.colors[3 * i + 1]; rgb[2] = g.colors[3 * i + 2];
                } else if (XF && g.sh_staged) {
                    const uint4 c = geo.bin[i];
                    rgb[0] = __uint_as_float(c.x); rgb[1] = __uint_as_float(c.y); rgb[2] = __uint_as_float(c.z);
                } else if (!g.colors && !g.sh_staged) {
                    sh_fwd(cam.sh_degree, p, cam.campos, g.shs + (size_t)3 * g.M * i, rgb, clamped);
                }
                radius = (int)rad;
                float c2[3] = {0.f, 0.f, 0.f};
                if (XF) {
                    c2[0] = xc2[0]; c2[1] = xc2[1]; c2[2] = xc2[2];
                } else if (g.colors2) {
                    c2[0] = pre_c2[0]; c2[1] = pre_c2[1]; c2[2] = pre_c2[2];
                }
                const uint32_t rlo = (uint32_t)x0 | ((uint32_t)y0 << 16), rhi = (uint32_t)x1 | ((uint32_t)y1 << 16);
                q0 = make_float4(px, py, K_AC * ca, K_AC * cc);  // render-record conic form
                q2 = make_float4(rgb[0], rgb[1], rgb[2], __uint_as_float(rlo));
                q3 = make_float4(c2[0], c2[1], c2[2], __uint_as_float(rhi));
                if (XF) {  // (tracking form: three quarters now, q1 after the scan measured 0.7 us faster)
                    float4* rr = geo.rr + (size_t)RR_F4 * i;
                    rr[0] = q0;
                    rr[2] = q2;
                    rr[3] = q3;
                }
                q1 = make_float4(K_B * cb, XF ? xop : pre_op, pv.z, 0.f);  // .w: workgroup-local instance offset, below
                // live-tile mask (Camera::cull): the render's own conservative block-mask test per rect tile
                uint32_t live = 0xFFFFFFFFu;
                if (cam.cull && tiles <= 32u) {
                    const MaskGeom mg = mask_geom(q0, q1);
                    live = 0u;
                    for (int ty = y0, k = 0; ty < y1; ty++)
                        for (int tx = x0; tx < x1; tx++, k++)
                            live |= tile_reached(mg, (float)(tx * TILE_X), (float)(ty * TILE_Y)) ? 1u << k : 0u;
                }
                if constexpr (EXACT) culled = culled_below(live, tiles);
                geo.bin[i] = make_uint4(rlo, rhi, __float_as_uint(pv.z), live);
                if (!g.sh_staged && !g.colors) geo.clamp[i] = clamped;  // (read only by the SH backward)
                for (int ty = y0, k = 0; ty < y1; ty++)  // per-tile instance counts -> bucket ranges
                    for (int tx = x0; tx < x1; tx++, k++) {
                        if (!tile_live(live, (uint32_t)k)) continue;
                        if (LDS_HIST) atomicAdd(&s_hist[ty * cam.gx + tx], 1u);
                        else atomicAdd(&counts[(ty * cam.gx + tx) * TILE_CTR_STRIDE], 1u);
                    }
            }
        }
        radii[i] = radius;
        geo.tiles[i] = tiles;
        if (tiles == 0) geo.bin[i] = make_uint4(0u, 0u, 0u, 0u);
        if (XF && g.xf.store) {  // the rendervars for the backward (the same values as gsr_track_transform_fwd's)
            const float m[3] = {p.x, p.y, p.z};
            track_xform_store(i, m, xq, xc2, xop, xs, const_cast<float*>(g.means3D), const_cast<float*>(g.rotations),
                              const_cast<float*>(g.colors2), const_cast<float*>(g.opacities),
                              const_cast<float*>(g.scales));
        }
    }
    // workgroup scan of tiles touched: the local instance offset goes into the render
    // record (q1.w; the render kernels add the scanned workgroup base, blocksums[i >> pre_shift]),
    // the workgroup total into wgsum (input of the two-level scan)
    __shared__ uint32_t wsum[PRE_BLOCK / 64], wcul[PRE_BLOCK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = wave_incl_scan(tiles);
    if (lane == 63) wsum[wv] = incl;
    if constexpr (EXACT) {  // the workgroup's culled instances (the exact tail, duplicate)
        const uint32_t cincl = wave_incl_scan(culled);
        if (lane == 63) wcul[wv] = cincl;
    }
    __syncthreads();
    uint32_t woff = 0;
    for (int k = 0; k < wv; k++) woff += wsum[k];
    if (tiles) {
        q1.w = __uint_as_float(woff + incl - tiles);
        float4* rr = geo.rr + (size_t)RR_F4 * i;
        if (!XF) {  // the whole 64-B record in one go, one full line (two partial writes of the line took
            rr[0] = q0;  // mapping's preprocess 49.7 us, this 41.5)
            rr[2] = q2;
            rr[3] = q3;
        }
        rr[1] = q1;
    }
    // top bit: prefiltered violation anywhere in the workgroup (folded into counters[1] by the scan)
    const bool viol = __syncthreads_or(violation);
    if (threadIdx.x == blockDim.x - 1) {
        geo.wgsum[blockIdx.x] = (woff + incl) | (viol ? 0x80000000u : 0u);
        if constexpr (EXACT) {
            uint32_t cw = 0;
            for (int k = 0; k < (int)(blockDim.x >> 6); k++) cw += wcul[k];
            geo.wgcull[blockIdx.x] = cw;
        }
    }
    if (LDS_HIST)
        for (int t = threadIdx.x; t < ntiles; t += blockDim.x) counts[(size_t)blockIdx.x * ntiles + t] = s_hist[t];
    if constexpr (CLK) kclock_end(clk);
}

// The 12 forms: the transform-fused one is static-only, so it never carries the exact tail's bookkeeping
struct PickPreprocess {
    template <bool LDS_HIST, bool XF, bool CLK, bool EXACT>
    auto operator()() const { return &preprocess_kernel<LDS_HIST, XF, CLK, EXACT && !XF>; }
};

hipError_t launch_preprocess(const Camera& cam, const GaussIn& g, GeomPtrs geo, int* radii, uint32_t* counts,
                             bool lds_hist, int ntiles, int nb, hipStream_t s, unsigned long long* clk) {
    if (nb == 0) return hipSuccess;
    const bool xf = g.xf.mw != nullptr;
    const bool exact = cam.tail_exact && cam.cull && !xf;
    const auto k = dispatch_bools(PickPreprocess{}, lds_hist, xf, clk != nullptr, exact);
    hipLaunchKernelGGL(k, dim3(nb), dim3(1 << cam.pre_shift), lds_hist ? sizeof(uint32_t) * ntiles : 0, s, cam, g,
                       geo, radii, counts, ntiles, clk);
    return hipGetLastError();
}

// ----------------------------------------------------------- mark visible --
__global__ void mark_visible_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ view,
                                    uint8_t* __restrict__ vis) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    vis[i] = xform4x3(p, view).z > 0.001f ? 1 : 0;
}

hipError_t launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* vis, hipStream_t s) {
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, vis);
    return hipGetLastError();
}

}  // namespace gsr
