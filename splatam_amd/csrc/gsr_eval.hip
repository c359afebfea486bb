// gsr_eval.hip -- the per-frame metrics of SplaTAM's eval() (utils/eval_helpers.py:466-512) on the device,
// without a host read (include/gsr_glue.h: gsr_eval_frame): PSNR, MS-SSIM, the two depth columns, n_valid and
// the per-channel MSE of one rendered frame against its capture, written into one 8-float row.  One launch
// for the pixel metrics plus, with MS-SSIM, one launch per pyramid level (six in all; no combine launch):
//
//   eval_pixel_kernel  a grid-stride pass over the H*W pixels: the masks, the three channels' squared
//                      errors, the two depth sums and the valid count; the last workgroup to arrive sums the
//                      workgroups' partials in a fixed order and writes every column but MS-SSIM's.
//   eval_level_kernel  one workgroup per 32x16 tile of a level's valid output and channel: the haloed 42x26
//                      tile of both images into LDS (level 0 applies the mask while loading), the 2x2 average
//                      pool of the rows / columns the tile owns to the next level's images, the 11-tap pass
//                      along H for the five moments (X, Y, XX, YY, XY) into LDS, the pass along W, the cs /
//                      ssim maps and their sums over the tile; the last workgroup to arrive sums the tiles in a
//                      fixed order into the level's per-channel means, and at level 4 forms the product over
//                      the levels and writes the MS-SSIM column.
//
// Latency-bound work (a 320x240 frame: 450 tiles at level 0), so the aim is few launches and no host read.
// Precision: every per-pixel operation of the reference is done as the reference does it, in float32, each
// rounded on its own (masking, differences, squares, the pooled images); every SUM -- the reductions over the
// image and the window's weighted moments, where sigma^2 = E[x^2] - mu^2 cancels -- is accumulated in float64
// (gfx950 issues fp64 FMAs at half the fp32 rate, and this is a few MFLOP) and rounded to float32 once, in
// the row.  Sums run in a fixed order (lane tree, wave order, workgroup order): no float atomics, the same
// bits on every run.
#include <math.h>

#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_errors.h"
#include "gsr_layout.h"
#include "gsr_wave.h"

namespace gsr {
namespace {

constexpr int EV_BLOCK = 256;
constexpr int EV_WAVES = EV_BLOCK / 64;
constexpr int EV_PIX_MAX_BLOCKS = 512;  // the pixel pass's grid bound (larger images stride)
constexpr int EV_PIX_VALS = 6;          // se_r, se_g, se_b, depth_rmse sum, depth_l1 sum, n_valid
constexpr int EV_TAPS = 11, EV_HALO = EV_TAPS - 1;
constexpr int EV_TW = 32, EV_TH = 16;   // a workgroup's tile of the valid output
constexpr int EV_IW = EV_TW + EV_HALO, EV_IH = EV_TH + EV_HALO;
constexpr int EV_LEVELS = 5;
constexpr int EV_MIN_SIDE = 161;        // (min(H, W) - 1) / 2^4 > 10: the last level still holds a window
// workspace: words [0] the pixel pass's arrival counter, [1] the pyramid's (both zero between calls; the
// first EV_HEAD_BYTES hold nothing else), then the levels' means, the pixel partials, the tiles' partials
// and the pooled images of levels 1 .. 4
constexpr size_t EV_HEAD_BYTES = 128;

struct EvWin {
    double g[EV_TAPS];
};

struct EvLayout {
    int h[EV_LEVELS], w[EV_LEVELS];
    size_t lvl, pix, part, img[EV_LEVELS];  // byte offsets (img[l]: X of level l, its Y follows; img[0] unused)
    size_t total;
    static EvLayout make(int H, int W, bool ms) {
        EvLayout l{};
        size_t o = EV_HEAD_BYTES;
        l.lvl = o; o = align_up(o + 8 * (size_t)(EV_LEVELS * 6), 128);
        l.pix = o; o = align_up(o + 8 * (size_t)(EV_PIX_MAX_BLOCKS * EV_PIX_VALS), 128);
        l.part = o;
        l.h[0] = H; l.w[0] = W;
        for (int k = 1; k < EV_LEVELS; k++) { l.h[k] = (l.h[k - 1] + 1) / 2; l.w[k] = (l.w[k - 1] + 1) / 2; }
        if (ms) {
            const size_t ntiles = (size_t)((W - EV_HALO + EV_TW - 1) / EV_TW) * ((H - EV_HALO + EV_TH - 1) / EV_TH);
            o = align_up(o + 8 * 2 * 3 * ntiles, 128);
            for (int k = 1; k < EV_LEVELS; k++) {
                l.img[k] = o;
                o = align_up(o + 4 * 2 * 3 * (size_t)l.h[k] * l.w[k], 128);
            }
        }
        l.total = o;
        return l;
    }
};

// Sums v over the workgroup in a fixed order (each wave's lane tree, then the four waves); every thread
// returns with the sums in v.  s_red: EV_WAVES * N doubles, free again after the call.
template <int N>
__device__ __forceinline__ void block_sum_d(double (&v)[N], double* s_red) {
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v[k] += __shfl_down(v[k], d, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();  // (an earlier call's readers are done with s_red)
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < N; k++) s_red[w * N + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = (s_red[k] + s_red[N + k]) + (s_red[2 * N + k] + s_red[3 * N + k]);
}

struct EvPix {
    int HW;
    const float *im, *depth_sil, *gt_im, *gt_depth;
    float sil_thres;
    int use_sil, ms_ssim;
    uint32_t* counter;
    double* part;
    float* row;
};

__global__ void __launch_bounds__(EV_BLOCK) eval_pixel_kernel(EvPix a) {
#pragma clang fp contract(off)
    __shared__ double s_red[EV_WAVES * EV_PIX_VALS];
    const int tid = threadIdx.x, HW = a.HW;
    double v[EV_PIX_VALS] = {0., 0., 0., 0., 0., 0.};
    for (long long p = (long long)blockIdx.x * EV_BLOCK + tid; p < HW; p += (long long)gridDim.x * EV_BLOCK) {
        const float gd = a.gt_depth[p];
        const float valid = gd > 0.f ? 1.f : 0.f;
        const float pres = a.depth_sil[(size_t)HW + p] > a.sil_thres ? 1.f : 0.f;
        const float m = a.use_sil ? pres * valid : valid;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float d = a.im[(size_t)c * HW + p] * m - a.gt_im[(size_t)c * HW + p] * m;
            v[c] += (double)(d * d);
        }
        float diff = a.depth_sil[p] * valid - gd;
        if (a.use_sil) diff = diff * pres;
        v[3] += (double)(sqrtf(diff * diff) * valid);
        v[4] += (double)(fabsf(diff) * valid);
        v[5] += (double)valid;  // (a count: exact)
    }
    block_sum_d(v, s_red);
    if (tid < EV_PIX_VALS) st_agent(a.part + (size_t)blockIdx.x * EV_PIX_VALS + tid, v[tid]);
    if (!last_block_arrive(a.counter)) return;
    const int nb = gridDim.x;
#pragma unroll
    for (int k = 0; k < EV_PIX_VALS; k++) v[k] = 0.;
    for (int b = tid; b < nb; b += EV_BLOCK)
#pragma unroll
        for (int k = 0; k < EV_PIX_VALS; k++) v[k] += ld_agent(a.part + (size_t)b * EV_PIX_VALS + k);
    block_sum_d(v, s_red);
    if (tid == 0) {
        double psnr = 0.;
        float mse[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double ms = v[c] / (double)HW;
            psnr += 20. * log10(1. / sqrt(ms));
            mse[c] = (float)ms;
        }
        a.row[0] = (float)(psnr / 3.);
        if (!a.ms_ssim) a.row[1] = __builtin_nanf("");
        a.row[2] = (float)(v[3] / v[5]);
        a.row[3] = (float)(v[4] / v[5]);
        a.row[4] = (float)v[5];
        a.row[5] = mse[0]; a.row[6] = mse[1]; a.row[7] = mse[2];
    }
}

struct EvLevel {
    int H, W, level;            // this level's extent
    const float *x, *y;         // [3,H,W] each (level 0: im, gt_im)
    const float *depth_sil, *gt_depth;  // level 0's mask
    float sil_thres;
    int use_sil;
    float *nx, *ny;             // the next level's images [3,Hn,Wn] (nullptr at the last level)
    int Hn, Wn;
    uint32_t* counter;
    double *part, *lvl;
    float* row;
    EvWin win;
};

__device__ __forceinline__ double ev_relu(double v) { return v > 0. ? v : (v != v ? v : 0.); }  // torch.relu keeps NaN

template <bool MASKED>
__global__ void __launch_bounds__(EV_BLOCK) eval_level_kernel(EvLevel a) {
    __shared__ float s_x[EV_IH][EV_IW], s_y[EV_IH][EV_IW];
    __shared__ double s_v[5][EV_TH][EV_IW];
    __shared__ double s_red[EV_WAVES * 6];
    const int tid = threadIdx.x, H = a.H, W = a.W;
    const int ch = blockIdx.z, r0 = blockIdx.y * EV_TH, c0 = blockIdx.x * EV_TW;
    const int Ho = H - EV_HALO, Wo = W - EV_HALO;
    const size_t plane = (size_t)H * W;
    // ---- the haloed tile (zero outside the image; no counted output reads those)
    for (int i = tid; i < EV_IH * EV_IW; i += EV_BLOCK) {
        const int ly = i / EV_IW, lx = i - ly * EV_IW, gy = r0 + ly, gx = c0 + lx;
        float xv = 0.f, yv = 0.f;
        if (gy < H && gx < W) {
            const size_t p = (size_t)gy * W + gx;
            xv = a.x[ch * plane + p];
            yv = a.y[ch * plane + p];
            if (MASKED) {
                const float valid = a.gt_depth[p] > 0.f ? 1.f : 0.f;
                const float pres = a.depth_sil[plane + p] > a.sil_thres ? 1.f : 0.f;
                const float m = a.use_sil ? pres * valid : valid;
                xv = xv * m;
                yv = yv * m;
            }
        }
        s_x[ly][lx] = xv;
        s_y[ly][lx] = yv;
    }
    __syncthreads();
    // ---- avg_pool2d(2, 2, padding = extent % 2, zero pad counted): the pooled pixels whose window starts
    //      (clamped to 0) in the rows / columns this tile owns -- [r0, r0 + 16) x [c0, c0 + 32), the last tile
    //      of an axis to the image's end (at most 26 / 42: inside the halo)
    if (a.nx) {
        const int pr = H & 1, pc = W & 1;
        const int r1 = blockIdx.y == gridDim.y - 1 ? H : r0 + EV_TH, c1 = blockIdx.x == gridDim.x - 1 ? W : c0 + EV_TW;
        const int py0 = r0 == 0 ? 0 : (r0 + pr + 1) / 2, py1 = (r1 + pr + 1) / 2;
        const int px0 = c0 == 0 ? 0 : (c0 + pc + 1) / 2, px1 = (c1 + pc + 1) / 2;
        const int nw = px1 - px0, n = (py1 - py0) * nw;
        const size_t nplane = (size_t)a.Hn * a.Wn;
        for (int i = tid; i < n; i += EV_BLOCK) {
            const int py = py0 + i / nw, px = px0 + i % nw;
            const int ya = 2 * py - pr - r0, xa = 2 * px - pc - c0;  // local; -1: the zero pad (tile 0 only)
            double sx = 0., sy = 0.;
#pragma unroll
            for (int dy = 0; dy < 2; dy++)
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int yy = ya + dy, xx = xa + dx;
                    if (yy >= 0 && xx >= 0) {
                        sx += (double)s_x[yy][xx];
                        sy += (double)s_y[yy][xx];
                    }
                }
            a.nx[ch * nplane + (size_t)py * a.Wn + px] = (float)(0.25 * sx);
            a.ny[ch * nplane + (size_t)py * a.Wn + px] = (float)(0.25 * sy);
        }
    }
    // ---- the 11 taps along H: five moments for 16 rows x 42 columns
    for (int i = tid; i < EV_TH * EV_IW; i += EV_BLOCK) {
        const int r = i / EV_IW, c = i - r * EV_IW;
        double m0 = 0., m1 = 0., m2 = 0., m3 = 0., m4 = 0.;
#pragma unroll
        for (int k = 0; k < EV_TAPS; k++) {
            const double g = a.win.g[k], xv = (double)s_x[r + k][c], yv = (double)s_y[r + k][c];
            m0 = fma(g, xv, m0);
            m1 = fma(g, yv, m1);
            m2 = fma(g, xv * xv, m2);  // (products of two float32 values: exact in float64)
            m3 = fma(g, yv * yv, m3);
            m4 = fma(g, xv * yv, m4);
        }
        s_v[0][r][c] = m0; s_v[1][r][c] = m1; s_v[2][r][c] = m2; s_v[3][r][c] = m3; s_v[4][r][c] = m4;
    }
    __syncthreads();
    // ---- the 11 taps along W, the maps, the tile's sums
    double sums[2] = {0., 0.};
    for (int o = tid; o < EV_TH * EV_TW; o += EV_BLOCK) {
        const int r = o / EV_TW, c = o - r * EV_TW;
        if (r0 + r >= Ho || c0 + c >= Wo) continue;
        double m[5] = {0., 0., 0., 0., 0.};
#pragma unroll
        for (int k = 0; k < EV_TAPS; k++) {
            const double g = a.win.g[k];
#pragma unroll
            for (int q = 0; q < 5; q++) m[q] = fma(g, s_v[q][r][c + k], m[q]);
        }
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        const double mu1 = m[0], mu2 = m[1];
        const double s1 = m[2] - mu1 * mu1, s2 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
        const double cs = (2. * s12 + C2) / (s1 + s2 + C2);
        sums[0] += cs;
        sums[1] += (2. * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs;
    }
    block_sum_d(sums, s_red);
    const size_t ntile = (size_t)gridDim.x * gridDim.y;
    const size_t b = ch * ntile + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (tid < 2) st_agent(a.part + 2 * b + tid, sums[tid]);
    if (!last_block_arrive(a.counter)) return;
    // ---- last workgroup: the level's means per channel, tiles summed in index order
    double t[6] = {0., 0., 0., 0., 0., 0.};
    for (size_t i = tid; i < ntile; i += EV_BLOCK)
#pragma unroll
        for (int k = 0; k < 6; k++) t[k] += ld_agent(a.part + 2 * ((k >> 1) * ntile + i) + (k & 1));
    block_sum_d(t, s_red);
    if (tid != 0) return;
    const double cnt = (double)Ho * (double)Wo;
#pragma unroll
    for (int k = 0; k < 6; k++) a.lvl[6 * a.level + k] = t[k] / cnt;  // [level][channel][cs, ssim]
    if (a.level != EV_LEVELS - 1) return;
    const double wl[EV_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    double acc = 0.;
    for (int c = 0; c < 3; c++) {
        double p = pow(ev_relu(t[2 * c + 1] / cnt), wl[EV_LEVELS - 1]);
        for (int l = 0; l < EV_LEVELS - 1; l++) p *= pow(ev_relu(a.lvl[6 * l + 2 * c]), wl[l]);
        acc += p;
    }
    a.row[1] = (float)(acc / 3.);
}

EvWin make_window() {
    EvWin w;
    double s = 0.;
    for (int k = 0; k < EV_TAPS; k++) {
        w.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2. * 1.5 * 1.5));
        s += w.g[k];
    }
    for (int k = 0; k < EV_TAPS; k++) w.g[k] /= s;
    return w;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_eval_workspace_bytes(int H, int W, int ms_ssim) {
    if (!image_size_ok(H, W)) return 0;
    if (ms_ssim && (H < EV_MIN_SIDE || W < EV_MIN_SIDE)) return 0;
    return EvLayout::make(H, W, ms_ssim != 0).total;
}

int gsr_eval_frame(int H, int W, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                   float sil_thres, int use_sil_mask, int ms_ssim, void* workspace, float* row, void* stream) {
    if (!image_size_ok(H, W)) return fail(GSR_ERR_INVALID_ARG, "eval_frame: bad image size");
    if (ms_ssim && (H < EV_MIN_SIDE || W < EV_MIN_SIDE))
        return fail(GSR_ERR_INVALID_ARG, "eval_frame: MS-SSIM is defined for min(H, W) > 160 only (ms_ssim = 0 skips it)");
    if (!im || !depth_sil || !gt_im || !gt_depth || !workspace || !row)
        return fail(GSR_ERR_INVALID_ARG, "eval_frame: null pointer");
    if (!aligned16(workspace)) return fail(GSR_ERR_INVALID_ARG, "eval_frame: workspace must be 16-byte aligned");
    const EvLayout lay = EvLayout::make(H, W, ms_ssim != 0);
    char* const ws = (char*)workspace;
    uint32_t* const counters = (uint32_t*)ws;
    const hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    EvPix p{HW, im, depth_sil, gt_im, gt_depth, sil_thres, use_sil_mask, ms_ssim, counters + 0, (double*)(ws + lay.pix), row};
    const int nb = HW > EV_PIX_MAX_BLOCKS * EV_BLOCK ? EV_PIX_MAX_BLOCKS : (HW + EV_BLOCK - 1) / EV_BLOCK;
    hipLaunchKernelGGL(eval_pixel_kernel, dim3(nb), dim3(EV_BLOCK), 0, st, p);
    if (ms_ssim) {
        static const EvWin win = make_window();
        for (int l = 0; l < EV_LEVELS; l++) {
            EvLevel a{};
            a.H = lay.h[l]; a.W = lay.w[l]; a.level = l;
            if (l == 0) {
                a.x = im; a.y = gt_im;
            } else {
                a.x = (const float*)(ws + lay.img[l]);
                a.y = a.x + 3 * (size_t)a.H * a.W;
            }
            a.depth_sil = depth_sil; a.gt_depth = gt_depth; a.sil_thres = sil_thres; a.use_sil = use_sil_mask;
            if (l + 1 < EV_LEVELS) {
                a.Hn = lay.h[l + 1]; a.Wn = lay.w[l + 1];
                a.nx = (float*)(ws + lay.img[l + 1]);
                a.ny = a.nx + 3 * (size_t)a.Hn * a.Wn;
            }
            a.counter = counters + 1;
            a.part = (double*)(ws + lay.part);
            a.lvl = (double*)(ws + lay.lvl);
            a.row = row;
            a.win = win;
            const dim3 grid((a.W - EV_HALO + EV_TW - 1) / EV_TW, (a.H - EV_HALO + EV_TH - 1) / EV_TH, 3);
            if (l == 0)
                hipLaunchKernelGGL(eval_level_kernel<true>, grid, dim3(EV_BLOCK), 0, st, a);
            else
                hipLaunchKernelGGL(eval_level_kernel<false>, grid, dim3(EV_BLOCK), 0, st, a);
        }
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, "eval_frame");
}

}  // extern "C"
