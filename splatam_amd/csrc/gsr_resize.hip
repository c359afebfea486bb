// gsr_resize.hip -- a frame's copies at other resolutions (include/gsr_glue.h: gsr_resize_frame): the
// tracking frame of SplaTAM-S (tracking_image_height / width, scripts/splatam.py:517-523) and the
// densification frame (densification_image_height / width), which the reference's dataset loader
// makes on the host (datasets/gradslam_datasets/basedataset.py:224-257: colour bilinear, depth
// nearest).  One launch on the caller's stream for up to two outputs:
//
//   rs_resize_kernel    one thread per output pixel, the first output's pixels and then the second's,
//                       x fastest: the three colour channels (bilinear, half-pixel centres, edge
//                       clamp) and the depth (nearest) of that pixel.
//
// A streaming kernel: no LDS, no atomics, no workspace, no counters.  Neighbouring threads read
// neighbouring (or the same) source columns of at most two source rows per plane and write
// neighbouring outputs, so every access is coalesced on the planar [C,H,W] layout.
//
// The source columns / rows and the weights come from integers (quotient and remainder of
// ((2 x + 1) W - w) / (2 w)), never from a float scale, and every float operation is rounded on its
// own (no contraction) in the order include/gsr_glue.h states, so resize.resize_literal's
// elementwise torch ops form the same bits.  The taps and the lerp are gsr_resize_taps.h's, which
// gsr_ingest.hip shares.
#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_errors.h"
#include "gsr_resize_taps.h"

namespace gsr {
namespace {

constexpr int RS_BLOCK = 256;

struct RsOut {
    int h, w;
    float* im;
    float* depth;
};

__global__ void __launch_bounds__(RS_BLOCK)
rs_resize_kernel(int H, int W, const float* __restrict__ im, const float* __restrict__ depth, RsOut o0, RsOut o1,
                 long long n0, long long total) {
    long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= total) return;
    const bool second = p >= n0;
    if (second) p -= n0;
    const RsOut o = second ? o1 : o0;
    const int y = (int)(p / o.w), x = (int)(p - (long long)y * o.w);
    const size_t N = (size_t)H * W, n = (size_t)o.h * o.w;
    // depth: nearest, floor(dst * in / out); the bits are copied
    const int ny = (int)(((long long)y * H) / o.h), nx = (int)(((long long)x * W) / o.w);
    o.depth[p] = depth[(size_t)ny * W + nx];
    // colour: horizontally on the two rows, then vertically
    const RsTap tx = rs_tap(x, W, o.w), ty = rs_tap(y, H, o.h);
    const size_t r0 = (size_t)ty.i0 * W, r1 = (size_t)ty.i1 * W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float* const src = im + (size_t)c * N;
        const float top = rs_lerp(src[r0 + tx.i0], tx.t == 0.f ? 0.f : src[r0 + tx.i1], tx.t);
        float v = top;
        if (ty.t != 0.f) {
            const float bot = rs_lerp(src[r1 + tx.i0], tx.t == 0.f ? 0.f : src[r1 + tx.i1], tx.t);
            v = rs_lerp(top, bot, ty.t);
        }
        o.im[(size_t)c * n + p] = v;
    }
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_resize_frame(int H, int W, const float* im, const float* depth, int h0, int w0, float* im_out0,
                     float* depth_out0, int h1, int w1, float* im_out1, float* depth_out1, void* stream) {
    auto refuse = [&](const char* what) { return fail(GSR_ERR_INVALID_ARG, std::string("resize_frame: ") + what); };
    if (!image_size_ok(H, W)) return refuse("bad image size");
    if (!im || !depth) return refuse("null input");
    RsOut outs[2] = {{h0, w0, im_out0, depth_out0}, {h1, w1, im_out1, depth_out1}};
    long long count[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        RsOut& o = outs[k];
        if (!o.im && !o.depth) {  // an absent output: its sizes are not read
            o.h = o.w = 1;
            continue;
        }
        if (!o.im || !o.depth) return refuse("an output needs both its colour and its depth pointer");
        if (!image_size_ok(o.h, o.w)) return refuse("bad output size");
        // the taps' numerators (2 i + 1) n_in - n_out stay below 2 n_in n_out: kept inside an int
        if (2LL * o.w * W > 0x7fffffffLL || 2LL * o.h * H > 0x7fffffffLL) return refuse("sizes too large");
        count[k] = (long long)o.h * o.w;
    }
    const long long total = count[0] + count[1];
    if (total == 0) return refuse("no output");
    const long long blocks = (total + RS_BLOCK - 1) / RS_BLOCK;
    if (blocks > 0x7fffffffLL) return refuse("sizes too large");
    hipLaunchKernelGGL(rs_resize_kernel, dim3((unsigned)blocks), dim3(RS_BLOCK), 0, (hipStream_t)stream, H, W, im,
                       depth, outs[0], outs[1], count[0], total);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, "resize_frame");
}

}  // extern "C"
