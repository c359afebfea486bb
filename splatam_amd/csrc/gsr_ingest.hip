// gsr_ingest.hip -- a raw sensor frame into the frames the sequence reads (include/gsr_glue.h: gsr_ingest_frame):
// what the reference's intake does op by op on arrival (scripts/ros_handler.py:402-411, 434-435;
// datasets/gradslam_datasets/basedataset.py:250-257, 312-316) -- the interleaved uint8 [H,W,3] image to planar
// float32 colour in [0, 1], the uint16 [H,W] depth image to metres with the far readings marked -1 -- and, in
// the same launch, the frame's copies at the tracking and the densification resolution.  One launch on the
// caller's stream:
//
//   ig_ingest_kernel    one grid in two parts, cut at a block boundary.  The first `qblocks` blocks convert the
//                       full-size frame, flat over its N = H W pixels, four pixels per lane: 12 colour bytes in
//                       (three dwords where the image starts on a 4-byte address), one float4 out to each of the
//                       three planes; four depth readings in (one 8-byte load where they start on an 8-byte
//                       address), one float4 out.  The other blocks form the small outputs like
//                       rs_resize_kernel (gsr_resize.hip), one thread per output pixel, the first output's
//                       pixels and then the second's, x fastest -- reading the BYTES and converting every tap
//                       on the fly: the float frame is being written by other blocks of this launch and is
//                       never read.  The conversion is a pure function of the byte (of the reading), so the
//                       small outputs hold the bits gsr_resize_frame forms from the float frame.
//
// A streaming kernel: no LDS, no atomics, no workspace, no counters; plain vector stores.  Neighbouring lanes
// read neighbouring bytes and write neighbouring floats.  The vector forms are chosen per pointer from the
// addresses the call is given (a frame may be a slice of a larger capture buffer: any byte address for the
// colour, any 2-byte address for the depth) and need N % 4 == 0 for the planes' float4 stores; the tail quad
// and every other case go byte by byte.
//
// Every float operation is rounded on its own (no contraction): the colour is ONE float32 division by 255 (not a
// multiply by a reciprocal), the depth ONE float64 division rounded to float32 once.
#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_errors.h"
#include "gsr_resize_taps.h"

#include <math.h>

namespace gsr {
namespace {

constexpr int IG_BLOCK = 256;

struct IgOut {
    int h, w;
    float* im;
    float* depth;
};

// the depth rule's parameters: metres = (float)((double)u / scale); far (>= max_depth, when used) is -1
struct IgDepth {
    double scale;
    float max_depth;
    int use_max;
};

__device__ __forceinline__ float ig_colour(unsigned b) { return (float)b / 255.0f; }

__device__ __forceinline__ float ig_depth(unsigned u, const IgDepth& r) {
    const float d = (float)((double)u / r.scale);
    return (r.use_max && d >= r.max_depth) ? -1.0f : d;
}

typedef float IgFloat4 __attribute__((ext_vector_type(4)));

// four neighbouring floats: one 16-byte store (VEC: p is 16-byte aligned) or four 4-byte ones
template <bool VEC>
__device__ __forceinline__ void ig_store4(float* p, float a, float b, float c, float d) {
    if constexpr (VEC) {
        *reinterpret_cast<IgFloat4*>(__builtin_assume_aligned(p, 16)) = IgFloat4{a, b, c, d};
    } else {
        p[0] = a, p[1] = b, p[2] = c, p[3] = d;
    }
}

// pixels [4 q, 4 q + 4) of the full-size frame (fewer in the tail quad); OUT_VEC: N % 4 == 0 and im, depth 16-byte
// aligned, so every quad of every plane starts on a 16-byte address (and there is no tail)
template <bool OUT_VEC>
__device__ __forceinline__ void ig_full_quad(long long q, long long N, const unsigned char* __restrict__ rgb,
                                             const unsigned short* __restrict__ d16, const IgDepth& rule,
                                             float* __restrict__ im, float* __restrict__ depth, int rgb_vec,
                                             int d16_vec) {
    const long long p0 = 4 * q;
    if (p0 + 4 > N) {  // the tail: one to three pixels, byte by byte
        for (long long p = p0; p < N; p++) {
            for (int c = 0; c < 3; c++) im[c * N + p] = ig_colour(rgb[3 * p + c]);
            depth[p] = ig_depth(d16[p], rule);
        }
        return;
    }
    unsigned b[12];
    if (rgb_vec) {  // 12 q bytes past a 4-byte address
        const unsigned* const w = reinterpret_cast<const unsigned*>(rgb + 3 * p0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned v = w[k];
#pragma unroll
            for (int j = 0; j < 4; j++) b[4 * k + j] = (v >> (8 * j)) & 0xffu;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) b[k] = rgb[3 * p0 + k];
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
        ig_store4<OUT_VEC>(im + c * N + p0, ig_colour(b[c]), ig_colour(b[3 + c]), ig_colour(b[6 + c]),
                           ig_colour(b[9 + c]));
    unsigned u[4];
    if (d16_vec) {  // 8 q bytes past an 8-byte address
        const uint2 v = *reinterpret_cast<const uint2*>(d16 + p0);
        u[0] = v.x & 0xffffu, u[1] = v.x >> 16, u[2] = v.y & 0xffffu, u[3] = v.y >> 16;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) u[k] = d16[p0 + k];
    }
    ig_store4<OUT_VEC>(depth + p0, ig_depth(u[0], rule), ig_depth(u[1], rule), ig_depth(u[2], rule),
                       ig_depth(u[3], rule));
}

// output pixel p of a small output: rs_resize_kernel's pixel with every tap converted from the bytes
__device__ __forceinline__ void ig_small_pixel(long long p, int H, int W, const unsigned char* __restrict__ rgb,
                                               const unsigned short* __restrict__ d16, const IgDepth& rule,
                                               const IgOut& o) {
    const int y = (int)(p / o.w), x = (int)(p - (long long)y * o.w);
    const size_t n = (size_t)o.h * o.w;
    // depth: nearest, floor(dst * in / out)
    const int ny = (int)(((long long)y * H) / o.h), nx = (int)(((long long)x * W) / o.w);
    o.depth[p] = ig_depth(d16[(size_t)ny * W + nx], rule);
    // colour: horizontally on the two rows, then vertically
    const RsTap tx = rs_tap(x, W, o.w), ty = rs_tap(y, H, o.h);
    const size_t r0 = (size_t)ty.i0 * W, r1 = (size_t)ty.i1 * W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned char* const src = rgb + c;
        const float top = rs_lerp(ig_colour(src[3 * (r0 + tx.i0)]),
                                  tx.t == 0.f ? 0.f : ig_colour(src[3 * (r0 + tx.i1)]), tx.t);
        float v = top;
        if (ty.t != 0.f) {
            const float bot = rs_lerp(ig_colour(src[3 * (r1 + tx.i0)]),
                                      tx.t == 0.f ? 0.f : ig_colour(src[3 * (r1 + tx.i1)]), tx.t);
            v = rs_lerp(top, bot, ty.t);
        }
        o.im[(size_t)c * n + p] = v;
    }
}

__global__ void __launch_bounds__(IG_BLOCK)
ig_ingest_kernel(int H, int W, const unsigned char* __restrict__ rgb, const unsigned short* __restrict__ d16,
                 IgDepth rule, float* __restrict__ im, float* __restrict__ depth, int rgb_vec, int d16_vec,
                 int out_vec, long long nquads, unsigned qblocks, IgOut o0, IgOut o1, long long n0,
                 long long nsmall) {
    if (blockIdx.x < qblocks) {  // (uniform per block)
        const long long q = (long long)blockIdx.x * IG_BLOCK + threadIdx.x;
        if (q >= nquads) return;
        const long long N = (long long)H * W;
        if (out_vec)
            ig_full_quad<true>(q, N, rgb, d16, rule, im, depth, rgb_vec, d16_vec);
        else
            ig_full_quad<false>(q, N, rgb, d16, rule, im, depth, rgb_vec, d16_vec);
        return;
    }
    long long p = (long long)(blockIdx.x - qblocks) * IG_BLOCK + threadIdx.x;
    if (p >= nsmall) return;
    const bool second = p >= n0;
    if (second) p -= n0;
    ig_small_pixel(p, H, W, rgb, d16, rule, second ? o1 : o0);
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_ingest_frame(int H, int W, const unsigned char* rgb_hwc, const unsigned short* depth_u16,
                     double png_depth_scale, int use_max_depth, float max_depth, float* im, float* depth, int h0,
                     int w0, float* im_out0, float* depth_out0, int h1, int w1, float* im_out1, float* depth_out1,
                     void* stream) {
    auto refuse = [&](const char* what) { return fail(GSR_ERR_INVALID_ARG, std::string("ingest_frame: ") + what); };
    if (!image_size_ok(H, W)) return refuse("bad image size");
    if (!rgb_hwc || !depth_u16) return refuse("null input");
    if (!isfinite(png_depth_scale) || !(png_depth_scale > 0.0)) return refuse("png_depth_scale must be finite and > 0");
    if (use_max_depth && max_depth != max_depth) return refuse("max_depth is NaN");
    if (!im != !depth) return refuse("the full frame needs both its colour and its depth pointer");
    IgOut outs[2] = {{h0, w0, im_out0, depth_out0}, {h1, w1, im_out1, depth_out1}};
    long long count[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        IgOut& o = outs[k];
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
    const long long N = (long long)H * W, nsmall = count[0] + count[1];
    const long long nquads = im ? (N + 3) / 4 : 0;
    if (nquads + nsmall == 0) return refuse("no output");
    const long long qblocks = (nquads + IG_BLOCK - 1) / IG_BLOCK;
    const long long blocks = qblocks + (nsmall + IG_BLOCK - 1) / IG_BLOCK;
    if (blocks > 0x7fffffffLL) return refuse("sizes too large");
    // the vector forms, per pointer: quad q starts 12 q colour bytes, 8 q depth bytes and 16 q output bytes in
    // (plane c another 4 c N bytes)
    const int rgb_vec = (uintptr_t)rgb_hwc % 4 == 0, d16_vec = (uintptr_t)depth_u16 % 8 == 0;
    const int out_vec = im && N % 4 == 0 && aligned16(im) && aligned16(depth);
    const IgDepth rule = {png_depth_scale, max_depth, use_max_depth != 0};
    hipLaunchKernelGGL(ig_ingest_kernel, dim3((unsigned)blocks), dim3(IG_BLOCK), 0, (hipStream_t)stream, H, W, rgb_hwc,
                       depth_u16, rule, im, depth, rgb_vec, d16_vec, out_vec, nquads, (unsigned)qblocks, outs[0],
                       outs[1], count[0], nsmall);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : hip_fail(e, "ingest_frame");
}

}  // extern "C"
