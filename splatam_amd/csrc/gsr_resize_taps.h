// gsr_resize_taps.h -- the sample rules of a frame's small copies (include/gsr_glue.h: gsr_resize_frame), shared
// by the kernel that resizes a float frame (gsr_resize.hip) and the one that forms the small frames straight
// from the sensor's bytes (gsr_ingest.hip): the bilinear axis' taps and the lerp.
//
// The source columns / rows and the weights come from integers (quotient and remainder of
// ((2 x + 1) W - w) / (2 w)), never from a float scale, and every float operation is rounded on its own (no
// contraction) in the order include/gsr_glue.h states.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

// The left tap and the weight of the right one along an axis of n_in source and n_out output samples:
// s = max(0, (i + 0.5) n_in / n_out - 0.5) = max(0, ((2 i + 1) n_in - n_out) / (2 n_out)).
struct RsTap {
    int i0, i1;
    float t;
};
__device__ __forceinline__ RsTap rs_tap(int i, int n_in, int n_out) {
    const int den = 2 * n_out;
    const int num = (2 * i + 1) * n_in - n_out;  // (< 2 n_in n_out: the entry refuses sizes beyond an int)
    RsTap r;
    if (num <= 0) {
        r.i0 = 0;
        r.t = 0.f;
    } else {
        r.i0 = num / den;
        r.t = (float)(num - r.i0 * den) / (float)den;
    }
    r.i1 = min(r.i0 + 1, n_in - 1);
    return r;
}

// a + t (b - a); a tap of weight zero is not read into the result (a NaN or an infinity there stays out)
__device__ __forceinline__ float rs_lerp(float a, float b, float t) {
#pragma clang fp contract(off)
    return t == 0.f ? a : a + t * (b - a);
}

}  // namespace gsr
