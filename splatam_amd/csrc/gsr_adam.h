// gsr_adam.h -- torch.optim.Adam's element update as the fused optimizer steps apply it: the coefficient
// record, its one host fill and the two element forms.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace gsr {

// The coefficients every element of a step shares.  Embedded in the kernel argument records (AdamArgs,
// MapAdam, ShAdam) in this order: reordering the fields moves the kernels' argument bytes.
struct AdamCoef {
    float w1;        // 1 - beta1 (lerp weight)
    float beta2;
    float omb2;      // 1 - beta2
    float bc2_sqrt;  // sqrt(1 - beta2^step)
    float eps;
};
// torch forms these scalars from python floats (double) and rounds them to float in the kernels
inline AdamCoef adam_coef(double beta1, double beta2, double eps, int step) {
    return {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(1.0 - pow(beta2, (double)step)),
            (float)eps};
}
// 1 - beta1^step; a tensor's step_size is (float)(-lr / adam_bc1(beta1, step))
inline double adam_bc1(double beta1, int step) { return 1.0 - pow(beta1, (double)step); }

// torch.optim.Adam's element update (foreach form: exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2)
// .addcmul_(g, g, 1-b2); p.addcdiv_(exp_avg, sqrt(exp_avg_sq)/sqrt(bc2) + eps, -lr/bc1)), in the two forms
// the library holds:
//   adam_update_elem  exact: no FP contraction, each operation rounded like torch's separate kernels.  Used by
//                     gsr_map_transform_bwd_adam (MapAdam, gsr_mapping.hip) and the SH colour step inside sh_bwd
//                     (ShAdam, gsr_sh.hip), which share it: the two kernels had contracted differently and
//                     diverged by an ulp from the second step on.
//   adam_elem         contracted: the same text under the compiler's default contraction, which fuses the
//                     multiply-adds.  Used by gsr_adam_step (AdamArgs, gsr_mapping.hip) and by the pose step
//                     (adam_update, gsr_glue_common.h, which rounds PoseAdam's double beta2 on the device).
//                     It differs from torch's separately rounded kernels by those roundings.
// The forms are not unified here: that would move the bits of FusedAdam and of every tracked pose, and the
// pinned 40-iteration frame already sits at 1.7 % of its 2 % bound.  Unifying them is a decision of its own,
// with its own measurements.
__device__ __forceinline__ float adam_update_elem(float p, float g, float& m, float& v, float ss, const AdamCoef& c) {
#pragma clang fp contract(off)
    const float mm = m + c.w1 * (g - m);
    float v2 = v * c.beta2;
    v2 = v2 + c.omb2 * g * g;
    const float denom = sqrtf(v2) / c.bc2_sqrt + c.eps;
    m = mm;
    v = v2;
    return p + ss * (mm / denom);
}
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float ss, const AdamCoef& c) {
    m = m + c.w1 * (g - m);
    v = v * c.beta2;
    v = v + c.omb2 * g * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p + ss * (m / denom);
}

}  // namespace gsr
