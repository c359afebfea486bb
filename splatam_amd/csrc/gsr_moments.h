// gsr_moments.h -- the second-moment index algebra of the backward_power == 2 route: which moments a pair
// forms in the tile backward (bwd_tile's MOM variants, gsr_render_bwd.h) and how gauss_bwd_mom_kernel
// (gsr_backward_power.hip) reads them back as the symmetric matrix of the pair's base values.
//
// MOM (backward_power == 2, gauss_bwd_mom_kernel): the pair's second moments instead of its values.
// The geometric terms are u = h (dx, dy, dx^2, dx dy, dy^2) (h = G dL/dG), so u_i u_j = h^2 dx^a dy^b
// with a + b in {2, 3, 4}: 12 distinct monomial moments instead of 15 products.  Layout:
//   [0, 12)  sum h^2 dx^a dy^b, monomial t: (2,0) (1,1) (0,2) | (3,0) (2,1) (1,2) (0,3) | (4,0) (3,1) (2,2) (1,3) (0,4)
//   12       sum (G dL/dalpha)^2
//   MOM 1 (colours precomputed, 16 sums): [13, 16) sum (dch dL/dpix_c)^2
//   MOM 2 (SH colours, 34 sums): [13, 19) sum dch^2 dL/dpix_c dL/dpix_d (c <= d, row-major),
//                                [19, 34) sum u_i dch dL/dpix_c (i-major)
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace gsr {

constexpr int mom_nv(int mom) { return mom == 1 ? 16 : 34; }  // sums per instance record
__host__ __device__ constexpr int mono_t(int a, int b) {  // monomial index of dx^a dy^b, a + b in {2, 3, 4}
    return a + b == 2 ? 2 - a : (a + b == 3 ? 3 + (3 - a) : 7 + (4 - a));
}
__host__ __device__ constexpr int u_a(int i) { return i == 0 ? 1 : (i == 2 ? 2 : (i == 3 ? 1 : 0)); }  // u_i ~ dx^a dy^b
__host__ __device__ constexpr int u_b(int i) { return i == 1 ? 1 : (i == 3 ? 1 : (i == 4 ? 2 : 0)); }
__host__ __device__ constexpr int ww_q(int c, int d) {  // MOM 2 index of the colour product (c, d), any order
    return c > d ? 13 + (d == 0 ? c : (d == 1 ? 2 + c : 5)) : 13 + (c == 0 ? d : (c == 1 ? 2 + d : 5));
}
static_assert(mono_t(2, 0) == 0 && mono_t(0, 2) == 2 && mono_t(0, 3) == 6 && mono_t(4, 0) == 7 && mono_t(0, 4) == 11, "");
static_assert(ww_q(0, 0) == 13 && ww_q(2, 1) == 17 && ww_q(2, 2) == 18, "");
// Per-entry quantities the moments are formed from
struct MomIn {
    float m20, m11, m02;  // h^2 dx^2, h^2 dx dy, h^2 dy^2
    float dx, dy, xx, xy, yy;
    float o2, c2;         // (G dL/dalpha)^2, dch^2
    float hc[3];          // h dch dL/dpix_c (MOM 2)
};
// moment Q of one entry (per-pixel constants: dp2[c] = dL/dpix_c^2, dpp[6] = the c <= d products)
template <int MOM, int Q>
__device__ __forceinline__ float mom_val(const MomIn& e, const float (&dp2)[3], const float (&dpp)[6]) {
    if constexpr (Q < 3) return Q == 0 ? e.m20 : (Q == 1 ? e.m11 : e.m02);
    else if constexpr (Q < 5) return e.m20 * (Q == 3 ? e.dx : e.dy);
    else if constexpr (Q < 7) return e.m02 * (Q == 5 ? e.dx : e.dy);
    else if constexpr (Q < 10) return e.m20 * (Q == 7 ? e.xx : (Q == 8 ? e.xy : e.yy));
    else if constexpr (Q < 12) return e.m02 * (Q == 10 ? e.xy : e.yy);
    else if constexpr (Q == 12) return e.o2;
    else if constexpr (MOM == 1) return e.c2 * dp2[Q - 13];
    else if constexpr (Q < 19) return e.c2 * dpp[Q - 13];
    else {
        constexpr int i = (Q - 19) / 3, c = (Q - 19) % 3;
        const float mono = i == 0 ? e.dx : (i == 1 ? e.dy : (i == 2 ? e.xx : (i == 3 ? e.xy : e.yy)));
        return e.hc[c] * mono;
    }
}
// One reduction pass over moments [Q0, Q0 + N) of the step's four entries.
template <int MOM, int Q0, int... Q>
__device__ __forceinline__ void mom_values(const MomIn (&e)[4], const float (&dp2)[3], const float (&dpp)[6], float* v,
                                           std::integer_sequence<int, Q...>) {
    constexpr int N = sizeof...(Q);
#pragma unroll
    for (int k = 0; k < 4; k++) ((v[N * k + Q] = mom_val<MOM, Q0 + Q>(e[k], dp2, dpp)), ...);
}
// (the tile backward's row reduction into the lane's LDS slot: defined in gsr_render_bwd.h, whose bwd_tile is
// mom_pass's only caller)
template <int N>
__device__ __forceinline__ void reduce_store(const float (&v)[4 * N], int lane, float* dst, bool store);
template <int MOM, int Q0, int N>
__device__ __forceinline__ void mom_pass(const MomIn (&e)[4], const float (&dp2)[3], const float (&dpp)[6], int lane,
                                         float* dst) {
    float v[4 * N];
    mom_values<MOM, Q0>(e, dp2, dpp, v, std::make_integer_sequence<int, N>{});
    reduce_store<N>(v, lane, dst + Q0, true);
}
// The moments as the symmetric 9 x 9 matrix of the base values b = (u0..u4, G dL/dalpha, dch dL/dpix_0..2)
// (MOM 1 forms no colour cross moments: those entries stay 0).
template <int MOM, int IJ>
struct MomSlot {  // (frontend-evaluated: every register-array index below is a compile-time constant)
    static constexpr int i = IJ / 9, j = IJ % 9;
    static constexpr int q = (i < 5 && j < 5) ? mono_t(u_a(i) + u_a(j), u_b(i) + u_b(j))
                             : (i == 5 && j == 5) ? 12
                             : (i >= 6 && j >= 6) ? (MOM == 1 ? (i == j ? 13 + (i - 6) : -1) : ww_q(i - 6, j - 6))
                             : (MOM == 2 && i < 5 && j >= 6) ? 19 + 3 * i + (j - 6)
                             : (MOM == 2 && j < 5 && i >= 6) ? 19 + 3 * j + (i - 6)
                                                             : -1;
};
template <int MOM, int... IJ>
__device__ __forceinline__ void mom_matrix(const float* S, float (&Sm)[9][9], std::integer_sequence<int, IJ...>) {
    ((Sm[MomSlot<MOM, IJ>::i][MomSlot<MOM, IJ>::j] = MomSlot<MOM, IJ>::q >= 0 ? S[MomSlot<MOM, IJ>::q >= 0 ? MomSlot<MOM, IJ>::q : 0] : 0.f), ...);
}

}  // namespace gsr
