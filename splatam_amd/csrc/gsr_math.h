// gsr_math.h -- per-Gaussian device maths: projection, covariance and conic, SH evaluation, the render
// record's conic scales and the block / tile masks of a Gaussian's alpha ellipse.
#pragma once
#include "gsr_layout.h"

namespace gsr {

// ------------------------------------------------------------ device math --
// The functions below restate forward.cu / backward.cu / auxiliary.h in
// standard notation.  They keep the operation order of oracle/gsr_oracle.c and
// disable FMA contraction so that preprocess outputs (radii, tile rects) are
// bit-identical to the float32 oracle.

__constant__ static const float kSH_C0 = 0.28209479177387814f;
__constant__ static const float kSH_C1 = 0.4886025119029199f;
__constant__ static const float kSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                             -1.0925484305920792f, 0.5462742152960396f};
__constant__ static const float kSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                             0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                             -0.5900435899266435f};

__device__ __forceinline__ float3 xform4x3(float3 p, const float* m) {  // auxiliary.h:58-66
#pragma clang fp contract(off)
    return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
                       m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}

__device__ __forceinline__ float4 xform4x4(float3 p, const float* m) {  // auxiliary.h:68-77
#pragma clang fp contract(off)
    return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14], m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

__device__ __forceinline__ float ndc2pix(float v, int S) {  // auxiliary.h:41-44 (double literals)
    return (float)((((double)v + 1.0) * S - 1.0) * 0.5);
}

__device__ __forceinline__ void get_rect(float px, float py, int r, int gx, int gy, int& x0, int& y0, int& x1,
                                         int& y1) {  // auxiliary.h:46-56
#pragma clang fp contract(off)
    float fr = (float)r;
    int a = (int)((px - fr) / (float)TILE_X);
    int b = (int)((py - fr) / (float)TILE_Y);
    float cx = px + fr; cx = cx + (float)TILE_X; cx = cx - 1.0f;
    float cy = py + fr; cy = cy + (float)TILE_Y; cy = cy - 1.0f;
    int c = (int)(cx / (float)TILE_X);
    int d = (int)(cy / (float)TILE_Y);
    a = max(a, 0); b = max(b, 0); c = max(c, 0); d = max(d, 0);
    x0 = min(a, gx); y0 = min(b, gy); x1 = min(c, gx); y1 = min(d, gy);
}

// Sigma = R S^2 R^T, R from the un-normalised quaternion (forward.cu:118-152)
__device__ __forceinline__ void rot_from_quat(float4 q, float R[3][3]) {
#pragma clang fp contract(off)
    float r = q.x, x = q.y, y = q.z, z = q.w;
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z); R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z); R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y); R[2][1] = 2.f * (y * z + r * x); R[2][2] = 1.f - 2.f * (x * x + y * y);
}

__device__ __forceinline__ void cov3d_fwd(float3 s3, float mod, float4 q, float cov[6]) {
#pragma clang fp contract(off)
    float R[3][3];
    rot_from_quat(q, R);
    float s[3] = {mod * s3.x, mod * s3.y, mod * s3.z};
    float M[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) M[k][i] = s[k] * R[i][k];
    float S[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) S[i][j] = M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j];
    cov[0] = S[0][0]; cov[1] = S[0][1]; cov[2] = S[0][2];
    cov[3] = S[1][1]; cov[4] = S[1][2]; cov[5] = S[2][2];
}

struct Proj {
    float tx, ty, tz, xmul, ymul;
    float Mx[2][3];  // J V3
    float a, b, c;   // cov2D (+0.3 low-pass on the diagonal)
};

// forward.cu:74-113 (EWA, with the +-1.3 tanfov clamp) in standard notation
__device__ __forceinline__ void cov2d_fwd(float3 mean, float fx, float fy, float tanx, float tany, const float c3[6],
                                          const float* view, Proj& o) {
#pragma clang fp contract(off)
    float3 t = xform4x3(mean, view);
    float limx = 1.3f * tanx, limy = 1.3f * tany;
    float txtz = t.x / t.z, tytz = t.y / t.z;
    o.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    o.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    o.tx = t.x; o.ty = t.y; o.tz = t.z;
    float J00 = fx / t.z, J02 = -(fx * t.x) / (t.z * t.z);
    float J11 = fy / t.z, J12 = -(fy * t.y) / (t.z * t.z);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.Mx[0][k] = J00 * view[4 * k + 0] + J02 * view[4 * k + 2];
        o.Mx[1][k] = J11 * view[4 * k + 1] + J12 * view[4 * k + 2];
    }
    float S[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float u0[3], u1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        u0[k] = S[k][0] * o.Mx[0][0] + S[k][1] * o.Mx[0][1] + S[k][2] * o.Mx[0][2];
        u1[k] = S[k][0] * o.Mx[1][0] + S[k][1] * o.Mx[1][1] + S[k][2] * o.Mx[1][2];
    }
    float a = o.Mx[0][0] * u0[0] + o.Mx[0][1] * u0[1] + o.Mx[0][2] * u0[2];
    float b = o.Mx[0][0] * u1[0] + o.Mx[0][1] * u1[1] + o.Mx[0][2] * u1[2];
    float c = o.Mx[1][0] * u1[0] + o.Mx[1][1] * u1[1] + o.Mx[1][2] * u1[2];
    o.a = a + 0.3f;
    o.b = b;
    o.c = c + 0.3f;
}

// conic = inverse of the (dilated) 2D covariance (forward.cu:219-224), shared by
// preprocess and the backward (which recomputes it rather than storing it):
// one contraction-free sequence, so both get the same bits.  Returns det.
__device__ __forceinline__ float conic_of(const Proj& pj, float& ca, float& cb, float& cc) {
#pragma clang fp contract(off)
    const float det = pj.a * pj.c - pj.b * pj.b;
    const float det_inv = 1.f / det;
    ca = pj.c * det_inv;
    cb = -pj.b * det_inv;
    cc = pj.a * det_inv;
    return det;
}

// forward.cu:20-71 (one channel at a time, same order as the oracle)
__device__ __forceinline__ void sh_fwd(int deg, float3 pos, const float* campos, const float* sh, float rgb[3],
                                       unsigned& clamped_bits) {
#pragma clang fp contract(off)
    float dx = pos.x - campos[0], dy = pos.y - campos[1], dz = pos.z - campos[2];
    float len = sqrtf(dx * dx + dy * dy + dz * dz);
    float x = dx / len, y = dy / len, z = dz / len;
    clamped_bits = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
#define S(k) sh[3 * (k) + ch]
        float res = kSH_C0 * S(0);
        if (deg > 0) {
            res = res - kSH_C1 * y * S(1) + kSH_C1 * z * S(2) - kSH_C1 * x * S(3);
            if (deg > 1) {
                float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                res = res + (kSH_C2[0] * xy * S(4) + kSH_C2[1] * yz * S(5) + kSH_C2[2] * (2.f * zz - xx - yy) * S(6) +
                             kSH_C2[3] * xz * S(7) + kSH_C2[4] * (xx - yy) * S(8));
                if (deg > 2) {
                    res = res + (kSH_C3[0] * y * (3.f * xx - yy) * S(9) + kSH_C3[1] * xy * z * S(10) +
                                 kSH_C3[2] * y * (4.f * zz - xx - yy) * S(11) +
                                 kSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * S(12) +
                                 kSH_C3[4] * x * (4.f * zz - xx - yy) * S(13) + kSH_C3[5] * z * (xx - yy) * S(14) +
                                 kSH_C3[6] * x * (xx - 3.f * yy) * S(15));
                }
            }
        }
#undef S
        res = res + 0.5f;
        if (res < 0.f) clamped_bits |= 1u << ch;
        rgb[ch] = fmaxf(res, 0.f);
    }
}

// Render-record form of the conic (written by preprocess, staged to LDS as is):
// prescaled so that
//   p2 = A' dx^2 + B' dx dy + C' dy^2 = log2(e) * power      (forward.cu:341)
// feeds v_exp_f32 (exp2) directly, laid out as
//   sa = q0 = (x, y, A', C'),  sb = q1 = (B', opacity, depth, -)
// so (x, y) - pixel and (A', C') * (dx, dy) are packed-f32 pairs.  Forward and
// backward read the same values and evaluate p2 through the same contraction-
// free sequence, so both see bit-identical alphas (the backward recovers T by
// dividing by 1 - alpha and must take exactly the forward's decisions).
constexpr float kLog2e = 1.4426950408889634f;
typedef float v2f __attribute__((ext_vector_type(2)));
constexpr float K_AC = -0.5f * kLog2e;  // render-record scale of conic A and C
constexpr float K_B = -kLog2e;          // render-record scale of conic B
__device__ __forceinline__ v2f pix_delta(float4 sa, v2f pix) {
#pragma clang fp contract(off)
    return v2f{sa.x, sa.y} - pix;
}
// p2 = (A' dx) dx + (C' dy) dy, then + (B' dx) dy: forward.cu:341's order (the two square terms, of one
// sign, summed first; the cross term last), as FMAs on the packed (A' dx, C' dy).  The forward and the
// backward evaluate the same expression, so their alpha decisions agree bit for bit.  (Round 4 evaluated
// dx (A' dx + B' dy) + C' dy^2, one VALU less; its per-element gradient errors moved away from the
// float32 reference arithmetic's: config 4's worst dscales element 0.127 of its float32 error scale against
// 0.05 -- tools/alpha_forms.py replays both orders in the CPU oracle, profiles/r7_alpha_forms_cpu.txt.)
__device__ __forceinline__ float eval_p2(float4 sa, float4 sb, v2f d) {
#pragma clang fp contract(off)
    const v2f t = v2f{sa.z, sa.w} * d;  // (A' dx, C' dy)
    return __builtin_fmaf(sb.x * d.x, d.y, __builtin_fmaf(t.x, d.x, t.y * d.y));
}

// Pixel of thread tid within its 16x16 tile: wave w covers the 8x8 quadrant
// (w & 1, w >> 1); inside it, 16-lane row r covers the 4x4 block (r & 1, r >> 1),
// lanes row-major.  Tile block b = 4w + r is at block column 2(w & 1) + (r & 1),
// block row 2(w >> 1) + (r >> 1).  Small square footprints cull round Gaussians
// tightly (pixel-pair evaluations per instance on the config-3 frame, AABB cull:
// 16x4 strips 105, 8x8 quadrants 90, 4x4 blocks 48; tools/tile_balance.py).
__device__ __forceinline__ int tile_px(int tid) { return 8 * ((tid >> 6) & 1) + 4 * ((tid >> 4) & 1) + (tid & 3); }
__device__ __forceinline__ int tile_py(int tid) { return 8 * (tid >> 7) + 4 * ((tid >> 5) & 1) + ((tid >> 2) & 3); }

// Ellipse half-extents of the region where o * exp(-0.5 d^T Q d) >= 1/255
// (forward.cu:341-351), with margins that exceed the float32 error of
// evaluating `power` (grows with the conic's eccentricity kappa), so culling
// never changes a result.  Returns false for anything unusual (non-finite
// values, non-positive-definite conic, extreme eccentricity): no culling.
// Sets never = true when alpha <= o < 1/255 (never blended).
__device__ __forceinline__ bool alpha_extent(float4 a, float4 b, float& hx, float& hy, bool& never) {
    // conic from the render-record scaling (a few ulp off the preprocess values; the
    // margins below are orders of magnitude larger)
    const float A = a.z * (1.f / K_AC), B = b.x * (1.f / K_B), C = a.w * (1.f / K_AC), o = b.y;
    const float det = A * C - B * B;
    never = false;
    if (!(det > 0.f) || !(A > 0.f) || !isfinite(det) || !isfinite(a.x) || !isfinite(a.y) || !isfinite(o))
        return false;
    const float kappa = A * C / det;  // 1 / (1 - rho^2) >= 1
    if (!(kappa < 1e4f)) return false;
    const float t = 255.f * o;
    if (t < 0.999f) {
        never = true;
        return true;
    }
    const float tau = fmaxf(__logf(t), 0.f) * (1.001f + 4e-6f * kappa) + 1e-3f;
    hx = sqrtf(2.f * tau * C / det) * 1.001f + 0.01f;
    hy = sqrtf(2.f * tau * A / det) * 1.001f + 0.01f;
    return true;
}

// 16-bit mask of the 4x4-pixel blocks of a tile (bit 4w + r, layout of
// tile_px / tile_py) that a Gaussian can contribute to.
__device__ __forceinline__ uint32_t block_mask(float4 a, float4 b, float x0, float y0) {
    float hx = 0.f, hy = 0.f;
    bool never;
    if (!alpha_extent(a, b, hx, hy, never)) return 0xFFFFu;
    if (never) return 0u;
    const float xl = a.x - hx, xh = a.x + hx, yl = a.y - hy, yh = a.y + hy;
    uint32_t mx = 0, my = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        mx |= (xh >= x0 + 4.f * c && xl <= x0 + 4.f * c + 3.f) ? 1u << c : 0u;
        my |= (yh >= y0 + 4.f * c && yl <= y0 + 4.f * c + 3.f) ? 1u << c : 0u;
    }
    uint32_t m = 0;
#pragma unroll
    for (int bi = 0; bi < 16; bi++) {
        const int w = bi >> 2, r = bi & 3;
        const int cx = 2 * (w & 1) + (r & 1), cy = 2 * (w >> 1) + (r >> 1);
        m |= ((mx >> cx) & (my >> cy) & 1u) << bi;
    }
    return m;
}

// Sorted tile list entries: (4x4-block mask << 32) | Gaussian id.  The sort writes
// plain ids; render_fwd computes the ellipse-exact block_mask_exact of every entry
// it stages (one per thread, from the render record it loads anyway) and writes
// it into the entry's high half, where render_bwd (which only stages entries
// render_fwd staged) reads it.
typedef uint64_t PointEntry;
__device__ __forceinline__ uint32_t pe_id(PointEntry p) { return (uint32_t)p; }
__device__ __forceinline__ uint32_t pe_mask(PointEntry p) { return (uint32_t)(p >> 32); }

// block_mask with the ellipse instead of its bounding box: per block row the
// x-extent of the alpha >= 1/255 ellipse q(u) = A ux^2 + 2B ux uy + C uy^2 <= 2 tau
// over the row's y-span is exact (the left boundary (-B uy - sqrt(2 tau A - det
// uy^2)) / A is convex in uy, so its minimum over an interval is the leftmost
// point uy = B sqrt(2 tau / (det C)) clamped to the interval; symmetrically on
// the right); margins cover the float32 error.  ~10 % fewer pixel-pair
// evaluations than the box on a frame (tools/tile_balance.py).
// The per-Gaussian half of block_mask_exact.  hx < 0: no culling (full mask);
// hy < 0: never blended (empty mask).  The reciprocals, logarithm and square roots are the
// hardware's (v_rcp / v_log / v_sqrt_f32, ~1 ulp; the correctly rounded library forms cost ~10
// instructions each): the margins (x 1.001, + 1e-3 on tau, + 0.01 / 0.02 px) exceed their error by
// four orders of magnitude.
struct MaskGeom {
    float ax, ay, hx, hy, B, inv_A, twoA_tau, det, us, eps;
};
constexpr int MASK_GEOM_F = 10;
__device__ __forceinline__ MaskGeom mask_geom(float4 a, float4 b) {
    MaskGeom g;
    g.ax = a.x;
    g.ay = a.y;
    const float A = a.z * (1.f / K_AC), B = b.x * (1.f / K_B), C = a.w * (1.f / K_AC), o = b.y;
    const float det = A * C - B * B;
    const float rdet = __builtin_amdgcn_rcpf(det);
    const float kappa = A * C * rdet;  // 1 / (1 - rho^2) >= 1
    // anything unusual (non-finite values, a conic that is not positive definite, extreme eccentricity): no culling
    const bool bad = !(det > 0.f) || !(A > 0.f) || !isfinite(det) || !isfinite(a.x) || !isfinite(a.y) ||
                     !isfinite(o) || !(kappa < 1e4f);
    const float t = 255.f * o;
    const bool never = t < 0.999f;  // alpha <= o < 1/255: never blended
    // tau = ln(255 o), with the margin of the float32 error of `power` (grows with kappa)
    const float tau = fmaxf(__builtin_amdgcn_logf(t) * 0.69314718f, 0.f) * (1.001f + 4e-6f * kappa) + 1e-3f;
    const float k2 = 2.f * tau * rdet;
    const float hx = __builtin_amdgcn_sqrtf(k2 * C) * 1.001f + 0.01f;
    const float hy = __builtin_amdgcn_sqrtf(k2 * A) * 1.001f + 0.01f;
    g.hx = bad ? -1.f : (never ? 0.f : hx);
    g.hy = bad ? 0.f : (never ? -1.f : hy);
    g.B = B;
    g.det = det;
    g.twoA_tau = 2.f * tau * A;
    g.inv_A = __builtin_amdgcn_rcpf(A);
    g.us = B * __builtin_amdgcn_sqrtf(k2 * __builtin_amdgcn_rcpf(C));  // uy of the leftmost point (rightmost: -us)
    g.eps = 0.02f + 0.002f * hx;
    return g;
}
// Block row r (pixel centres y0 + 4r .. + 3): the ellipse's x-extent over the row's y-span
// [lo, hi] is [xmin, xmax]; the row's blocks are the columns c with x0 + 4c <= xmax and
// xmin <= x0 + 4c + 3, i.e. c in [ceil((xmin - x0 - 3) / 4), floor((xmax - x0) / 4)] (a rounding of
// the scaled differences can only widen that range: the mask stays conservative).
__device__ __forceinline__ uint32_t mask_of_geom(const MaskGeom& g, float x0, float y0) {
    if (g.hx < 0.f) return 0xFFFFu;
    if (g.hy < 0.f) return 0u;
    const float dy0 = y0 - g.ay;
    const float xa = g.ax - g.eps, xb = g.ax + g.eps;
    const float qx = -0.25f * (x0 + 3.f), px = -0.25f * x0;
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float ylo = dy0 + 4.f * r, yhi = ylo + 3.f;
        const bool row = yhi >= -g.hy && ylo <= g.hy;  // the row meets the ellipse's y-span
        const float lo = fmaxf(ylo, -g.hy), hi = fminf(yhi, g.hy);
        const float ul = __builtin_amdgcn_fmed3f(g.us, lo, hi), ur = __builtin_amdgcn_fmed3f(-g.us, lo, hi);
        const float wl = __builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-g.det * ul, ul, g.twoA_tau), 0.f));
        const float wr = __builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-g.det * ur, ur, g.twoA_tau), 0.f));
        const float xmin = xa - __builtin_fmaf(g.B, ul, wl) * g.inv_A;
        const float xmax = xb + __builtin_fmaf(-g.B, ur, wr) * g.inv_A;
        // column range, clamped to [0, 4) / [-1, 3] in float before the conversion
        const int clo = (int)__builtin_amdgcn_fmed3f(ceilf(__builtin_fmaf(xmin, 0.25f, qx)), 0.f, 4.f);
        const int chi = (int)__builtin_amdgcn_fmed3f(floorf(__builtin_fmaf(xmax, 0.25f, px)), -1.f, 3.f);
        const uint32_t cm = row ? ((1u << (chi + 1)) - 1u) & ~((1u << clo) - 1u) : 0u;  // (chi + 1, clo in [0, 4])
        // block (column c, row r) -> bit 4w + rr, w = 2 (r >> 1) + (c >> 1), rr = 2 (r & 1) + (c & 1)
        const int base = 8 * (r >> 1) + 2 * (r & 1);
        m |= ((cm & 3u) << base) | ((cm >> 2) << (base + 4));
    }
    return m;
}
// Whether the ellipse can reach the tile at all (Camera::cull): mask_of_geom's test with the tile's whole
// pixel-centre span [y0, y0 + 15] as one row and [x0, x0 + 15] as one column -- a superset of the union of its
// sixteen block tests (it also admits the unit gaps between block rows / columns), so conservative like them;
// one test per rect tile instead of the sixteen of mask_of_geom(...) != 0
__device__ __forceinline__ bool tile_reached(const MaskGeom& g, float x0, float y0) {
    if (g.hx < 0.f) return true;
    if (g.hy < 0.f) return false;
    const float ylo = y0 - g.ay, yhi = ylo + 15.f;
    if (!(yhi >= -g.hy && ylo <= g.hy)) return false;
    const float lo = fmaxf(ylo, -g.hy), hi = fminf(yhi, g.hy);
    const float ul = __builtin_amdgcn_fmed3f(g.us, lo, hi), ur = __builtin_amdgcn_fmed3f(-g.us, lo, hi);
    const float wl = __builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-g.det * ul, ul, g.twoA_tau), 0.f));
    const float wr = __builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-g.det * ur, ur, g.twoA_tau), 0.f));
    const float xmin = (g.ax - g.eps) - __builtin_fmaf(g.B, ul, wl) * g.inv_A;
    const float xmax = (g.ax + g.eps) + __builtin_fmaf(-g.B, ur, wr) * g.inv_A;
    return xmax >= x0 && xmin <= x0 + 15.f;
}
__device__ __forceinline__ uint32_t block_mask_exact(float4 a, float4 b, float x0, float y0) {
    return mask_of_geom(mask_geom(a, b), x0, y0);
}
// 4-bit mask of the 8x8-pixel wave quadrants of a tile (bit w: pixel centres
// x0+8(w&1) .. +7, y0+8(w>>1) .. +7) that a Gaussian can contribute to.
__device__ __forceinline__ uint32_t quad_mask(float4 a, float4 b, float x0, float y0) {
    float hx = 0.f, hy = 0.f;
    bool never;
    if (!alpha_extent(a, b, hx, hy, never)) return 0xFu;
    if (never) return 0u;
    const float xl = a.x - hx, xh = a.x + hx, yl = a.y - hy, yh = a.y + hy;
    const uint32_t mx = (xh >= x0 && xl <= x0 + 7.f ? 1u : 0u) | (xh >= x0 + 8.f && xl <= x0 + 15.f ? 2u : 0u);
    const uint32_t my = (yh >= y0 && yl <= y0 + 7.f ? 1u : 0u) | (yh >= y0 + 8.f && yl <= y0 + 15.f ? 2u : 0u);
    // bit w = x half (w & 1) and y half (w >> 1)
    return (mx * (my & 1u)) | ((mx * (my >> 1)) << 2);
}

}  // namespace gsr
