// gsr_render_bwd.h -- the tile backward of the power-1 render as a device function (bwd_tile), the counterpart
// of gsr_render_fwd.h's fwd_tile: its variants (BwdVariant and the named forms), its shape and LDS layout
// (BwdShape), the per-pair sums and their row reduction, and render_bwd_kernel itself.  Shared by
// gsr_backward.hip (render_bwd_kernel's power-1 forms, render_bwd_m2d_kernel, render_track_kernel) and
// gsr_backward_power.hip (render_bwd_kernel's two second-moment forms).
#pragma once
#include "gsr_clock.h"
#include "gsr_diag.h"
#include "gsr_launch.h"
#include "gsr_layout.h"
#include "gsr_math.h"
#include "gsr_moments.h"
#include "gsr_wave.h"

namespace gsr {

// One variant of the tile backward, named by its members instead of by a positional list.
// DUAL: the pass also carries a second colour set (colors2, dL_dpix2) composited
// with the same alpha / T (one dual forward): the per-pair dL/dalpha is the sum
// of both renders'.  OPAC / COL1 / COL2: whether dL/dopacity, dL/dcolors and
// dL/dcolors2 are wanted; absent ones are neither formed nor reduced (tracking
// needs only the geometric sums and the depth colours).  Records use the packed
// layout of rec_sums() (gsr_launch.h): [hx, hy, hxx, hxy, hyy | G dL/dalpha | dch dp(3) | dch dq(Q2)].
// Q2: how many leading channels of dL_dpix2 may be non-zero (3, or 1 when the caller
// promises the rest are zero -- SplaTAM's tracking loss differentiates only the depth
// channel of the [depth, silhouette, depth^2] image).
// MOM (backward_power == 2): the pair's second moments instead of its values (gsr_moments.h).
// C1 = 1: the single-image colour sums of a tile whose dL/dpix channels 1 and 2 are zero (SplaTAM's
// depth/silhouette render: its loss differentiates the depth channel only) -- one colour sum instead of
// three; the batch shape and the record layout stay those of the C1 = 3 variant (the two missing sums are
// stored as zeros), so both serve the same launch.
// M2D1 (the mapping form only: DUAL, OPAC, COL1, COL2, Q2 = 1): the first colour set's own share of (hx, hy) as
// two more sums per pair, from a second accumulator A1 that follows the single-image variant's recurrence
// operation for operation (A1_0 = bg . dL/dpix, e1 = c . dL/dpix - A1, x1 = e1 Tn, A1 <- fma(alpha, e1, A1)); the
// pair adds (araw x1) dx and (araw x1) dy, masked like dLa.  Gaussian-splatting densification reads the RGB
// render's own means2D gradient (scripts/splatam.py:256), which the shared accumulator A does not separate.
template <bool DUAL_, bool OPAC_, bool COL1_, bool COL2_, int Q2_ = 3, int MOM_ = 0, int C1_ = 3, bool M2D1_ = false>
struct BwdVariant {
    static constexpr bool DUAL = DUAL_, OPAC = OPAC_, COL1 = COL1_, COL2 = COL2_, M2D1 = M2D1_;
    static constexpr int Q2 = Q2_, MOM = MOM_, C1 = C1_;
    static_assert(DUAL || !COL2, "COL2 needs the dual colour set");
    static_assert(!MOM || (!DUAL && OPAC && COL1), "the moment variants form every single-image gradient");
    static_assert(Q2 == 1 || Q2 == 3, "Q2 is 1 or 3 channels");
    static_assert(C1 == 3 || (C1 == 1 && COL1 && !DUAL && !MOM), "one colour sum: single-image colour variants only");
    static_assert(!M2D1 || (DUAL && OPAC && COL1 && COL2 && Q2 == 1 && !MOM && C1 == 3), "M2D1: the mapping form only");
};
// The forms written out by hand: SplaTAM tracking (the geometric sums and the depth colour of the second image),
// mapping with the first colour set's own (hx, hy) pair, and the two moment forms (1: colours precomputed, 2: SH).
using TrackVariant = BwdVariant<true, false, false, true, 1>;
using MapM2dVariant = BwdVariant<true, true, true, true, 1, 0, 3, true>;
template <int MOM>
using MomVariant = BwdVariant<false, true, true, false, 3, MOM>;
// V with one colour sum (C1 = 1)
template <class V>
using OneColour = BwdVariant<V::DUAL, V::OPAC, V::COL1, V::COL2, V::Q2, V::MOM, 1, V::M2D1>;

// Per-pair geometric terms (hx, hy, hx dx, hx dy, hy dy[, G dL/dalpha]) with
// h = G * dL/dG = (o * G) * dL/dalpha.
template <bool OPAC>
__device__ __forceinline__ void pair_geom(float* vk, float araw, float dLa, float G, v2f d) {
    // (araw dLa, G dLa), like the walk's (e Tn, alpha Tn), as one v_pk_mul_f32: the same two products, bitwise
    // the same sums as two v_mul_f32, 2 VALU per pair less (profiles/r8h_ab_pk_reduce.txt)
    if constexpr (OPAC) {
        const v2f ho = v2f{araw, G} * dLa;
        const v2f hv = ho.x * d;
        const v2f hh = hv.x * d;
        vk[0] = hv.x;
        vk[1] = hv.y;
        vk[2] = hh.x;
        vk[3] = hh.y;
        vk[4] = hv.y * d.y;
        vk[5] = ho.y;
        return;
    }
    const v2f hv = (araw * dLa) * d;  // (hx, hy)
    const v2f hh = hv.x * d;          // (hx dx, hx dy)
    vk[0] = hv.x;
    vk[1] = hv.y;
    vk[2] = hh.x;
    vk[3] = hh.y;
    vk[4] = hv.y * d.y;
    if (OPAC) vk[5] = G * dLa;
}
// Per-pair colour terms dch * dL/dpix (COL1: C1 = 3 channels, or 1 on a tile whose dL/dpix channels 1 and
// 2 are zero) and dch * dL/dpix2 (COL2, Q2 channels).
template <bool COL1, bool COL2, int Q2, int C1 = 3>
__device__ __forceinline__ void pair_colours(float* vk, float dch, v2f dp01, float dp2, float dq0, v2f dq01,
                                             float dq2) {
    if (COL1 && C1 == 1) {
        vk[0] = dch * dp01.x;
    } else if (COL1) {
        const v2f t = dch * dp01;
        vk[0] = t.x;
        vk[1] = t.y;
        vk[2] = dch * dp2;
    }
    float* v2 = vk + (COL1 ? C1 : 0);
    if (COL2 && Q2 == 1) {
        v2[0] = dch * dq0;
    } else if (COL2) {
        const v2f t = dch * dq01;
        v2[0] = t.x;
        v2[1] = t.y;
        v2[2] = dch * dq2;
    }
}
// Row totals of 4 entries x N values (entry-major) -> the LDS slots of this
// lane's entry: dst points at the entry's slot (+ the pass's value offset).
template <int N>
__device__ __forceinline__ void reduce_store(const float (&v)[4 * N], int lane, float* dst, bool store) {
    float r[RowReduce<N>::R];
    row_reduce<N>(v, r, lane);
    if (store && (lane & RowReduce<N>::WRITER_MASK) == 0) {
        float* p = dst + row_m0<N>(lane);
#pragma unroll
        for (int m = 0; m < RowReduce<N>::R; m++) p[m] = r[m];
    }
}

// Gaussians staged per batch: the per-row partial sums take 16 x batch x NV floats of LDS
// Entries staged per batch, and the batch's budget of per-(entry, block) LDS slots: each entry
// owns popcount(block mask) consecutive slots of NV floats (about 3 on average, at most 16), so a
// batch of BB entries is cut short when its masks need more than BS slots.
#ifndef GSR_BWD_BB
// batch of the variants with <= 6 sums (timing experiments may override); 144 and 160 entries (512 /
// 576 slots, still 5 waves/SIMD) measured 3-4 us slower on the config-3 tracking launch (r3 ab5)
#define GSR_BWD_BB 128
#endif
#ifndef GSR_BWD_WBB
// batch of the wide variants (> 6 sums): 96 measured faster than 64 (mapping render_bwd 362 -> 326 us) at 5
// waves/SIMD; 128 entries with a 384-slot budget (the 96-entry batch's s_acc; 2.7 blocks per entry on
// average) stay at 5 waves/SIMD and measured 3 % faster again (single-image full gradient 88 -> 85.5 us,
// config-4 dual 425 -> 410 us; profiles/r3_ab_render_bwd.txt); 448 slots drop the mapping variant to 4
#define GSR_BWD_WBB 128
#endif
template <int NV, int MOM = 0>
constexpr int bwd_batch() { return MOM ? 128 : (NV <= 6 ? GSR_BWD_BB : GSR_BWD_WBB); }
#ifndef GSR_BWD_WBS
#define GSR_BWD_WBS 384  // slot budget of the wide variants' batches
#endif
#ifndef GSR_BWD_BS
#define GSR_BWD_BS (4 * GSR_BWD_BB)  // slot budget of the batches of the variants with <= 6 sums
#endif
#ifndef GSR_BWD_M2D_BS
// slot budget of the M2D1 variant (12 sums per slot): the wide variants' 384 slots, 34.2 KB of LDS per workgroup
// -- four workgroups per CU, which is what its registers allow anyway (GSR_BWD_M2D_WAVES).  352 slots would fit
// five (32.7 KB); a batch cut short moves no sum, because an entry lives in one batch
#define GSR_BWD_M2D_BS GSR_BWD_WBS
#endif
// the moment variants (backward_power == 2): 19 / 37 sums per slot; 256 / 128 slots keep 4 workgroups per CU
template <int NV, int MOM = 0>
constexpr int bwd_slots() { return MOM == 1 ? 256 : (MOM == 2 ? 128 : (NV <= 6 ? GSR_BWD_BS : GSR_BWD_WBS)); }

// The record of V's launch (rec_sums(), gsr_launch.h) and the sums a pair forms: the record's, less the two
// colour sums a C1 = 1 tile leaves zero; the moment forms' own count
template <class V>
constexpr RecSums bwd_sums() { return rec_sums(V::OPAC, V::COL1, V::COL2, V::Q2, V::M2D1); }
template <class V>
constexpr int bwd_nv() { return V::MOM ? mom_nv(V::MOM) : bwd_sums<V>().nv - (V::COL1 ? 3 - V::C1 : 0); }
// 5 waves per SIMD (96 VGPRs; the wide variants reduce in two passes to fit), except
// the dual variants with a 3-channel second gradient (mapping-style), which spill
// at 96 VGPRs and run at 4
#ifndef GSR_BWD_WIDE_WAVES
#define GSR_BWD_WIDE_WAVES 5
#endif
#ifndef GSR_BWD_MAP_WAVES
#define GSR_BWD_MAP_WAVES 4
#endif
#ifndef GSR_BWD_M2D_WAVES
#define GSR_BWD_M2D_WAVES 4  // the M2D1 form: see render_bwd_m2d_kernel (gsr_backward.hip)
#endif
template <class V>
constexpr int bwd_waves() {
    return V::MOM ? 4 : ((V::DUAL && V::Q2 == 3) ? GSR_BWD_MAP_WAVES : ((V::OPAC && V::COL1) ? GSR_BWD_WIDE_WAVES : 5));
}

// A tile backward's shape and LDS layout (carved from one byte array, so a kernel that also runs the
// forward of the same tile -- render_track_kernel -- can alias the two phases' LDS)
template <class V>
struct BwdShape {
    static constexpr int NV = bwd_nv<V>();
    static constexpr int NV3 = V::MOM ? NV : bwd_sums<V>().nv;  // the record's sums (C1 = 3)
    static constexpr int O_COL = bwd_sums<V>().o_col, O_M1 = bwd_sums<V>().o_m1;  // colour sums, the M2D1 pair
    static constexpr int BB = bwd_batch<NV3, V::MOM>(), BS = V::M2D1 ? GSR_BWD_M2D_BS : bwd_slots<NV3, V::MOM>();
    static constexpr int RS = V::MOM ? (NV3 + 1) & ~1 : bwd_sums<V>().rec.stride;  // record stride (floats)
    static constexpr int LS = BB + 4;          // row-list stride (u32)
    // entry BB is a dummy (opacity 0, never blends) that pads the row lists; its slot BS
    // absorbs the pad entries' (zero) sums
    static constexpr int SL = BB + 1;
    // PACKC: the dual render's second colour set needs only channel 0 (Q2 = 1): staged as s_c.w (the
    // tile-rect half s_c.w carried is consumed at staging), so a pair reads one colour float4, not two
    // (no s_d array; the two-float4 staging measured 74 against 72.5 us on the config-3 dual lean launch,
    // profiles/r3_ab_render_bwd.txt)
    static constexpr bool PACKC = V::DUAL && V::Q2 == 1;
    static constexpr size_t o_a = 0, o_b = o_a + 16 * SL, o_c = o_b + 16 * SL, o_d = o_c + 16 * SL;
    static constexpr size_t o_acc = o_d + 16 * ((V::DUAL && !PACKC) ? SL : 1);
    static constexpr size_t o_list = o_acc + (4 * (BS + 1) * NV + 15) / 16 * 16;
    static constexpr size_t o_u = o_list + 4 * 16 * LS, o_mask = o_u + 4 * BB, o_base = o_mask + 2 * BB;
    static constexpr size_t o_rmax = (o_base + 2 * BB + 3) / 4 * 4;
    static constexpr size_t bytes = o_rmax + 64;
};

// One thread's pixel inputs of the tile backward: the forward's final transmittance and last
// contributor, dL/dpix of both colour sets
struct BwdPix {
    float T_final;
    uint32_t last;
    float dp0, dp1, dp2, dq0, dq1, dq2;
};
// ... of pixel (px, py), loaded from the forward's images and the incoming gradients into the caller's zeroed
// `pin` (left as it is outside the image; of dL_dpix2 the Q2 leading channels, with DUAL).  The pixel and `pin`
// come from the kernel: a loader that forms the pixel from the tile itself, or returns the record, compiles to
// other register numbers in all 21 kernels that use it
template <bool DUAL, int Q2>
__device__ __forceinline__ void load_bwd_pix(BwdPix& pin, const Camera& cam, int px, int py,
                                             const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                                             const float* __restrict__ dL_dpix, const float* __restrict__ dL_dpix2) {
    const bool inside = px < cam.W && py < cam.H;
    const int pid = py * cam.W + px;
    const int HW = cam.W * cam.H;
    if (inside) {
        pin.T_final = final_T[pid];
        pin.last = n_contrib[pid];
        pin.dp0 = dL_dpix[pid];
        pin.dp1 = dL_dpix[HW + pid];
        pin.dp2 = dL_dpix[2 * HW + pid];
        if (DUAL) {
            pin.dq0 = dL_dpix2[pid];
            if (Q2 == 3) {
                pin.dq1 = dL_dpix2[HW + pid];
                pin.dq2 = dL_dpix2[2 * HW + pid];
            }
        }
    }
}

// Per pixel the reference's back-to-front recurrence (backward.cu:966-1017)
// is carried on dot products with dL/dpixel: the colour accumulated behind the
// current Gaussian, accum_rec . dL/dpix, is one scalar A updated as
// A <- A + alpha (c . dL/dpix - A) after each contributing Gaussian (the
// reference's last_alpha / last_color / accum_rec update, one step earlier).
//
// Work split: each 16-lane row owns a 4x4-pixel block and walks its own list of
// the batch entries whose contribution ellipse reaches the block (block_mask),
// 4 entries per step; the per-pair products are summed over the row with the
// transposed in-row reduction (row_reduce) into a per-(block, entry) LDS slot,
// and after the batch one thread per entry adds its (at most 16) block slots
// in block order (deterministic) and stores ONE 48-B record per (tile,
// Gaussian) instance at its unsorted position.
// 5 workgroups per CU (<= 96 VGPRs): a 640x480 frame's 1200 tiles are all resident
// at once, so there is no second dispatch round behind the slowest tiles.
template <class V>
__device__ __forceinline__ void bwd_tile(const Camera& cam, int tile, const BwdPix& pin,
                                         const uint2* __restrict__ ranges, const PointEntry* __restrict__ point_list,
                                         const float4* __restrict__ rr, const uint32_t* __restrict__ blocksums,
                                         float* __restrict__ inst, const BwdGuard& guard, char* smem,
                                         RenderDiag& dg) {
    constexpr bool DUAL = V::DUAL, OPAC = V::OPAC, COL1 = V::COL1, COL2 = V::COL2, M2D1 = V::M2D1;
    constexpr int Q2 = V::Q2, MOM = V::MOM, C1 = V::C1;
    using L = BwdShape<V>;
    constexpr int NV = L::NV;
    constexpr int BB = L::BB, BS = L::BS, RS = L::RS, LS = L::LS;
    constexpr bool PACKC = L::PACKC;
    float4* const s_a = reinterpret_cast<float4*>(smem + L::o_a);
    float4* const s_b = reinterpret_cast<float4*>(smem + L::o_b);
    float4* const s_c = reinterpret_cast<float4*>(smem + L::o_c);
    [[maybe_unused]] float4* const s_d = reinterpret_cast<float4*>(smem + L::o_d);
    uint32_t* const s_u = reinterpret_cast<uint32_t*>(smem + L::o_u);
    uint16_t* const s_mask = reinterpret_cast<uint16_t*>(smem + L::o_mask);
    uint16_t* const s_base = reinterpret_cast<uint16_t*>(smem + L::o_base);
    float* const s_acc = reinterpret_cast<float*>(smem + L::o_acc);
    uint32_t* const s_rmax = reinterpret_cast<uint32_t*>(smem + L::o_rmax);
    uint32_t* const s_list = reinterpret_cast<uint32_t*>(smem + L::o_list);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = (tid >> 4) & 3;
    const int tx = tile % cam.gx, ty = tile / cam.gx;
    const int px = tx * TILE_X + tile_px(tid);
    const int py = ty * TILE_Y + tile_py(tid);
    const float x0 = (float)(tx * TILE_X), y0 = (float)(ty * TILE_Y);
    const uint2 range = ranges[tile];
    const float T_final = pin.T_final;
    const uint32_t last = pin.last;
    const float dp0 = pin.dp0, dp1 = pin.dp1, dp2 = pin.dp2, dq0 = pin.dq0, dq1 = pin.dq1, dq2 = pin.dq2;
    // per-block (row) maximum of the pixels' last contributor: the forward's per-tile record (one uniform
    // 64-B load, no reduction over n_contrib before the first list entries can be fetched), else reduced here
    uint32_t bmax = 0;
    int rm[4];
    if (cam.rowmax) {
        const uint4* rp = reinterpret_cast<const uint4*>(cam.rowmax + 16 * tile);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint4 q = rp[b];
            bmax = max(bmax, max(max(q.x, q.y), max(q.z, q.w)));
        }
        const uint4 qw = rp[w];  // the wave's four blocks (a second, cached 16-B load)
        rm[0] = (int)qw.x; rm[1] = (int)qw.y; rm[2] = (int)qw.z; rm[3] = (int)qw.w;
    } else {
        uint32_t rmax = last;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) rmax = max(rmax, (uint32_t)__shfl_xor((int)rmax, o));
        if ((lane & 15) == 0) s_rmax[4 * w + row] = rmax;
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 16; b++) bmax = max(bmax, s_rmax[b]);
#pragma unroll
        for (int r = 0; r < 4; r++) rm[r] = (int)s_rmax[4 * w + r];
    }
    // Instances behind every pixel's last contributor receive zero gradient.
    for (uint32_t k = range.x + bmax + tid; k < range.y; k += TILE_PIX) {
        const uint32_t gk = pe_id(point_list[k]);
        const RenderRec r = load_rr(rr, gk);
        const uint32_t u = instance_slot(rr_rect(r), rr_offset(r, blocksums, gk, cam.pre_shift), tx, ty);
        float2* dst = reinterpret_cast<float2*>(inst + (size_t)RS * u);
#pragma unroll
        for (int m = 0; m < RS / 2; m++) dst[m] = make_float2(0.f, 0.f);
    }
    // background term of dL/dalpha, -T_final / (1 - alpha) * (bg . dL/dpix) (backward.cu:1014), folded
    // into the accumulator: with A' = A - Tbg / T (Tbg = -T_final bg.dL/dpix, T the transmittance in
    // front of the current Gaussian), dL/dalpha = T_n (c . dL/dpix - A') and A' follows A's own recurrence
    // A' <- A' + alpha (c . dL/dpix - A') (T_n = T / (1 - alpha)), from A'_0 = bg . dL/dpix: the colour
    // behind the last Gaussian is the background.  Bitwise the plain recurrence when bg = 0.
    float bg_dot = cam.bg[0] * dp0 + cam.bg[1] * dp1 + cam.bg[2] * dp2;
    [[maybe_unused]] float A1 = 0.f;  // (M2D1) the first colour set's accumulator: its background term alone
    if constexpr (M2D1) A1 = bg_dot;
    if (DUAL) bg_dot += cam.bg[0] * dq0 + cam.bg[1] * dq1 + cam.bg[2] * dq2;
    const v2f pix = v2f{(float)px, (float)py};
    const v2f dp01 = v2f{dp0, dp1}, dq01 = v2f{dq0, dq1};
    const v2f dp2q0 = v2f{dp2, dq0};  // (PACKC) the colour dot's second packed pair
    // (MOM) per-pixel products of the colour gradient the colour moments need
    [[maybe_unused]] const float mdp2[3] = {dp0 * dp0, dp1 * dp1, dp2 * dp2};
    [[maybe_unused]] const float mdpp[6] = {dp0 * dp0, dp0 * dp1, dp0 * dp2, dp1 * dp1, dp1 * dp2, dp2 * dp2};
    float T = T_final, A = bg_dot;
    [[maybe_unused]] float ablate_sink = 0.f;  // (timing ablation 1)
    const int my_e = row_entry(lane);
    // Slots start zero; after every batch the used slots (those of the batch's entries, every slot a row
    // list can have written) are cleared, and the pad slot only ever receives zeros.
    constexpr bool kBulkClear = !OPAC;
    for (int q = tid; q < (BS + 1) * NV; q += TILE_PIX) s_acc[q] = 0.f;
    const uint32_t* my_list = s_list + (4 * w + row) * LS;
    if (tid == 0) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        s_a[BB] = z;
        s_b[BB] = z;
        s_c[BB] = z;
        if (DUAL && !PACKC) s_d[BB] = z;
    }
    // Batch staging, software-pipelined two batches deep: thread t < batch holds entry t's
    // render record (already in its LDS form) and block-sum word for the next batch, and the
    // sorted list entry for the batch after it, so neither dependent load (list entry ->
    // record) is waited on while a batch is rasterised; the instance slot is formed at staging.
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pb = pa, pc = pa, pd = pa;
    uint32_t pbs = 0, pm = 0, prh = 0;  // prh: tile-rect hi (q3.w) when q3 is not staged
    PointEntry pn = 0;
    auto fetch_entry = [&](int hi_) {
        if (tid < min(BB, hi_)) pn = point_list[range.x + (uint32_t)(hi_ - 1 - tid)];
    };
    auto fetch_rec = [&](int hi_) {
        if (tid < min(BB, hi_)) {
            const uint32_t gi = pe_id(pn);
            pm = pe_mask(pn);
            const RenderRec r = load_rr(rr, gi);
            pbs = blocksums[gi >> cam.pre_shift];
            pa = r.q0; pb = r.q1; pc = r.q2;
            if (DUAL && !PACKC) {
                pd = r.q3;
            } else {
                prh = __float_as_uint(r.q3.w);
                if (PACKC) pd.x = r.q3.x;
            }
        }
    };
    fetch_entry((int)bmax);
    fetch_rec((int)bmax);
    fetch_entry((int)bmax - BB);
    const uint32_t mean4 = sched_mean4(cam, guard.counters);
    const bool multi_round = sched_multi_round(cam);
    int hi_pf = (int)bmax;  // the batch start the staged registers hold
    dg.phase(0);
    for (int hi = (int)bmax; hi > 0;) {
        prio_by_remaining(hi, mean4, multi_round);
        if (hi != hi_pf) {  // the previous batch was cut by its slot budget: re-fetch (rare)
            fetch_entry(hi);
            fetch_rec(hi);
            fetch_entry(hi - BB);
        }
        const int cmax = min(BB, hi);
        int ts_ = tid;
        asm volatile("" : "+v"(ts_));  // staging addresses formed here, not hoisted across the batch loop
        if (ts_ < cmax) {
            s_u[ts_] = instance_slot(make_uint2(__float_as_uint(pc.w), (DUAL && !PACKC) ? __float_as_uint(pd.w) : prh),
                                     pbs + __float_as_uint(pb.w), tx, ty);
            s_a[ts_] = pa;
            s_b[ts_] = pb;
            s_c[ts_] = PACKC ? make_float4(pc.x, pc.y, pc.z, pd.x) : pc;
            if (DUAL && !PACKC) s_d[ts_] = pd;
            s_mask[ts_] = (uint16_t)pm;  // the instance's exact 4x4-block mask (sorted list entry)
        }
        __syncthreads();
        dg.phase(1);
        fetch_rec(hi - BB);        // records of the next batch (list entries loaded a batch ago)
        fetch_entry(hi - 2 * BB);  // list entries of the batch after it
        hi_pf = hi - BB;
        // entries j with pos = hi-1-j >= rmax lie behind every pixel of the block
        const int jmin[4] = {hi - rm[0], hi - rm[1], hi - rm[2], hi - rm[3]};
        // list words: (LDS byte offset of entry j's staged record, 16 j) | (byte offset of its slot) << 16
        static_assert(16 * BB < 65536 && (BS + 1) * NV * 4 < 65536, "list words hold 16-bit byte offsets");
        SlotLists sl = build_row_slot_lists(s_mask, s_base, cmax, BS, w, jmin, s_list + 4 * w * LS, LS,
                                            (uint32_t)(16 * BB) | ((uint32_t)(BS * NV * 4) << 16), 16u,
                                            (uint32_t)(NV * 4));
        if constexpr (kDupPhase == 3) {  // (VALU census only: the same lists again)
            asm volatile("" ::: "memory");
            sl = build_row_slot_lists(s_mask, s_base, cmax, BS, w, jmin, s_list + 4 * w * LS, LS,
                                      (uint32_t)(16 * BB) | ((uint32_t)(BS * NV * 4) << 16), 16u, (uint32_t)(NV * 4));
        }
        const int n = sl.len, cnt = sl.cnt;
        dg.phase(2);
        const int jlo16 = 16 * (hi - (int)last);  // pos = hi-1-j < last  <=>  j >= jlo  <=>  16 j >= 16 jlo
        for (int i = 0; i < n; i += 4) {
            // this lane's entry slot (the reduction's writer lanes): the high half of its entry's word
            const uint32_t soff = reinterpret_cast<const uint16_t*>(my_list + i + my_e)[1];
            // byte offsets 16 j of the step's entries in s_a / s_b / s_c / s_d: the low halves of the four
            // words, one ds_read_u16 each (zero-extended by the load: no v_and per entry on the VALU)
            int jb[4];
#pragma unroll
            for (int k = 0; k < 4; k++) jb[k] = (int)reinterpret_cast<const uint16_t*>(my_list + i + k)[0];
            auto rec = [&](const float4* arr, int k) {
                return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(arr) + jb[k]);
            };
            v2f d[4];
            float G[4], araw[4], alpha[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float4 a = rec(s_a, k), b = rec(s_b, k);
                d[k] = pix_delta(a, pix);
                const float p2 = eval_p2(a, b, d[k]);                       // log2(e) * power
                // position in the tile list before the pixel's last contributor, power <= 0, alpha >= 1/255
                // (alpha = min(0.99, araw) >= 1/255 <=> araw >= 1/255); the pad entry has opacity 0.
                // Non-contributing pairs continue with alpha 0: T and A then pass through unchanged
                // (1 / (1 - 0) == 1 exactly).  Without the opacity sum the mask is applied to araw (a
                // masked pair's h = araw dL/dalpha is then 0, and G may even be inf there); with it,
                // G dL/dalpha needs a finite G and a masked dL/dalpha.
                G[k] = __builtin_amdgcn_exp2f(OPAC ? fminf(p2, 0.f) : p2);
                const float ar = b.y * G[k];
                ok[k] = jb[k] >= jlo16 && p2 <= 0.0f && ar >= 1.0f / 255.0f;
                araw[k] = (OPAC || ok[k]) ? ar : 0.f;
                alpha[k] = fminf(0.99f, araw[k]);
                if (OPAC) alpha[k] = ok[k] ? alpha[k] : 0.f;
            }
            {
                bool pad[4];
#pragma unroll
                for (int k = 0; k < 4; k++) pad[k] = jb[k] == 16 * BB;
                dg.step(pad, ok);
            }
            // (no wave-uniform skip of steps without a contributing pair: 0.04 % of steps, and the test
            // cost 2 VALU + a branch per step; config-4 dual 396 -> 387 us without it)
            // serial part (in list order): T and A, then dL/dalpha and dchannel/dcolor
            float dLa[4], dch[4];
            [[maybe_unused]] float h1[4];  // (M2D1) araw dL/dalpha of the first colour set alone
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float4 c = rec(s_c, k);
                float cd;
                if (PACKC) {  // (c.x, c.y) . dp01 + (c.z, c.w) . (dp2, dq0): pk_mul + pk_fma + add
                    const v2f t = __builtin_elementwise_fma(v2f{c.z, c.w}, dp2q0, v2f{c.x, c.y} * dp01);
                    cd = t.x + t.y;
                } else if (DUAL) {
                    const float4 c2 = rec(s_d, k);
                    const v2f t = v2f{c.x, c.y} * dp01 + v2f{c2.x, c2.y} * dq01;
                    cd = __builtin_fmaf(c.z, dp2, __builtin_fmaf(c2.z, dq2, t.x + t.y));
                } else if (C1 == 1) {  // dL/dpix channels 1, 2 zero on this tile: the same value (up to a zero's sign)
                    cd = c.x * dp0;
                } else {
                    const v2f t = v2f{c.x, c.y} * dp01;
                    cd = __builtin_fmaf(c.z, dp2, t.x + t.y);
                }
                const float inv = __builtin_amdgcn_rcpf(1.f - alpha[k]);   // v_rcp_f32 (~1 ulp)
                const float Tn = T * inv;                                   // T / (1 - alpha), backward.cu:978
                const float e = cd - A;
                const v2f xd = v2f{e, alpha[k]} * Tn;  // (e Tn, alpha Tn): one v_pk_mul_f32, the same two products
                const float x = xd.x;
                dch[k] = xd.y;                          // 0 when masked
                dLa[k] = (OPAC && !ok[k]) ? 0.f : x;    // (without OPAC: h = araw dLa is 0 when masked)
                if constexpr (M2D1) {  // the single-image variant's operations, on the first colour set alone
                    const v2f t1 = v2f{c.x, c.y} * dp01;
                    const float e1 = __builtin_fmaf(c.z, dp2, t1.x + t1.y) - A1;
                    const float x1 = e1 * Tn;
                    h1[k] = araw[k] * (ok[k] ? x1 : 0.f);
                    A1 = __builtin_fmaf(alpha[k], e1, A1);
                }
                T = Tn;  // masked pairs: alpha = 0 and v_rcp_f32(1) == 1 exactly (tools/micro/rcp_one.hip)
                A = __builtin_fmaf(alpha[k], e, A);     // unchanged when masked
            }
            // Per pair: (hx, hy, hx*dx, hx*dy, hy*dy, G*dL/dalpha, dch*dL/dpix, dch*dL/dpix2) with
            // h = G * dL/dG = (o * G) * dL/dalpha.  gauss_bwd turns them into the reference's
            // per-pair quantities (backward.cu:1020-1038): dmean2D = -ddel * (Q [hx, hy]),
            // dconic = -0.5 * (hxx, hxy, hyy); both are linear in the sums (Q is per Gaussian).
            float* dst = reinterpret_cast<float*>(reinterpret_cast<char*>(s_acc) + soff);  // the (entry, block) slot
            if constexpr (MOM > 0) {  // backward_power == 2: the pair's second moments (gauss_bwd_mom_kernel)
                MomIn e[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const v2f ho = v2f{araw[k], G[k]} * dLa[k];
                    const float h = ho.x, o = ho.y;
                    const float hx = h * d[k].x, hy = h * d[k].y;
                    e[k].m20 = hx * hx;
                    e[k].m11 = hx * hy;
                    e[k].m02 = hy * hy;
                    e[k].dx = d[k].x;
                    e[k].dy = d[k].y;
                    e[k].xx = d[k].x * d[k].x;
                    e[k].xy = d[k].x * d[k].y;
                    e[k].yy = d[k].y * d[k].y;
                    e[k].o2 = o * o;
                    e[k].c2 = dch[k] * dch[k];
                    const float hc = h * dch[k];
                    e[k].hc[0] = hc * dp0;
                    e[k].hc[1] = hc * dp1;
                    e[k].hc[2] = hc * dp2;
                }
                // passes of 4 moments (the reduction's cost is per value: the pass size only sets how
                // many products are live at once)
                mom_pass<MOM, 0, 4>(e, mdp2, mdpp, lane, dst);
                mom_pass<MOM, 4, 4>(e, mdp2, mdpp, lane, dst);
                mom_pass<MOM, 8, 4>(e, mdp2, mdpp, lane, dst);
                if constexpr (MOM == 1) {
                    mom_pass<MOM, 12, 4>(e, mdp2, mdpp, lane, dst);
                } else {
                    mom_pass<MOM, 12, 4>(e, mdp2, mdpp, lane, dst);
                    mom_pass<MOM, 16, 4>(e, mdp2, mdpp, lane, dst);
                    mom_pass<MOM, 20, 4>(e, mdp2, mdpp, lane, dst);
                    mom_pass<MOM, 24, 5>(e, mdp2, mdpp, lane, dst);
                    mom_pass<MOM, 29, 5>(e, mdp2, mdpp, lane, dst);
                }
            } else if constexpr (NV <= 6) {  // one reduction over all values
                float v[4 * NV];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    pair_geom<OPAC>(v + NV * k, araw[k], dLa[k], G[k], d[k]);
                    pair_colours<COL1, COL2, Q2, C1>(v + NV * k + L::O_COL, dch[k], dp01, dp2, dq0, dq01, dq2);
                }
                if constexpr (kAblate == 1) {
#pragma unroll
                    for (int q = 0; q < 4 * NV; q++) ablate_sink += v[q];
                } else {
                    reduce_store<NV>(v, lane, dst, true);
                }
            } else {  // wide variants: geometric (+ opacity), then colour sums (register pressure).  G dL/dalpha
                // rides with the 5 geometric sums: 6 + 6 instead of 5 + 7 sums for mapping is 84 instead of 96 DPP
                // adds per step (render_bwd 312 -> 303 us at config 4, profiles/r3_split_ab.txt)
                constexpr int NA = L::O_COL, NB = (M2D1 ? L::O_M1 : NV) - NA;
                if constexpr (M2D1) {  // the pair first, a pass of its own: h1 is dead before the wide passes
                    float v[4 * 2];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const v2f m = h1[k] * d[k];
                        v[2 * k] = m.x;
                        v[2 * k + 1] = m.y;
                    }
                    reduce_store<2>(v, lane, dst + L::O_M1, true);
                }
                {
                    float v[4 * NA];
#pragma unroll
                    for (int k = 0; k < 4; k++) pair_geom<OPAC>(v + NA * k, araw[k], dLa[k], G[k], d[k]);
                    reduce_store<NA>(v, lane, dst, true);
                }
                {
                    float v[4 * NB];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        pair_colours<COL1, COL2, Q2, C1>(v + NB * k, dch[k], dp01, dp2, dq0, dq01, dq2);
                    }
                    reduce_store<NB>(v, lane, dst + NA, true);
                }
            }
        }
        dg.phase(3);
        __syncthreads();
        dg.phase(4);
        // Entry totals: TPE threads per entry, thread q of an entry owns values m = q, q + TPE, ...
        // and adds the entry's consecutive block slots in ascending block order (deterministic);
        // the TPE threads store adjacent floats of the packed record.
        constexpr int TPE = TILE_PIX / BB, NQ = (NV + TPE - 1) / TPE, NQR = (RS + TPE - 1) / TPE;
        int t_ = tid;
        asm volatile("" : "+v"(t_));  // addresses formed here, not hoisted across the batch loop (VGPRs)
        const int e = t_ / TPE, q = t_ % TPE;
        if (kAblate != 2 && e < cnt) {
            float c[NQ];
#pragma unroll
            for (int i = 0; i < NQ; i++) c[i] = 0.f;
            const int nb = __popc((uint32_t)s_mask[e]);
            float* src = s_acc + (int)s_base[e] * NV;
            for (int b = 0; b < nb; b++, src += NV) {
#pragma unroll
                for (int i = 0; i < NQ; i++)
                    if (q + TPE * i < NV) {
                        c[i] += src[q + TPE * i];
                        if constexpr (!kBulkClear) src[q + TPE * i] = 0.f;
                    }
            }
            float* dst = inst + (size_t)RS * s_u[e];  // packed record (RecLayout): the NV sums, zero pad
#pragma unroll
            for (int i = 0; i < NQR; i++)
                if (q + TPE * i < RS) {
                    // (plain stores: streaming stores measured neutral for render_bwd and 3-9 us slower for the
                    // gauss_bwd that reads the records next: profiles/r4l_ab_nt.txt, r4m_ab_nt_tail.txt)
                    const float val = i < NQ ? c[i] : 0.f;  // (C1 = 1: the two absent colour sums are zero)
                    dst[q + TPE * i] = val;
                }
        }
        dg.phase(5);
        __syncthreads();
        // The batch's slots back to zero for the next batch's reduction: the used range [0, slots of entries
        // < cnt) as contiguous float4 stores (the next batch's staging barrier orders them before its walk).
        // Re-zeroing each slot right after reading it cost bank-conflicted scattered stores in the totals
        // (slot stride NV = 6 words: entries whose slot bases differ by 16 share banks).  Only in the lean
        // variants (no opacity gradient: the tracking render): the full-gradient ones are at their VGPR
        // bound, where the sweep's bookkeeping spilled (render_bwd<1,1,1,1,1,0>: 16 B of scratch, +10 us at
        // config 4), so they keep re-zeroing in the totals
        if constexpr (kBulkClear) {
            const int used = cnt > 0 ? (int)s_base[cnt - 1] + __popc((uint32_t)s_mask[cnt - 1]) : 0;
            float4* const a4 = reinterpret_cast<float4*>(s_acc);
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q4 = tid; q4 < (used * NV + 3) / 4; q4 += TILE_PIX) a4[q4] = z;
        }
        dg.phase(6);
        dg.batch();
        hi -= cnt;
    }
    if (kAblate == 1 && ablate_sink == 1.2345f) inst[0] = ablate_sink;  // keeps the per-pair values alive
}

template <bool DUAL, bool OPAC, bool COL1, bool COL2, int Q2 = 3, int MOM = 0>
__global__ void __launch_bounds__(TILE_PIX, (bwd_waves<BwdVariant<DUAL, OPAC, COL1, COL2, Q2, MOM>>()))
render_bwd_kernel(Camera cam, const uint2* __restrict__ ranges, const PointEntry* __restrict__ point_list,
                  const float4* __restrict__ rr, const uint32_t* __restrict__ blocksums,
                  const float* __restrict__ final_T,
                  const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dpix,
                  const float* __restrict__ dL_dpix2, float* __restrict__ inst, BwdGuard guard,
                  unsigned long long* clk) {
    using V = BwdVariant<DUAL, OPAC, COL1, COL2, Q2, MOM>;
    kclock_begin(clk);
    RenderDiag dg;  // (diagnostics builds only, gsr_diag.h)
    dg.begin();
    if (guard.overflow()) {  // invalid forward state (static-mode overflow): touch nothing
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
    load_bwd_pix<DUAL, Q2>(pin, cam, px, py, final_T, n_contrib, dL_dpix, dL_dpix2);
    if constexpr (!DUAL && COL1 && MOM == 0) {
        // a tile whose incoming gradient has zero channels 1 and 2 everywhere (SplaTAM's depth/silhouette
        // render: get_loss differentiates only its depth channel, scripts/splatam.py:262-270) forms one colour
        // sum per pair instead of three; the others are exactly zero (records identical up to a zero's sign)
        if (!__syncthreads_or(pin.dp1 != 0.f || pin.dp2 != 0.f)) {
            bwd_tile<OneColour<V>>(cam, tile, pin, ranges, point_list, rr, blocksums, inst, guard, smem, dg);
            dg.end();
            kclock_end(clk);
            return;
        }
    }
    bwd_tile<V>(cam, tile, pin, ranges, point_list, rr, blocksums, inst, guard, smem, dg);
    dg.end();
    kclock_end(clk);
}
// The kernel of a named variant (its first six members are the kernel's arguments)
template <class V>
constexpr auto render_bwd_of() {
    static_assert(V::C1 == 3 && !V::M2D1, "render_bwd_kernel picks C1 per tile; M2D1 is render_bwd_m2d_kernel");
    return &render_bwd_kernel<V::DUAL, V::OPAC, V::COL1, V::COL2, V::Q2, V::MOM>;
}

}  // namespace gsr
