// gsr_launch.h -- the kernel launchers of every translation unit, with the argument records only they
// need, for the files that launch them (gsr_capi.hip) or define them.  Grouped by the defining file.
#pragma once
#include "gsr_adam.h"
#include "gsr_layout.h"

namespace gsr {

// ---------------------------------------------------- gsr_preprocess.hip --
hipError_t launch_preprocess(const Camera& cam, const GaussIn& g, GeomPtrs geo, int* radii, uint32_t* counts,
                             bool lds_hist, int ntiles, int nb, hipStream_t s, unsigned long long* clk = nullptr);
hipError_t launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* vis, hipStream_t s);
// ------------------------------------------------------- gsr_binning.hip --
hipError_t launch_tile_colscan(uint32_t* counts, int nb, int ntiles, uint32_t* tot, GeomPtrs geo, uint2* ranges,
                               uint32_t* status, bool tail, hipStream_t s, unsigned long long* clk = nullptr,
                               Gate gate = Gate{});
hipError_t launch_scan_counts(GeomPtrs geo, int nb, const uint32_t* tile_count, int tile_stride, int ntiles,
                              uint2* ranges, uint32_t* status, hipStream_t s);
// Row-major render schedule (the paths that do not run tile_plan).
hipError_t launch_identity_order(uint32_t* order, int ntiles, hipStream_t s);
// lds_hist: the colscan ran without its scan tail; every workgroup scans the workgroup and tile totals (`tot`)
// itself, workgroup 0 writes ranges, counters and `status` (static mode; may be null).
hipError_t launch_duplicate_bucket(const Camera& cam, int P, GeomPtrs geo, uint2* ranges, const uint32_t* tot,
                                   uint32_t* cursor, bool lds_hist, int ntiles, uint64_t* keys, uint64_t* point_list,
                                   int nb, SpecGuard guard, uint32_t* status, hipStream_t s, unsigned long long* clk = nullptr);
// --------------------------------------------------------- gsr_radix.hip --
hipError_t launch_duplicate(const Camera& cam, int P, GeomPtrs geo, uint64_t* keys, uint32_t* gid,
                            int nb, hipStream_t s);
hipError_t launch_radix_sort(uint64_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t n, int nsb, int npass,
                             hipStream_t s);
hipError_t launch_gather_ids(const uint32_t* vals, const uint32_t* gid, uint64_t* point_list, uint32_t n, hipStream_t s);
// ------------------------------------------------------- gsr_forward.hip --
// SplaTAM's tracking L1 loss (get_loss tracking=True, scripts/splatam.py:262-296) and its
// gradient images formed in the dual forward's per-pixel epilogue (gsr_track_forward_dual_static):
// the same mask / sums / sign gradient as gsr_track_l1_fwd_bwd, without reading the images back.
struct TrackL1 {
    const float* gt_im;     // [3,H,W]
    const float* gt_depth;  // [1,H,W]
    float sil_thres, w_im, w_depth;
    const float* seed;      // dL/dloss (device scalar, read when the kernel runs)
    float* dL_dim;          // [3,H,W]
    float* dL_dds;          // [3,H,W] (channels 1, 2 written as zero)
    float* scratch;         // arrival counters (zero between launches), then 2 partials per tile
    float* loss;            // device scalar
    float* terms;           // NULL, or 2 floats next to the loss: {w_im * image sum, w_depth * depth sum}
};
int track_l1_fused_scratch_floats(int ntiles);
// keys: the unsorted tile buckets (render_fwd sorts each tile's bucket into point_list in
// its prologue; the keys are scratch afterwards); nullptr when point_list is already
// sorted (radix fallback)
hipError_t launch_render_fwd(const Camera& cam, const uint2* ranges, uint64_t* point_list, uint64_t* keys,
                             GeomPtrs geo, const float* colors2, float* final_T, uint32_t* n_contrib,
                             float* out_color, float* out_color2, float* out_depth, SpecGuard guard, hipStream_t s,
                             unsigned long long* clk = nullptr, const TrackL1* l1 = nullptr);
// --------------------------------------------------------- gsr_reuse.hip --
// geometry reuse (gsr_forward_reuse): the render records' colours replaced by `colors` [P,3]
hipError_t launch_recolour(int P, const float* colors, GeomPtrs geo, hipStream_t s, Gate gate = Gate{});
// gated geometry reuse: geom [0, counters) + counters[0..3] and the radii from the previous call, the render
// records' colour quarter replaced by this call's colours (recolour fused into the copy)
hipError_t launch_reuse_copy(Gate gate, const void* prev_geom, void* geom, size_t geom_bytes, size_t tiles_offset,
                             const float* colors, const int* prev_radii, int* radii, int P, hipStream_t s);
struct EqualPairs {
    int npairs;
    const float* a[8];
    const float* b[8];
    long long n[8];
};
// *word = e when any pair differs bitwise (word not cleared: see Gate)
hipError_t launch_epoch_mismatch(const EqualPairs& q, uint32_t* word, uint32_t e, hipStream_t s);
hipError_t launch_bitwise_equal(const EqualPairs& q, int* flag, hipStream_t s);
// ------------------------------------------------------ gsr_backward.hip --
// (the tile backward its render kernels inline, bwd_tile, and render_bwd_kernel itself: gsr_render_bwd.h)
// the tracking iteration's forward (+ L1) and render backward in one launch (gsr_backward.hip); inst receives
// the pose-fused gauss_bwd's per-instance records (track_records_floats)
hipError_t launch_render_track(const Camera& cam, const uint2* ranges, uint64_t* point_list, uint64_t* keys,
                               GeomPtrs geo, float* final_T, uint32_t* n_contrib, float* out_color,
                               float* out_color2, float* out_depth, SpecGuard guard, const TrackL1& l1, float* inst,
                               hipStream_t s, unsigned long long* clk = nullptr);
int track_records_stride();  // floats per instance record of the tracking render backward (6)
// Per-(tile, Gaussian) instance record of the power-1 backward: the per-pair sums
// the launched render_bwd variant forms, packed (no slots for absent terms):
// [hx, hy, hxx, hxy, hyy | G dL/dalpha (o_op) | dch dp (o_c1, 3) | dch dq (o_c2, n_c2)]
// padded to an even count (float2 stores); 6 floats (24 B) for SplaTAM tracking.
struct RecLayout {
    int stride;                 // floats per record (even)
    int o_op, o_c1, o_c2, n_c2; // offsets, -1 when absent
};
// The one statement of that layout: the record of a variant that forms the opacity sum (op), the colour sums
// (c1: three slots, also where a tile forms one, bwd_tile's C1 = 1), q2 second-colour sums (c2) and the first
// colour set's own (hx, hy) pair (m2d).  BwdShape (gsr_render_bwd.h) sizes the tile backward from it, and
// bwd_rec_layout() hands its `rec` to gauss_bwd.
struct RecSums {
    RecLayout rec;
    int o_col;  // where the colour sums start: the geometric sums and the opacity sum lie before it
    int o_m1;   // the M2D1 pair, -1 when absent
    int nv;     // sums per record (stride: nv rounded up to even)
};
constexpr RecSums rec_sums(bool op, bool c1, bool c2, int q2, bool m2d = false) {
    RecSums s{};
    int nv = 5;
    s.rec.o_op = op ? nv : -1;
    nv += op ? 1 : 0;
    s.o_col = nv;
    s.rec.o_c1 = c1 ? nv : -1;
    nv += c1 ? 3 : 0;
    s.rec.o_c2 = c2 ? nv : -1;
    s.rec.n_c2 = c2 ? q2 : 0;
    nv += s.rec.n_c2;
    s.o_m1 = m2d ? nv : -1;
    nv += m2d ? 2 : 0;
    s.nv = nv;
    s.rec.stride = (nv + 1) & ~1;
    return s;
}
static_assert(rec_sums(true, true, true, 3).rec.stride == INST_REC_MAX && rec_sums(true, true, true, 1, true).nv == INST_REC_MAX,
              "INST_REC_MAX: the largest records, every sum of a dual render and the M2D1 form");
RecLayout bwd_rec_layout(unsigned need, bool dual);
hipError_t launch_render_bwd(const Camera& cam, const uint2* ranges, const uint64_t* point_list, GeomPtrs geo,
                             const float* final_T, const uint32_t* n_contrib, const float* dL_dpix,
                             const float* colors2, const float* dL_dpix2, unsigned need, float* inst, BwdGuard guard,
                             hipStream_t s, unsigned long long* clk = nullptr);
// which optional per-pair sums render_bwd forms (the geometric ones always)
constexpr unsigned NEED_OPACITY = 1u, NEED_COLORS = 2u, NEED_COLORS2 = 4u;
constexpr unsigned NEED_DL2_CH0_ONLY = 8u;  // dL_dpix2 channels 1, 2 are promised zero
struct GradsOut {
    float* dmeans2D;
    float* dcolors;
    float* dopacity;
    float* dmeans3D;
    float* dcov3D;
    float* dsh;
    float* dscales;
    float* drot;
    float* dcolors2;  // second colour set of a dual render (nullptr otherwise)
};
// gsr_backward_dual_m2d: the mapping form's render backward with the first colour set's own (hx, hy) sums
// (bwd_tile's M2D1) and the per-Gaussian backward that turns them into that set's means2D gradient.  The
// record is the mapping variant's ten sums, then the pair at M2D_REC_PAIR: 12 floats, the stated maximum.
// M2dOut is a record of its own, not a field of RecLayout / GradsOut: those are by-value arguments of every
// gauss_bwd_kernel instantiation, whose argument layout (and device code) must not move.
constexpr int M2D_REC_PAIR = rec_sums(true, true, true, 1, true).o_m1;
static_assert(M2D_REC_PAIR == 10, "the mapping variant's ten sums, then the pair");
struct M2dOut {
    float* dmeans2D_c1 = nullptr;  // [P,3]: (x, y) in NDC units like dmeans2D, z written as 0
    int o_m1 = -1;                 // record offset of the pair, -1 when absent
};
int m2d_record_stride();
hipError_t launch_render_bwd_m2d(const Camera& cam, const uint2* ranges, const uint64_t* point_list, GeomPtrs geo,
                                 const float* final_T, const uint32_t* n_contrib, const float* dL_dpix,
                                 const float* dL_dpix2, float* inst, BwdGuard guard, hipStream_t s,
                                 unsigned long long* clk = nullptr);
hipError_t launch_gauss_bwd_m2d(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii, const float* inst,
                                RecLayout rec, const GradsOut& out, M2dOut m1, BwdGuard guard, hipStream_t s,
                                unsigned long long* clk = nullptr);
// Tracking (gsr_track_backward_dual): the pose gradient -- and the pose Adam step -- fused into
// gauss_bwd, whose per-Gaussian dL/dmeans_cam, dL/d[z,1,z^2] and (anisotropic) dL/drotation
// never leave registers.  Same maths as track_transform_bwd_kernel (gsr_glue.hip).
struct PoseFuse {
    const float* means_world;  // [P,3]
    const float* unnorm_rot;   // [P,4]
    int scols;                 // 1: isotropic map (rotation does not depend on the pose)
    float* cam_q;              // frame's quaternion column (stride qs)
    float* cam_t;              // frame's translation column (stride qs)
    int qs;
    const float* w2c;          // [16] row-major, depth colours
    float* scratch;            // arrival counters (zero between launches), 16 * nblocks partials, group sums
    float* adam_state;         // 15 floats (nullptr: write dq / dt instead)
    double lr_q, lr_t, beta1, beta2, eps;
    float* dq;                 // gradient outputs when adam_state == nullptr
    float* dt;
    const uint32_t* guard = nullptr;  // the forward's counters + capacity (Adam skipped on an overflow)
    uint32_t cap = 0;
    const float* loss = nullptr;      // best-candidate selection (PoseAdam::loss / best)
    float* best = nullptr;
    // log_scales [P, scols]: recompute each Gaussian's camera-frame mean / rotation / scale from the
    // world-frame map and the (pre-step) pose instead of reading GaussIn's arrays (the forward ran the
    // transform inside preprocess without storing them); nullptr: read GaussIn
    const float* ls = nullptr;
};
int pose_fuse_scratch_floats(int P);
hipError_t launch_gauss_bwd(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii, const float* inst,
                            RecLayout rec, const GradsOut& out, BwdGuard guard, hipStream_t s,
                            const PoseFuse* pose = nullptr, unsigned long long* clk = nullptr);
hipError_t launch_selftest_reduce9(const float* in, float* out, hipStream_t s);
// ------------------------------------------------------------ gsr_sh.hip --
// gsr_sh.hip: SH colour stages with LDS-staged, coalesced coefficient traffic
bool sh_staged(const Camera& cam, const GaussIn& g);
hipError_t launch_sh_eval(const Camera& cam, const GaussIn& g, GeomPtrs geo, hipStream_t s);
// The mapping optimizer's colour group applied to the SH coefficients inside sh_bwd (m == nullptr: none):
// torch.optim.Adam's element update with the scalars formed on the host like the other fused steps.
struct ShAdam {
    float* m = nullptr;
    float* v = nullptr;
    float ss = 0.f;
    AdamCoef c = {0.f, 0.f, 0.f, 1.f, 0.f};
    const uint32_t* guard = nullptr;  // the forward's status row / counters: skip the step on an overflow
    uint32_t cap = 0;
    uint32_t* halted = nullptr;       // gsr_map_adam.halted (sticky skip)
};
hipError_t launch_sh_bwd(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii, const float* drgb,
                         float* dmeans3D, float* dsh, BwdGuard guard, hipStream_t s, const ShAdam& sa = ShAdam{});
// ------------------------------------------------ gsr_backward_power.hip --
// backward_power != 1 (the vendored renderCUDAFused semantics, backward.cu:850-1140)
constexpr int JAC_FLOATS = 84;  // per-Gaussian linear chain pack, see gsr_backward_power.hip
constexpr int JAC_CONIC = 80;   // conic (A, B, C) inside the pack
int power_record_floats(int nsh);  // values stored per instance record
hipError_t launch_gauss_jac(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii, float* jac,
                            hipStream_t s);
hipError_t launch_render_bwd_power(const Camera& cam, const GaussIn& g, const uint2* ranges,
                                   const uint64_t* point_list, GeomPtrs geo, const float* jac, const float* final_T,
                                   const uint32_t* n_contrib, const float* dL_dpix, int power, float* rec,
                                   BwdGuard guard, hipStream_t s);
// Fisher-selective backward_power path (dL/dmeans3D + dL/dopacity only, colours precomputed):
// gauss_mpack (3x5 chain matrix per Gaussian, MPACK_FLOATS), render_bwd_fisher (4-float records), sums
constexpr int MPACK_FLOATS = 16;
hipError_t launch_gauss_mpack(const Camera& cam, const GaussIn& g, const int* radii, float* mpack, hipStream_t s);
hipError_t launch_render_bwd_fisher(const Camera& cam, const uint2* ranges, const uint64_t* point_list, GeomPtrs geo,
                                    const float* mpack, const float* final_T, const uint32_t* n_contrib,
                                    const float* dL_dpix, int power, float* rec, BwdGuard guard, hipStream_t s);
hipError_t launch_gauss_bwd_fisher(int P, GeomPtrs geo, const int* radii, const float* rec, float* dmeans3D,
                                   float* dopacity, BwdGuard guard, hipStream_t s);
hipError_t launch_gauss_bwd_power(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii,
                                  const float* rec, const GradsOut& out, BwdGuard guard, hipStream_t s);
// backward_power == 2 through per-instance second moments: render_bwd_kernel's MOM variants (gsr_render_bwd.h,
// instantiated by gsr_backward_power.hip) and gauss_bwd_mom_kernel
int moments_record_floats(bool sh);
hipError_t launch_render_bwd_moments(const Camera& cam, const uint2* ranges, const uint64_t* point_list, GeomPtrs geo,
                                     const float* final_T, const uint32_t* n_contrib, const float* dL_dpix, bool sh,
                                     float* inst, BwdGuard guard, hipStream_t s);
hipError_t launch_gauss_bwd_moments(const Camera& cam, const GaussIn& g, GeomPtrs geo, const int* radii,
                                    const float* inst, const GradsOut& out, BwdGuard guard, hipStream_t s);

}  // namespace gsr
