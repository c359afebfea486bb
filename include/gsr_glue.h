/* gsr_glue.h -- fused SplaTAM caller glue around the rasterizer.
 *
 * SplaTAM's tracking iteration (scripts/splatam.py:220-353, tracking=True)
 * spends more GPU time in ~300 small torch kernels around the two rasterizer
 * calls than in the rasterizer itself.  These entry points restate that glue
 * as a handful of HIP kernels with exactly the reference's math:
 *
 *   gsr_track_transform_fwd / _bwd
 *       transform_to_frame(params, t, gaussians_grad=False, camera_grad=True)
 *           (utils/slam_helpers.py:252-304)
 *       + transformed_params2rendervar / ...depthplussilhouette rotations,
 *         opacities and scales (slam_helpers.py:124-139, 234-249)
 *       + get_depth_and_silhouette colours [z, 1, z^2] (slam_helpers.py:196-213)
 *       Backward: gradient w.r.t. the frame's unnormalised camera quaternion and
 *       translation only (the Gaussians are detached in tracking), through
 *       F.normalize, build_rotation's own normalisation (slam_external.py:25-42)
 *       and, for anisotropic maps, quat_mult(cam_rot, normalize(q)).
 *       Deterministic: fixed-order two-level reduction.
 *
 *   gsr_track_l1_fwd / _bwd
 *       get_loss's tracking L1 terms (splatam.py:262-296 with use_l1,
 *       use_sil_for_loss, ignore_outlier_depth_loss=False): mask =
 *       (gt_depth > 0) & !isnan(depth) & !isnan(depth_sq - depth^2) &
 *       (silhouette > sil_thres); loss = w_im * sum(mask * |gt_im - im|) +
 *       w_depth * sum(mask * |gt_depth - depth|), and its gradient w.r.t. the
 *       RGB render and the [depth, silhouette, depth^2] render.
 *
 * All pointers are device float32 (contiguous), sizes in elements, `stream`
 * a hipStream_t.  Return GSR_OK (0) or a negative GSR_ERR_* (see gsr.h).
 */
#ifndef GSR_GLUE_H
#define GSR_GLUE_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Reduction scratch -- one contract for every `scratch` argument of this header
 * (gsr_track_transform_bwd(_adam), gsr_track_l1_fwd(_bwd), gsr_track_forward_*_static*,
 * gsr_track_backward_dual(_records), gsr_map_loss_fwd):
 *   - layout: the arrival counters are the scratch's first 272 32-bit words, whatever the
 *     call's sizes; the call's per-workgroup partial sums follow them;
 *   - the caller zero-fills the buffer once, before its first use.  Every call returns the
 *     counters to zero and overwrites the partials it reads; the partials are NOT left zero
 *     (nothing reads them before they are rewritten);
 *   - so any buffer of at least the call's *_scratch_floats() size serves any number of calls
 *     of any of these entry points, in any order, on one stream -- e.g. one buffer of the
 *     largest size for all of them.  Calls that may run concurrently (other streams, parallel
 *     graph branches) need buffers of their own.
 * Scratch floats needed by gsr_track_transform_bwd(_adam) (n = P) and
 * gsr_track_l1_fwd(_bwd) (n = H*W): */
int gsr_track_scratch_floats(int n);

/* cam_q: the frame's unnormalised (w,x,y,z) quaternion, element k at cam_q[k * q_stride]
 *        (params["cam_unnorm_rots"][..., t] is a strided view); cam_t likewise (3 values).
 * unnorm_rot [P,4], logit_opac [P,1], log_scales [P,S] (S = 1 isotropic -> tiled to 3, or 3).
 * w2c [4,4] row-major: curr_data["w2c"] used for the depth colours.
 * Outputs [P,3] means_cam, [P,4] rotations (normalised, rendervar form), [P,3] depth_colors,
 *         [P,1] opacities, [P,3] scales. */
int gsr_track_transform_fwd(int P, const float* means_world, const float* unnorm_rot, const float* logit_opac,
                            const float* log_scales, int scale_cols, const float* cam_q, const float* cam_t,
                            int q_stride, const float* w2c, float* means_cam, float* rotations, float* depth_colors,
                            float* opacities, float* scales, void* stream);

/* dL_dmeans_cam [P,3] (sum over both renders), dL_drot [P,4] (may be NULL), dL_ddepth_colors [P,3]
 * (may be NULL).  Writes dL/dcam_q (4 values, stride q_stride) and dL/dcam_t (3 values, stride
 * q_stride); scratch: gsr_track_scratch_floats(P) floats. */
int gsr_track_transform_bwd(int P, const float* means_world, const float* unnorm_rot, int scale_cols,
                            const float* cam_q, const float* means_cam, const float* w2c,
                            const float* dL_dmeans_cam, const float* dL_drot, const float* dL_ddepth_colors,
                            float* dL_dcam_q, float* dL_dcam_t, int q_stride, float* scratch, void* stream);

/* gsr_track_transform_bwd with the optimizer step fused in:
 * instead of writing the pose gradient, applies torch.optim.Adam (no weight
 * decay, no amsgrad; the tracking optimizer of scripts/splatam.py) to the
 * frame's pose column in place: cam_q (4 values) / cam_t (3 values) at stride
 * q_stride.  Hyperparameters are doubles (torch's are python floats: 1 - beta2
 * rounded from a float beta2 would be 1.3e-5 off).  adam_state: device, 15 floats [m_q 4, v_q 4, m_t 3, v_t 3, step],
 * zero-initialised by the caller per frame (SplaTAM re-creates the optimizer per
 * frame). */
/* Optional per-iteration bookkeeping of the fused pose optimizer (may be NULL):
 *   status / capacity: the static-mode status row of this iteration's forward and its binning
 *       capacity; when the row shows an overflow ([0] > capacity, [2] > [3], or [1] != 0) the
 *       Adam step is skipped -- pose and optimizer state stay as they were (the outputs of an
 *       overflowing forward are invalid);
 *   loss / best: scripts/splatam.py:726-731 best-candidate selection: after the step, if
 *       *loss < best[0] then best[0] = *loss, best[1..4] = the updated quaternion and
 *       best[5..7] = the updated translation (a NaN loss never replaces the candidate).  The
 *       caller starts a frame with best[0] = 1e20 and writes best[1..7] back after its last
 *       iteration (:760-763). */
typedef struct gsr_pose_track {
    const unsigned* status;
    unsigned capacity;
    const float* loss;
    float* best;
} gsr_pose_track;

int gsr_track_transform_bwd_adam(int P, const float* means_world, const float* unnorm_rot, int scale_cols,
                                 float* cam_q, float* cam_t, int q_stride, const float* means_cam,
                                 const float* w2c, const float* dL_dmeans_cam, const float* dL_drot,
                                 const float* dL_ddepth_colors, double lr_q, double lr_t, double beta1,
                                 double beta2, double eps, float* adam_state, float* scratch,
                                 const gsr_pose_track* track, void* stream);

/* im [3,H,W], depth_sil [3,H,W] (depth, silhouette, depth^2), gt_im [3,H,W], gt_depth [1,H,W].
 * loss: 1 float (device).  scratch: gsr_track_scratch_floats(H*W) floats. */
int gsr_track_l1_fwd(int H, int W, const float* im, const float* depth_sil, const float* gt_im,
                     const float* gt_depth, float sil_thres, float w_im, float w_depth, float* loss, float* scratch,
                     void* stream);

/* gsr_track_l1_fwd and gsr_track_l1_bwd in one pass (one launch): dL_dloss is
 * read when the kernel runs, so the caller's loss seed must already hold its
 * value (a static seed, e.g. the tracker's ones). */
int gsr_track_l1_fwd_bwd(int H, int W, const float* im, const float* depth_sil, const float* gt_im,
                         const float* gt_depth, float sil_thres, float w_im, float w_depth, const float* dL_dloss,
                         float* loss, float* dL_dim, float* dL_ddepth_sil, float* scratch, void* stream);

/* The loss's two weighted terms -- the `_terms` sibling of every tracking forward that writes `loss`
 * (gsr_track_l1_fwd, gsr_track_l1_fwd_bwd, gsr_track_forward_dual_static, ..._static_xf,
 * gsr_track_forward_backward_dual_static_xf): the same call with one more output, `terms` (device, 2 floats,
 * 4-byte aligned, not NULL), placed after `loss`:
 *     terms[0] = w_im * sum(mask * |gt_im - im|),  terms[1] = w_depth * sum(mask * |gt_depth - depth|)
 * -- get_loss's weighted losses['im'] and losses['depth'] (scripts/splatam.py:262-296, :345-347); the second
 * is what use_depth_loss_thres compares with depth_loss_thres (:748).  They are written by the thread that
 * writes the loss, from the same two sums, with plain stores: no further reduction or atomic, the reduction
 * scratch contract above unchanged.  loss keeps its own expression (w_im * s0 + w_depth * s1, which the
 * compiler may contract), so terms[0] + terms[1] may differ from it in the last bit; every other output is
 * bitwise that of the sibling without terms.  Wherever the loss is invalid (a static forward that overflowed)
 * so are the terms.  A NULL or misaligned `terms` is GSR_ERR_INVALID_ARG, reported before the sibling's own
 * checks, which follow unchanged (under the sibling's name in gsr_last_error). */
int gsr_track_l1_fwd_terms(int H, int W, const float* im, const float* depth_sil, const float* gt_im,
                           const float* gt_depth, float sil_thres, float w_im, float w_depth, float* loss,
                           float* terms, float* scratch, void* stream);
int gsr_track_l1_fwd_bwd_terms(int H, int W, const float* im, const float* depth_sil, const float* gt_im,
                               const float* gt_depth, float sil_thres, float w_im, float w_depth,
                               const float* dL_dloss, float* loss, float* terms, float* dL_dim, float* dL_ddepth_sil,
                               float* scratch, void* stream);

/* dL_dloss: 1 float (device).  Writes dL_dim [3,H,W] and dL_ddepth_sil [3,H,W]. */
int gsr_track_l1_bwd(int H, int W, const float* im, const float* depth_sil, const float* gt_im,
                     const float* gt_depth, float sil_thres, float w_im, float w_depth, const float* dL_dloss,
                     float* dL_dim, float* dL_ddepth_sil, void* stream);

/* gsr_forward_dual_static with the tracking L1 loss (gsr_track_l1_fwd_bwd
 * semantics) formed in the render's per-pixel epilogue: the loss (1 float) and
 * its gradient images dL_dim [3,H,W] / dL_ddepth_sil [3,H,W] are written without
 * reading the rendered images back; dL_dloss (device scalar, the caller's static
 * loss seed) is read when the kernel runs.  scratch:
 * gsr_track_forward_scratch_floats(W, H) floats (the reduction scratch contract above:
 * zero-filled before first use, counters left zero).  The loss is valid iff the status
 * reports no overflow. */
int gsr_track_forward_scratch_floats(int image_width, int image_height);
int gsr_track_forward_dual_static(const gsr_settings* settings, const gsr_gaussians* gaussians, const float* colors2,
                                  int capacity, unsigned* status, float* out_color, float* out_color2,
                                  float* out_depth, int* radii, const float* gt_im, const float* gt_depth,
                                  float sil_thres, float w_im, float w_depth, const float* dL_dloss, float* loss,
                                  float* dL_dim, float* dL_ddepth_sil, float* scratch, gsr_alloc_fn alloc,
                                  void* alloc_ctx, void* stream);
/* ... with the loss's two terms (gsr_track_l1_fwd_terms above); an empty map (P == 0) writes them as zero. */
int gsr_track_forward_dual_static_terms(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                        const float* colors2, int capacity, unsigned* status, float* out_color,
                                        float* out_color2, float* out_depth, int* radii, const float* gt_im,
                                        const float* gt_depth, float sil_thres, float w_im, float w_depth,
                                        const float* dL_dloss, float* loss, float* terms, float* dL_dim,
                                        float* dL_ddepth_sil, float* scratch, gsr_alloc_fn alloc, void* alloc_ctx,
                                        void* stream);

/* gsr_track_transform_fwd fused into gsr_track_forward_dual_static (SURVEY.md 8(f) row 3:
 * "transform-to-frame plus the [z,1,z^2] colours fused into preprocess"): the rasterizer's
 * preprocess forms each Gaussian's camera-frame rendervars from the world-frame map and the
 * frame's pose itself, so the transform is not a launch of its own and its outputs are not read
 * back.  Same results, bit for bit, as gsr_track_transform_fwd(xform -> gaussians->means3D,
 * ->rotations, colors2, ->opacities, ->scales) followed by gsr_track_forward_dual_static with
 * those arrays: here they are OUTPUTS (written by the forward, device [P,3] / [P,4] / [P,3] /
 * [P,1] / [P,3]) for the backward (gsr_track_backward_dual), unless store_rendervars is 0: then
 * nothing is written to them (storing them cost preprocess ~6 us at 300 k Gaussians) and the
 * backward recomputes the geometric ones from the world-frame map (its log_scales argument).  gaussians->colors_precomp: the
 * RGB colours [P,3] (input); shs and cov3D_precomp must be NULL. */
typedef struct gsr_track_xform {
    const float* means_world;  /* [P,3] */
    const float* unnorm_rot;   /* [P,4] */
    const float* logit_opac;   /* [P,1] */
    const float* log_scales;   /* [P,scale_cols] */
    int scale_cols;            /* 1 (isotropic, tiled to 3) or 3 */
    const float* cam_q;        /* the frame's quaternion, element k at cam_q[k * q_stride] */
    const float* cam_t;        /* the frame's translation, likewise */
    int q_stride;
    const float* w2c;          /* [4,4] row-major: depth colours */
    int store_rendervars;      /* 1: write the rendervars (outputs below); 0: do not -- the
                                  backward then recomputes them (gsr_track_backward_dual log_scales) */
    const uint8_t* alive;      /* (ABI 7) [P] or NULL: alive[i] == 0 culls Gaussian i like one behind the
                                  camera (radius 0, no instances, zero gradients) -- a capacity-padded map's
                                  free and pruned slots (splatam_amd.sequence) */
} gsr_track_xform;

int gsr_track_forward_dual_static_xf(const gsr_settings* settings, const gsr_gaussians* gaussians, float* colors2,
                                     const gsr_track_xform* xform, int capacity, unsigned* status, float* out_color,
                                     float* out_color2, float* out_depth, int* radii, const float* gt_im,
                                     const float* gt_depth, float sil_thres, float w_im, float w_depth,
                                     const float* dL_dloss, float* loss, float* dL_dim, float* dL_ddepth_sil,
                                     float* scratch, gsr_alloc_fn alloc, void* alloc_ctx, void* stream);
int gsr_track_forward_dual_static_xf_terms(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                           float* colors2, const gsr_track_xform* xform, int capacity,
                                           unsigned* status, float* out_color, float* out_color2, float* out_depth,
                                           int* radii, const float* gt_im, const float* gt_depth, float sil_thres,
                                           float w_im, float w_depth, const float* dL_dloss, float* loss,
                                           float* terms, float* dL_dim, float* dL_ddepth_sil, float* scratch,
                                           gsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* Tracking backward with the pose chain fused into the rasterizer's per-Gaussian
 * backward: gsr_backward_dual's render backward (depth channel of the second
 * image, no opacity / colour sums), then one per-Gaussian kernel whose
 * dL/dmeans_cam, dL/d[z,1,z^2] and (anisotropic) dL/drotation feed the 16 pose
 * sums of gsr_track_transform_bwd directly -- no per-Gaussian gradient reaches
 * memory.  The last workgroup applies the pose chain and, with adam_state, the
 * Adam step in place (gsr_track_transform_bwd_adam semantics); without it the
 * pose gradient goes to dL_dcam_q / dL_dcam_t (stride q_stride).  settings,
 * gaussians (camera-frame rendervars), radii, colors2 ([z,1,z^2]) and the buffers
 * are those of the gsr_forward_dual(_static) call; means_world / unnorm_rot /
 * scale_cols / cam_q / cam_t / w2c those of gsr_track_transform_fwd.  scratch:
 * gsr_track_backward_scratch_floats(P) floats (the reduction scratch contract above:
 * zero-filled before first use, counters left zero).  The Adam step is skipped when the forward's own device
 * counters show an overflow of num_rendered (its capacity); `track` (may be
 * NULL) adds the best-candidate selection (its status / capacity are not used).
 * log_scales [P, scale_cols] (may be NULL): recompute each Gaussian's camera-frame mean, rotation
 * and scale from means_world / unnorm_rot / log_scales and the frame's (pre-step) pose instead of
 * reading gaussians->means3D / rotations / scales -- for a forward that did not store them
 * (gsr_track_forward_dual_static_xf with store_rendervars = 0); bitwise the same values. */
int gsr_track_backward_scratch_floats(int P);
int gsr_track_backward_dual(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                            const float* colors2, const float* dL_dout_color, const float* dL_dout_color2,
                            int num_rendered, const void* geom_buffer, const void* binning_buffer,
                            const void* image_buffer, const float* means_world, const float* unnorm_rot,
                            int scale_cols, float* cam_q, float* cam_t, int q_stride, const float* w2c, double lr_q,
                            double lr_t, double beta1, double beta2, double eps, float* adam_state,
                            float* dL_dcam_q, float* dL_dcam_t, float* scratch, const gsr_pose_track* track,
                            const float* log_scales, gsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* The tracking iteration's render forward and render backward in ONE launch (render_track_kernel) --
 * what scripts/splatam.py:255-296 (get_loss(tracking=True)) + :722 (loss.backward()) run as
 * CudaRasterizer::Rasterizer::forward (rasterizer_impl.cu:198-339) and ::backward (:343-434) per
 * Renderer call:
 * gsr_track_forward_dual_static_xf's forward + L1 loss, then in the same workgroup the back-to-front
 * walk of gsr_track_backward_dual's render backward -- SplaTAM's tracking loss gradient is per pixel
 * (dL/dloss is the static seed dL_dloss), so a tile's backward needs nothing from other tiles and runs
 * from the pixel state still in registers.  inst_records: gsr_track_records_floats(capacity) floats
 * (device), receiving the per-instance sums gsr_track_backward_dual_records reads; they equal, bit for
 * bit, what gsr_track_backward_dual's render backward forms.  The gradient images are not formed.
 * out_color, out_color2 and out_depth all NULL: the rendered images are not stored either (the loss and
 * the backward consume them in registers; nor are the image buffer's final_T / n_contrib, so a render
 * backward from another loss seed cannot follow such a call). */
int gsr_track_records_floats(int capacity);

int gsr_track_forward_backward_dual_static_xf(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                              float* colors2, const gsr_track_xform* xform, int capacity,
                                              unsigned* status, float* out_color, float* out_color2,
                                              float* out_depth, int* radii, const float* gt_im,
                                              const float* gt_depth, float sil_thres, float w_im, float w_depth,
                                              const float* dL_dloss, float* loss, float* scratch,
                                              float* inst_records, gsr_alloc_fn alloc, void* alloc_ctx,
                                              void* stream);
int gsr_track_forward_backward_dual_static_xf_terms(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                                    float* colors2, const gsr_track_xform* xform, int capacity,
                                                    unsigned* status, float* out_color, float* out_color2,
                                                    float* out_depth, int* radii, const float* gt_im,
                                                    const float* gt_depth, float sil_thres, float w_im,
                                                    float w_depth, const float* dL_dloss, float* loss, float* terms,
                                                    float* scratch, float* inst_records, gsr_alloc_fn alloc,
                                                    void* alloc_ctx, void* stream);
/* gsr_track_backward_dual after gsr_track_forward_backward_dual_static_xf: only the pose-fused
 * per-Gaussian backward (the render backward's records come from inst_records). */
int gsr_track_backward_dual_records(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                                    const float* colors2, int num_rendered, const void* geom_buffer,
                                    const void* binning_buffer, const void* image_buffer, const float* means_world,
                                    const float* unnorm_rot, int scale_cols, float* cam_q, float* cam_t, int q_stride,
                                    const float* w2c, double lr_q, double lr_t, double beta1, double beta2,
                                    double eps, float* adam_state, float* dL_dcam_q, float* dL_dcam_t,
                                    float* scratch, const gsr_pose_track* track, const float* log_scales,
                                    const float* inst_records, gsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* ------------------------------------------------------------------ mapping --
 * get_loss(mapping=True, do_ba=False) (scripts/splatam.py:220-353) with the
 * Replica mapping config (configs/replica/splatam.py:82-103: use_l1,
 * use_sil_for_loss=False, ignore_outlier_depth_loss=False, weights im 0.5 /
 * depth 1.0), and the mapping optimizer (splatam.py:166-172).  Forward of the
 * transform is gsr_track_transform_fwd (identical outputs). */

/* Scratch floats of gsr_map_loss_fwd (the reduction scratch contract at
 * gsr_track_scratch_floats: zero-filled before first use, counters left zero, shareable
 * with the tracking entry points) and the per-call state gsr_map_loss_fwd hands to
 * gsr_map_loss_bwd. */
int gsr_map_loss_scratch_floats(int H, int W);
int gsr_map_loss_state_floats(int H, int W);

/* loss = w_im * (0.8 * mean|im - gt_im| + 0.2 * (1 - calc_ssim(im, gt_im)))
 *      + w_depth * mean over mask of |gt_depth - depth|,
 * mask = (gt_depth > 0) & !isnan(depth) & !isnan(depth_sq - depth^2)
 * (gs_helpers.py:18-19 l1_loss_v1, slam_external.py:66-97 calc_ssim with an
 * 11x11 sigma-1.5 window and zero padding).  im/gt_im/depth_sil [3,H,W],
 * gt_depth [1,H,W]; loss: 1 float (device); state: gsr_map_loss_state_floats. */
int gsr_map_loss_fwd(int H, int W, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                     float w_im, float w_depth, float* loss, float* state, float* scratch, void* stream);

/* Gradient of the loss above w.r.t. im [3,H,W] and depth_sil [3,H,W] (channels
 * 1, 2 written as zero), given dL_dloss (1 float, device) and the forward's state. */
int gsr_map_loss_bwd(int H, int W, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                     float w_im, float w_depth, const float* dL_dloss, const float* state, float* dL_dim,
                     float* dL_ddepth_sil, void* stream);

/* Backward of transform_to_frame(gaussians_grad=True, camera_grad=False) + the
 * rendervar builders: from the gradients of (means_cam, rotations, depth
 * colours, opacities, scales) [any but dL_dmeans_cam may be NULL] to the
 * gradients of means3D [P,3], unnorm_rotations [P,4], logit_opacities [P,1] and
 * log_scales [P,scale_cols] (outputs other than dL_dmeans may be NULL). */
int gsr_map_transform_bwd(int P, const float* unnorm_rot, const float* logit_opac, const float* log_scales,
                          int scale_cols, const float* cam_q, int q_stride, const float* means_cam, const float* w2c,
                          const float* dL_dmeans_cam, const float* dL_drot, const float* dL_ddepth_colors,
                          const float* dL_dopac, const float* dL_dscales, float* dL_dmeans, float* dL_dunnorm_rot,
                          float* dL_dlogit_opac, float* dL_dlog_scales, void* stream);

/* torch.optim.Adam state of the mapping optimizer for the five Gaussian
 * parameter tensors [means3D, unnorm_rotations, logit_opacities, log_scales,
 * colours (rgb_colors [P,3] or shs [P,M,3])]: exp_avg / exp_avg_sq of each
 * tensor's shape, per-tensor lr, and the optimizer step (>= 1, i.e. already
 * incremented) this update uses. */
typedef struct gsr_map_adam {
    float* exp_avg[5];
    float* exp_avg_sq[5];
    double lr[5];
    int step;
    double beta1, beta2, eps;
    /* optional: the counters of this iteration's static-mode forward and its binning capacity;
     * an overflow there (see gsr_pose_track) skips the step -- parameters and state unchanged.
     * Point it at the forward's own counters (geom_buffer + gsr_geom_counters_offset(P)); a
     * sticky status row would skip every later step once any earlier call overflowed.
     * gsr_backward_dual_sh_adam ignores it and guards on its own forward's counters. */
    const unsigned* status;
    unsigned capacity;
    /* optional device word, zero at the start of a frame (torch.optim.Adam's fresh state): a step
     * skipped because its forward overflowed sets it, and every later fused step (colour group,
     * transform backward) is skipped while it is set -- so the device never applies a step whose
     * bias corrections assume a step count the skipped one did not reach.  The caller re-runs the
     * frame from fresh state (splatam_amd.glue.MapAdam.reset) after reading it as non-zero. */
    unsigned* halted;
} gsr_map_adam;

/* gsr_backward_dual with the mapping optimizer's colour group (sh_adam->exp_avg[4] / exp_avg_sq[4] /
 * lr[4], step, betas, eps) applied to the SH coefficients gaussians->shs in place inside the
 * SH backward stage, instead of writing grads->dsh (which may be NULL) for
 * gsr_map_transform_bwd_adam to step: the 192-B-per-Gaussian gradient never makes the HBM round
 * trip.  Same element update (bitwise) as gsr_map_transform_bwd_adam's; call that one afterwards
 * with dL_dcolors = NULL.  Needs staged SH colours (M == (sh_degree+1)^2). */
int gsr_backward_dual_sh_adam(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                              const float* colors2, const float* dL_dout_color, const float* dL_dout_color2,
                              int num_rendered, const void* geom_buffer, const void* binning_buffer,
                              const void* image_buffer, const gsr_grads* grads, float* dcolors2, int dl2_channels,
                              const gsr_map_adam* sh_adam, gsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* gsr_map_transform_bwd with the optimizer step fused in: the parameters are
 * updated in place, no gradient is written.  dL_dcolors (the rasterizer's
 * gradient of the colour parameters, [P, color_cols]) steps `colors`; NULL
 * leaves them (and their state) untouched. */
int gsr_map_transform_bwd_adam(int P, float* means_world, float* unnorm_rot, float* logit_opac, float* log_scales,
                               int scale_cols, float* colors, int color_cols, const float* cam_q, int q_stride,
                               const float* means_cam, const float* w2c, const float* dL_dmeans_cam,
                               const float* dL_drot, const float* dL_ddepth_colors, const float* dL_dopac,
                               const float* dL_dscales, const float* dL_dcolors, const gsr_map_adam* adam,
                               void* stream);

/* SplaTAM's pruning inside a captured mapping frame (prune_gaussians, utils/slam_external.py:167-188, with
 * scripts/splatam.py:876-878 calling it between loss.backward() and optimizer.step()) without changing P:
 *   gsr_map_prune: alive[i] (uint8, 1 = kept) is cleared where the reference's remove_points would drop
 *     Gaussian i: sigmoid(logit_opac[i]) < opac_thr, or (remove_big) max_j exp(log_scales[i, j]) > big_thr
 *     (big_thr = 0.1 * scene_radius as the caller's float32 tensor holds it); each value formed as torch
 *     forms it (1 / (1 + exp(-x)), exp) so the decision is the reference's.  Already cleared entries stay.
 *   gsr_forward_dual_static_alive: gsr_forward_dual_static (include/gsr.h) where a Gaussian with
 *     alive[i] == 0 is culled like one behind the camera (radius 0, no instances, zero gradients); the
 *     others' images, binning order, gradients and optimizer steps are exactly those of the compacted
 *     set (the per-tile (depth, id) order of the survivors does not depend on the removed ids). */
int gsr_map_prune(int P, const float* logit_opac, const float* log_scales, int scale_cols, float opac_thr,
                  float big_thr, int remove_big, unsigned char* alive, void* stream);
int gsr_forward_dual_static_alive(const gsr_settings* settings, const gsr_gaussians* gaussians, const float* colors2,
                                  int capacity, unsigned* status, float* out_color, float* out_color2,
                                  float* out_depth, int* radii, const unsigned char* alive, gsr_alloc_fn alloc,
                                  void* alloc_ctx, void* stream);
/* The single-image counterpart: gsr_forward_static (include/gsr.h) with the same mask and the same rule --
 * alive[i] == 0 culls Gaussian i (radius 0, no instances, zero gradients from gsr_backward), the others'
 * image, depth, radii, status counters and gradients are exactly those of gsr_forward_static on the compacted
 * set.  alive == NULL with P > 0 is GSR_ERR_INVALID_ARG ("alive mask required"), after the static-mode check.
 * The view scorer of a capacity-padded map renders through it (splatam_amd.fisher.SequenceFisher). */
int gsr_forward_static_alive(const gsr_settings* settings, const gsr_gaussians* gaussians, int capacity,
                             unsigned* status, float* out_color, float* out_depth, int* radii,
                             const unsigned char* alive, gsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* The mapping iteration's transform fused into its forward (as
 * gsr_track_forward_dual_static_xf for tracking): gsr_track_transform_fwd(xform -> gaussians->means3D,
 * ->rotations, colors2, ->opacities, ->scales) followed by gsr_forward_dual_static_alive(..., xform->alive)
 * with those arrays, in one pass of preprocess -- the same results bit for bit, without the transform's
 * launch.  The five arrays are OUTPUTS (xform->store_rendervars must be 1: the mapping backward reads
 * them); gaussians->colors_precomp the RGB colours [P,3] (input); shs and cov3D_precomp must be NULL
 * (SH colours are evaluated ahead of preprocess, from the camera-frame means). */
int gsr_forward_dual_static_xf(const gsr_settings* settings, const gsr_gaussians* gaussians, float* colors2,
                               const gsr_track_xform* xform, int capacity, unsigned* status, float* out_color,
                               float* out_color2, float* out_depth, int* radii, gsr_alloc_fn alloc, void* alloc_ctx,
                               void* stream);

/* Gaussian-splatting densification's per-iteration statistics (accumulate_mean2d_gradient,
 * utils/slam_external.py:100-104, with scripts/splatam.py:349) in one launch, one lane per Gaussian, without
 * the reference's boolean index and its host read.  For radii[i] > 0:
 *     accum[i] += sqrtf(gx^2 + gy^2)   with (gx, gy) = dmeans2D[i, 0:2] (dmeans2D is [P,3]),
 *     denom[i] += 1,
 *     max_2D_radius[i] = max(max_2D_radius[i], radii[i]);
 * the other rows are not written.  The norm's operands are scaled by an exact power of two, so it stays
 * within 2 ulp for denormal gradients too (the plain expression's bits wherever that neither underflows nor
 * overflows).  dmeans2D is the RGB render's own gradient: gsr_backward_dual_m2d's dmeans2D_color1. */
int gsr_accumulate_mean2d(int P, const int* radii, const float* dmeans2D, float* accum, float* denom,
                          float* max_2D_radius, void* stream);

/* torch.optim.Adam (foreach implementation, no weight decay / amsgrad /
 * maximize) over up to 16 float32 tensors in one launch; every tensor shares
 * `step` (>= 1, already incremented) and has its own lr. */
typedef struct gsr_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long n;
    double lr;
} gsr_adam_tensor;
int gsr_adam_step(int n_tensors, const gsr_adam_tensor* tensors, int step, double beta1, double beta2, double eps,
                  void* stream);

/* Fisher / EIG view scoring glue (scripts/ros_handler.py:847-902).
 * gsr_points_to_camera: pts [P,3] = the Gaussians' means [P,3] in a candidate camera frame,
 *     (rel_w2c @ [means, 1]^T)^T[:, :3] (ros_handler.py:863-866); w2c [4,4] row-major (device),
 *     each coordinate summed left to right without contraction.
 * gsr_fisher_accumulate: H [P,4] (16-byte aligned) += [dmeans3D [P,3], dopacity [P,1]] * (*weight)
 *     (weight: device scalar), product and sum each rounded -- torch's
 *     H.add_(torch.cat([pts.grad, opacities.grad], 1) * w) in one launch (the visited-pose sum of
 *     compute_H_visited_inv, ros_handler.py:807-829). */
int gsr_points_to_camera(int P, const float* means, const float* w2c, float* pts, void* stream);
int gsr_fisher_accumulate(int P, const float* dmeans3D, const float* dopacity, const float* weight, float* H,
                          void* stream);

/* compute_eig_score (scripts/ros_handler.py:832-836), torch.sum(cur_H * H_train_inv), of one pose in one
 * launch, from the two gradients the power-2 backward left:
 *     *out = sum over the rows i with alive[i] != 0 (every row when alive == NULL) and c = 0..3 of
 *            (double) fl32(H[i,c] * H_inv[i,c]),  H[i,0..2] = dmeans3D[i,0..2], H[i,3] = dopacity[i].
 * dmeans3D [P,3], dopacity [P,1], H_inv [P,4] (16-byte aligned), alive uint8 [P] or NULL, out: one double
 * (device, 8-byte aligned).  Each product is rounded to float32 once, as the reference's elementwise product
 * is, and is not contracted into the sum; the sum is accumulated in float64.  A dead row is selected out, not
 * multiplied by zero: its H and H_inv may hold anything (NaN included) and do not reach the result -- the
 * rows of a capacity-padded map under its alive mask (splatam_amd.sequence).
 *   Order: at most 256 workgroups of 256 threads stride over the rows; a thread adds its rows in ascending
 * order (the four columns in order), a workgroup adds its threads by a lane tree and then its four waves,
 * and the last workgroup to arrive adds the workgroups' partials by the same tree over the workgroup index.
 * No float atomic: the same inputs (and the same P) give the same bits on every call.  The float64 sum of
 * n = 4 P non-negative terms in any order is within (n - 1) 2^-53 of the exact sum, relative.
 *   P == 0: *out = 0.0, no other pointer is read.  Everything is enqueued on `stream` (one launch) and
 * nothing waits on the host, so the call can be captured in a graph.
 * workspace: gsr_fisher_score_workspace_bytes() bytes of its own (a constant: the grid is bounded; not the
 * reduction scratch above), 16-byte aligned, zero-filled once before its first use: its arrival counter
 * (word 0, whatever P) returns to zero and the partials are written before they are read, so one buffer
 * serves any number of calls of any P on one stream; calls that may run concurrently need their own.
 * Refused with GSR_ERR_INVALID_ARG, nothing enqueued: P < 0, a NULL or misaligned out, and with P > 0 a NULL
 * dmeans3D, dopacity, H_inv or workspace, or a misaligned H_inv or workspace. */
size_t gsr_fisher_score_workspace_bytes(void);
int gsr_fisher_score(int P, const float* dmeans3D, const float* dopacity, const float* H_inv,
                     const unsigned char* alive, void* workspace, double* out, void* stream);

/* The silhouette half of the fork's mixed view gain (scripts/ros_handler.py:251-359, send_gains:
 * g_sil = (sil < 0.5).sum() / (W H) of a second, depth/silhouette render per candidate pose,
 * get_renders :955-985) without that render: *count (device, one unsigned) = the number of pixels
 * inside the image whose silhouette is < sil_thres (strict), from the buffers a finished forward
 * left -- geom_buffer, binning_buffer, image_buffer and num_rendered as gsr_backward takes them,
 * after gsr_forward and after gsr_forward_static (num_rendered = the capacity it returned) alike;
 * P, the image size and bg as in that forward's call (of `settings` only image_width,
 * image_height and bg are read; bg on the device, when the kernel runs).
 *   The silhouette of a pixel is the forward's image of a colour channel whose per-Gaussian value
 * is 1 with background bg[1] (SplaTAM's [z, 1, z^2] render, channel 1), decision by decision: the
 * tile's sorted, block-masked list walked front to back, alpha = min(0.99, opacity * exp2(p2)),
 * pairs with p2 > 0 or alpha < 1/255 skipped, the walk ended at T (1 - alpha) < 1e-4, C += alpha T
 * (product and sum each rounded), the value C + T bg[1].  The count therefore equals the count
 * taken from that render.  With bg[1] >= 0 a pixel's walk ends as soon as C >= sil_thres (the
 * value cannot fall below it again); with bg[1] < 0 it ends where the forward's does.
 *   The entry point zeroes *count itself (a one-thread kernel with a plain store, ahead of the count
 * kernel on `stream`; no memset node), then one 256-thread workgroup per tile adds its pixels with
 * one integer atomic: the result does not depend on the arrival order.  Everything is enqueued on
 * `stream` and nothing waits on the host, so the call can be captured in a graph.  After a
 * static-capacity forward that overflowed (num_rendered > capacity or a tile list longer than the
 * per-tile sort handles) the lists are not valid: the kernel does not walk them and *count is
 * unspecified (it stays zero); the forward's status row reports the overflow.  P == 0: every
 * silhouette is 0 (the forward writes zero images), *count = W H if 0 < sil_thres else 0, and the
 * buffers are not read.  Returns GSR_OK or a negative error code (gsr_last_error names the call). */
int gsr_silhouette_count(const gsr_settings* settings, int P, int num_rendered, const void* geom_buffer,
                         const void* binning_buffer, const void* image_buffer, float sil_thres, unsigned* count,
                         void* stream);

/* ------------------------------------------------------- keyframe selection --
 * SplaTAM's overlap keyframe selection (utils/keyframe_selection.py, scripts/splatam.py:820-837)
 * without a host read: everything is enqueued on `stream` (three launches), every input but the
 * sizes is read on the device when the kernels run, so the call can be captured in a graph and
 * replayed after the depth, the poses and the random words changed in place.
 *
 * Inputs: depth [H,W] (H <= 4096); fx, fy, cx, cy; w2c: the current frame's world-to-camera matrix
 * (16 floats, row-major); kf_w2c [n_kf,16]: the keyframes' est_w2c; kf_time [n_kf]: their time
 * indices; u_pix [S], perm_key [n_kf - 1] (or longer), u_draw [n_draws]: random 32-bit words;
 * cur_row: the bank row of the current frame (>= n_kf; keyframe i is bank row i); k_select <= 1022.
 *   1. sample: n_valid = #(depth > 0); sample j takes the valid pixel of row-major rank
 *      r_j = (u_pix[j] * n_valid) >> 32 (64-bit product) -- where the reference draws
 *      torch.randint(n_valid), whose bound only the device knows.  n_valid == 0: no points.
 *   2. back-project: x = (col - cx) / fx * z, y = (row - cy) / fy * z; world point
 *      w_a = R[0][a] x + R[1][a] y + R[2][a] z + t'_a, t'_a = -(R[0][a] t_0 + R[1][a] t_1 + R[2][a] t_2):
 *      the rigid inverse of w2c in closed form (the reference: torch.inverse).  Every product and
 *      sum is rounded on its own, sums left to right.
 *   3. drop: every sample whose rank another sample drew too (the reference's unique(...,
 *      return_counts) drops all copies), and a sample with rint(1e4 w_a) == 0 for all three a.
 *      Deliberate difference: the reference also drops two DISTINCT pixels whose points share a
 *      1e-4 m cell; they are kept here.
 *   4. project into every candidate (keyframes 0 .. n_kf - 2): p = est_w2c[:3] . (w, 1) (left to
 *      right), zz = p.z + 1e-5, u = (fx p.x + cx p.z) / zz, v = (fy p.y + cy p.z) / zz; inside when
 *      20 < u < W - 20, 20 < v < H - 20 and zz > 0.
 *   5. eligible: overlap > 0.  The window is the first min(k_select, #eligible) eligible
 *      candidates in ascending (perm_key[i], i) order -- a uniformly random subset, the
 *      reference's np.random.permutation(...)[:k] -- then keyframe n_kf - 1 if n_kf > 0, then cur_row.
 *   6. draw i picks window[(u_draw[i] * n_window) >> 32].
 * Outputs: overlap [n_kf - 1] kept samples inside each candidate; n_points [1] samples kept by 3;
 * window [k_select + 2] bank rows (unused entries -1) and n_window [1]; draw_rows / draw_times
 * [n_draws] (int64, torch.index_select indices): the drawn bank row and its time index (time_idx
 * for cur_row); sampled_pixels [S] (may be NULL): each sample's pixel row * W + col (-1: none).
 * workspace: gsr_keyframe_workspace_bytes(H, S) bytes of its own (not the reduction scratch above),
 * 16-byte aligned, zero-filled once before its first use: its arrival counters (the first 16
 * words, whatever the sizes) return to zero and everything else is written before it is read, so
 * one buffer of the largest size serves any number of calls on one stream. */
size_t gsr_keyframe_workspace_bytes(int H, int S);
int gsr_keyframe_select(int H, int W, const float* depth, float fx, float fy, float cx, float cy, const float* w2c,
                        const float* kf_w2c, int n_kf, int k_select, int S, const unsigned* u_pix,
                        const unsigned* perm_key, int n_draws, const unsigned* u_draw, const long long* kf_time,
                        long long time_idx, int cur_row, void* workspace, int* overlap, int* n_points, int* window,
                        int* n_window, long long* draw_rows, long long* draw_times, int* sampled_pixels,
                        void* stream);

/* ------------------------------------------------------------- evaluation --
 * One frame of SplaTAM's eval() (utils/eval_helpers.py:466-512) without a host read: everything is
 * enqueued on `stream` (one launch, six with MS-SSIM), every input but the sizes and the three
 * scalars is read on the device when the kernels run, so the call can be captured in a graph and
 * replayed after the four images changed in place.
 *
 * Inputs: im, gt_im [3,H,W] (the rendered and the captured colour); depth_sil [3,H,W] (channel 0 the
 * rendered depth, channel 1 the silhouette); gt_depth [1,H,W].  With 0/1 float masks
 *     valid = gt_depth > 0, presence = silhouette > sil_thres (strict),
 *     m = valid * presence when use_sil_mask, else valid
 * (use_sil_mask: the reference's `mapping_iters == 0 and not add_new_gaussians`), and every product
 * below a float32 multiplication -- a NaN or inf pixel under a zero mask stays NaN, as in the reference:
 *     wi = im * m, wg = gt_im * m;
 *     mse_c  = sum over the H*W pixels of (wi_c - wg_c)^2, divided by H*W;
 *     psnr   = the mean over the three channels of 20 log10(1 / sqrt(mse_c));
 *     e      = depth * valid - gt_depth, times presence when use_sil_mask;
 *     depth_rmse = sum(sqrt(e^2) * valid) / n_valid;  depth_l1 = sum(|e| * valid) / n_valid;
 *     n_valid = sum(valid).
 * depth_rmse is the reference's formula (:500-502, :507-509): the square root is taken per pixel, before
 * the sum, so it is the same mean absolute error as depth_l1 (up to the underflow of e^2), not a root
 * mean square; the reference writes both files (rmse.txt, l1.txt), so both columns are kept.  Nothing is
 * special-cased: n_valid == 0 gives NaN (0 / 0) in both depth columns, mse_c == 0 gives psnr = inf.
 * row (8 floats, device): {psnr, ms_ssim, depth_rmse, depth_l1, n_valid, mse_r, mse_g, mse_b}.
 *
 * ms_ssim: pytorch_msssim's ms_ssim(wi, wg, data_range=1.0, size_average=True), the call of :484,
 * restated here from its published definition -- the package is not a dependency, and parity with it
 * is NOT pinned by any test of this repository:
 *   window: 11 taps, g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) normalised to sum 1, applied separably along H
 *     and then along W as a valid (unpadded) correlation G*: an [h,w] image gives [h - 10, w - 10].
 *   per level and channel, X / Y the two images: mu1 = G*X, mu2 = G*Y, s1 = G*(X X) - mu1^2,
 *     s2 = G*(Y Y) - mu2^2, s12 = G*(X Y) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2,
 *     cs_map = (2 s12 + C2) / (s1 + s2 + C2), ssim_map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map;
 *     cs, ssim = the means of the two maps over the valid output.
 *   five levels; after each of the first four X and Y become avg_pool2d(kernel 2, stride 2, padding =
 *     extent % 2 per axis, the zero pad counted in the divisor): an odd extent n pools the windows
 *     [-1,0], [1,2], ..., [n-2,n-1] (index -1 a zero), each sum divided by 4, and yields (n + 1) / 2.
 *   ms_ssim = the mean over the three channels of prod_l v_l^w_l, v_0..3 = relu(cs) of levels 0..3,
 *     v_4 = relu(ssim) of level 4, w = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333].
 *   The definition exists for min(H, W) > 160 only: with ms_ssim != 0 a smaller image is refused
 *   (GSR_ERR_INVALID_ARG, nothing is written); with ms_ssim == 0 the column is NaN and the pyramid is
 *   not run.
 * Precision: the per-pixel operations above are float32, as the reference's; the sums over the image and
 * the window's weighted sums are accumulated in float64 in a fixed order (no float atomics: the same
 * inputs give the same bits on every run) and rounded to float32 once, in the row; the pooled images are
 * stored as float32.
 * workspace: gsr_eval_workspace_bytes(H, W, ms_ssim) bytes of its own (not the reduction scratch above;
 * 0 for sizes gsr_eval_frame refuses), 16-byte aligned, zero-filled once before its first use: its two
 * arrival counters (in the first 16 words, whatever the sizes) return to zero and everything else is
 * written before it is read, so one buffer of the largest size serves any sequence of sizes on one stream. */
size_t gsr_eval_workspace_bytes(int H, int W, int ms_ssim);
int gsr_eval_frame(int H, int W, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                   float sil_thres, int use_sil_mask, int ms_ssim, void* workspace, float* row, void* stream);

/* ---------------------------------------------------------- densification --
 * SplaTAM's add_new_gaussians (scripts/splatam.py:384-426) on a capacity-padded map without a host
 * read: everything is enqueued on `stream` (six launches), every input but the
 * sizes and the scalar settings is read on the device when the kernels run, so the call can be
 * captured in a graph and replayed after the images, the pose and n_live changed in place.  The
 * image may have any resolution of its own (a downscaled densification frame with its intrinsics).
 *
 * Inputs: depth_sil [3,H,W] (the silhouette render: channel 0 the rendered depth rd, channel 1 the
 * silhouette sil); gt_im [3,H,W]; gt_depth [1,H,W] (gt); fx, fy, cx, cy; w2c: the frame's estimated
 * world-to-camera matrix (16 floats on the device, row-major); sil_thres; capacity.
 * In/out: means3D [cap+1,3], rgb_colors [cap+1,3], unnorm_rotations [cap+1,4], logit_opacities
 * [cap+1,1], log_scales [cap+1,1], alive uint8 [cap+1], n_live int64 [1], overflow (one byte, OR-ed).
 * Out: n_added int64 [1]; dest int32 [H*W] (may be NULL): the row each pixel wrote, -1 if none.
 * All arithmetic is float32 and every operation is rounded on its own (no contraction):
 *   1. valid = gt > 0; err = |gt - rd| * valid (a product with 0.0 / 1.0, so a NaN or an infinite
 *      |gt - rd| under valid == 0 is a NaN).
 *   2. med = the value torch.median returns over all H*W values of err: element (H*W - 1) / 2 of the
 *      ascending order (the lower median); NaN if any err is NaN.  Found by selection on err's bit
 *      patterns (non-negative floats order as unsigned integers) in three passes of 11, 11 and 10
 *      bits with integer histograms; nothing is sorted and no float is accumulated.
 *   3. thr = 50 * med; selected = ((sil < sil_thres) | ((rd > gt) & (err > thr))) & valid.  Comparisons
 *      with a NaN are false: a NaN med leaves the silhouette term alone, a NaN sil is not selected.
 *   4. a selected pixel's row is n_live + r, r its rank among the selected pixels in row-major
 *      order, n_live the value before the call.  Only rows in [0, capacity) are written; the sink row
 *      `capacity` and every row no selected pixel maps to are not touched.
 *   5. the row's values: x = (col - cx) / fx * z, y = (row - cy) / fy * z with z = gt; means3D the world
 *      point by the closed-form rigid inverse of w2c exactly as step 2 of gsr_keyframe_select states
 *      it (the same left-to-right sums); rgb_colors = gt_im[:, row, col]; unnorm_rotations =
 *      (1, 0, 0, 0); logit_opacities = 0; log_scales = logf(sqrtf(q * q)), q = z / f, where f is
 *      (fx + fy) / 2 formed in double from the two floats passed and rounded to float once; alive = 1.
 *      (logf is the device library's: log_scales alone is not pinned bitwise.)
 *   6. n_added = the number selected (whether or not their rows fit); n_live = min(n_live + n_added,
 *      capacity); overflow |= (n_live + n_added > capacity).
 * Returns GSR_ERR_INVALID_ARG and writes nothing for H or W <= 0, H * W >= 2^31, capacity < 0 or a
 * NULL pointer other than dest.
 * workspace: gsr_densify_workspace_bytes(H, W) bytes of its own (0 for sizes gsr_densify_frame
 * refuses), 16-byte aligned, zero-filled once before its first use: its four arrival counters (in the
 * first 16 words, whatever the sizes) return to zero and everything else is written before it is
 * read (the histograms by the call's first launch), so one buffer of the largest size serves any sequence of
 * sizes on one stream. */
size_t gsr_densify_workspace_bytes(int H, int W);
int gsr_densify_frame(int H, int W, const float* depth_sil, const float* gt_im, const float* gt_depth, float fx,
                      float fy, float cx, float cy, const float* w2c, float sil_thres, int capacity, float* means3D,
                      float* rgb_colors, float* unnorm_rotations, float* logit_opacities, float* log_scales,
                      unsigned char* alive, long long* n_live, unsigned char* overflow, long long* n_added, int* dest,
                      void* workspace, void* stream);

/* gsr_densify_frame with the realtime loop's threshold (add_new_gaussians of scripts/splatam_realtime.py:
 * 430-482, its median_thr and median_scale): the contract above word for word, the same six launches and
 * the same workspace, except step 3's thr:
 *   use_median_thr != 0 and med > median_thr (false for a NaN med):
 *                             thr = (float)((double)median_scale * (double)median_thr) -- the product the
 *                             reference forms from two Python floats before torch rounds it to float32;
 *   use_median_thr != 0 otherwise: thr = 50.f * med.  median_scale is NOT used here: the reference resets
 *                             its scale to 50 on this branch (:450-451), and that quirk is kept;
 *   use_median_thr == 0:      thr = median_scale * med, in float32.
 * use_median_thr is the reference's `median_thr is not None`.  gsr_densify_frame is this call with
 * (0, 0, 50.f).  The decision is made in the kernel that reads med (no launch of its own).  The three
 * arguments come last.  Errors name "densify_frame_capped". */
int gsr_densify_frame_capped(int H, int W, const float* depth_sil, const float* gt_im, const float* gt_depth,
                             float fx, float fy, float cx, float cy, const float* w2c, float sil_thres, int capacity,
                             float* means3D, float* rgb_colors, float* unnorm_rotations, float* logit_opacities,
                             float* log_scales, unsigned char* alive, long long* n_live, unsigned char* overflow,
                             long long* n_added, int* dest, void* workspace, void* stream, int use_median_thr,
                             float median_thr, float median_scale);

/* initialize_first_timestep's point cloud (scripts/splatam_realtime.py:229-237) on a capacity-padded map:
 * selected = gt > 0 for every pixel -- no silhouette render is read and no median is formed -- and then
 * steps 4-6 of gsr_densify_frame exactly (rows n_live + rank in row-major order, the same values, n_added,
 * n_live, overflow, dest), by the same two kernels: two launches.  w2c: the first frame's world-to-camera
 * matrix.  A map that starts empty passes n_live = 0 and an all-zero alive.
 * workspace: gsr_densify_workspace_bytes(H, W) bytes under the contract above; the call uses one of the
 * four arrival counters and leaves it zero, so one buffer serves any interleaving of the three entries on
 * one stream.  Refuses what gsr_densify_frame refuses (there is no depth_sil); errors name "init_frame". */
int gsr_init_frame(int H, int W, const float* gt_im, const float* gt_depth, float fx, float fy, float cx, float cy,
                   const float* w2c, int capacity, float* means3D, float* rgb_colors, float* unnorm_rotations,
                   float* logit_opacities, float* log_scales, unsigned char* alive, long long* n_live,
                   unsigned char* overflow, long long* n_added, int* dest, void* workspace, void* stream);

/* ------------------------------------------------------------------ resize --
 * A frame's copies at other resolutions, for a tracking resolution (the reference's tracking_image_height /
 * width, scripts/splatam.py:517-523, 588-607: "SplaTAM-S") and a densification resolution of their own: one
 * launch on `stream` for up to two outputs, nothing read back, no workspace; every input but the sizes is read
 * on the device when the kernel runs, so the call can be captured in a graph.  Any size ratio, up or down,
 * separately in x and y.
 *
 * Inputs: im [3,H,W], depth [1,H,W].  Output k (k = 0, 1): im_out_k [3,h_k,w_k], depth_out_k [1,h_k,w_k]; an
 * output whose two pointers are both NULL is skipped (its sizes are not read).  For output pixel (y, x):
 *   depth: nearest neighbour, the source pixel (floor(y H / h), floor(x W / w)) in integer arithmetic -- the
 *     rule of cv2.INTER_NEAREST and of torch's mode="nearest".  The value is copied: the same bits.
 *   colour: bilinear with half-pixel centres and edge clamp, the sample positions of cv2.INTER_LINEAR and of
 *     torch's F.interpolate(mode="bilinear", align_corners=False), no antialiasing.  Along x: the source
 *     coordinate is sx = max(0, (x + 0.5) W / w - 0.5), formed exactly from integers: num = (2 x + 1) W - w,
 *     den = 2 w; num <= 0: x0 = 0, tx = 0; else x0 = num / den (integer quotient), tx = (float)(num - x0 den)
 *     / (float)den -- two exact conversions (w <= 2^23) and one correctly rounded division, never a float32
 *     scale factor; x1 = min(x0 + 1, W - 1).  The same in y (y0, y1, ty).  Then, in float32, every operation
 *     rounded on its own (no contraction), lerp(a, b, t) = a when t == 0, else a + t * (b - a):
 *         top = lerp(im[c, y0, x0], im[c, y0, x1], tx);   bot = lerp(im[c, y1, x0], im[c, y1, x1], tx);
 *         out[c, y, x] = lerp(top, bot, ty)
 *     -- horizontally on the two rows, then vertically.  A tap of weight zero is not read into the result: a
 *     NaN or an infinity reaches exactly the outputs that one of its four taps enters with a non-zero weight,
 *     and nothing is masked.  h == H and w == W: every weight is zero and the output is the input's bits.
 * Difference from the reference, deliberate: its loader resizes the uint8 image (cv2's 11-bit fixed-point
 * weights, rounded to a byte) and divides by 255 afterwards; this call resizes the float image.  Parity with
 * cv2's uint8 path is NOT pinned by any test of this repository.
 * Returns GSR_ERR_INVALID_ARG and launches nothing for H, W < 1 or H * W >= 2^31; a NULL im or depth; an
 * output with exactly one of its two pointers NULL; a present output with h, w < 1, h * w >= 2^31, or
 * 2 w W or 2 h H >= 2^31 (the numerators are ints); both outputs absent.  Errors name "resize_frame". */
int gsr_resize_frame(int H, int W, const float* im, const float* depth, int h0, int w0, float* im_out0,
                     float* depth_out0, int h1, int w1, float* im_out1, float* depth_out1, void* stream);

/* ------------------------------------------------------------------ ingest --
 * A raw sensor frame into the float frame the sequence reads and, in the same launch, into its copies at up to
 * two other resolutions: what the reference's intake does op by op on arrival (scripts/ros_handler.py:402-411,
 * 434-435; datasets/gradslam_datasets/basedataset.py:250-257, 312-316).  One launch on `stream`, nothing read
 * back, no workspace; every input but the sizes and the scalars is read on the device when the kernel runs, so
 * the call can be captured in a graph.
 *
 * Inputs: rgb_hwc, the interleaved uint8 image [H,W,3], at ANY byte address; depth_u16, the uint16 depth image
 * [H,W] in sensor units, at any 2-byte address (a frame may be a slice of a larger capture buffer).  Outputs:
 * im [3,H,W], depth [1,H,W] (float32, 4-byte aligned; 16-byte aligned pointers with H W % 4 == 0 get vector
 * stores) and the small outputs k = 0, 1 as in gsr_resize_frame.  Three roundings are the whole contract:
 *   colour: im[c, y, x] = (float)rgb[y, x, c] / 255.0f -- ONE correctly rounded float32 division, not a
 *     multiply by a reciprocal.  The value depends on the byte alone (a 256-entry table states it).  torch's
 *     device-side `x / 255` multiplies by the rounded reciprocal and may differ from this by one ulp for some
 *     bytes; torch's CPU form (a true division) does not differ.
 *   depth: d = (float)((double)u / png_depth_scale) -- the float64 quotient of numpy's `arr / png_depth_scale`,
 *     rounded to float32 ONCE.  A correctly rounded float32 division (float)u / (float)scale gives the same bits
 *     whenever the scale is a float32 value (53 >= 2 * 24 + 2 bits: the second rounding is innocuous), so
 *     torch's CPU `/` agrees; a float32 multiply by the reciprocal -- torch's device-side `/ scale` -- does
 *     not: it differs for 249 of the 65,536 readings at scale 6553.5, 38,850 at 1000, 19,860 at 5000.
 *     use_max_depth != 0 and d >= max_depth: -1.0f is written (the reference's
 *     `depth[depth >= 9.5] = -1`, the threshold a parameter).  A zero reading stays 0.0f: invalid to every
 *     consumer (`gt > 0`), like -1.
 *   small outputs: output k is present when both of its pointers are non-NULL and holds EXACTLY THE BITS
 *     gsr_resize_frame produces from the full-size im / depth above: depth nearest, colour bilinear with the
 *     integer-derived taps and the lerp that skips a zero weight.  They are formed from the raw bytes, every tap
 *     converted on the fly -- im / depth are being written by the same launch and are never read -- and the bits
 *     are the same because the conversion is a pure function of the byte.
 * im / depth (both NULL) may be absent when only small frames are wanted; both small outputs may be absent too.
 * Returns GSR_ERR_INVALID_ARG and launches nothing for: every size and overflow condition gsr_resize_frame
 * refuses; a NULL rgb_hwc or depth_u16; im / depth or a small output with exactly one pointer NULL; all three
 * outputs absent; png_depth_scale not finite or <= 0; use_max_depth != 0 with a NaN max_depth.  Errors name
 * "ingest_frame". */
int gsr_ingest_frame(int H, int W, const unsigned char* rgb_hwc, const unsigned short* depth_u16,
                     double png_depth_scale, int use_max_depth, float max_depth, float* im, float* depth, int h0,
                     int w0, float* im_out0, float* depth_out0, int h1, int w1, float* im_out1, float* depth_out1,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_GLUE_H */
