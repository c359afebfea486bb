"""SplaTAM's per-frame loop on one capture: a SLAM sequence whose frames reuse one HIP-graph tracker and one
HIP-graph mapper.

scripts/splatam.py:697-929 runs, per frame t: the constant-velocity pose initialisation (initialize_camera_pose,
:429-448), `num_iters` tracking iterations with the best candidate written back (:700-763), add_new_gaussians
(:384-426: Gaussians from the pixels the map does not explain, appended to every parameter tensor), the mapping
iterations over a keyframe window (:796-905, prune_gaussians inside), and the keyframe bookkeeping.  P changes
every frame, and a captured graph needs fixed shapes, so the per-frame GraphTracker / GraphMapper of
splatam_amd.tracker / splatam_amd.mapper would be rebuilt every frame (probe, warm-up, capture: tens of ms).

Here the map lives in a capacity-padded buffer: every per-Gaussian tensor has `capacity + 1` rows, a device
`alive` mask marks the live ones (the rasterizer culls the others like Gaussians behind the camera: radius 0, no
instances, zero gradients), and `n_live` (device) counts the appended rows.  add_new_gaussians becomes
`densify_static`: the silhouette render, the masks and the point cloud of every pixel on the device, the new
rows scattered to n_live + (their rank among the selected pixels) -- no host synchronisation, no reallocation.
After a frame's pruning, compact_static moves the live rows to the front in order (remove_points without
a reallocation), so the padded map's live rows are always the reference map's rows in its order; the sequence
raises (check()) when the capacity is exhausted.  The tracker renders
from a one-column pose slot and slot targets that each frame fills; the mapper draws from a keyframe window
set per frame (GraphMapper.set_keyframes).

Densification has two forms (`densify_mode`): "torch" (the default), densify_static as above, and "device",
the silhouette render followed by splatam_amd.densify.densify_device (gsr_densify_frame: the median by
selection, the ranks and the new rows in six launches; only selected pixels write).  With densify_frames /
densify_cam / densify_intrinsics either form renders and reads a densification frame of its own resolution
(the reference's densification_image_height / width, scripts/splatam.py:801-812).  With track_frames / track_cam
the tracker renders and compares against a tracking frame of its own resolution (the reference's
tracking_image_height / width, scripts/splatam.py:517-523, 588-607, 680-687 -- what makes
configs/replica/splatam_s.py "SplaTAM-S"): only the tracker's slot holds it; densification, the keyframe dicts
and bank, mapping, evaluate() and the view scorer keep the full-resolution frames, as in the reference, where
only tracking_curr_data differs.  track_size / densify_size (h, w) have the sequence make those frames itself:
the cameras and intrinsics through splatam_amd.resize (resized_camera, scale_intrinsics), each frame's small
copies by one gsr_resize_frame launch (resize.resize_device) -- at construction for the frames given, in push()
for a frame that arrives, so the realtime loop's caller pushes the full frame and nothing else.

Two keyframe policies (`keyframe_policy`):
* "window" (the default): the last `window - 1` keyframes plus the current frame; frame 0 and every
  keyframe_every-th frame are keyframes.  The draws are window indices from the sequence's numpy stream.
* "overlap": SplaTAM's own selection (keyframe_selection_overlap, :820-837, utils/keyframe_selection.py): a
  random sample of the frame's depth pixels is back-projected and projected into every keyframe but the last;
  the window is a random `window - 2` of the keyframes that see any of it, plus the last keyframe and the
  current frame.  It runs on the device (splatam_amd.keyframes.select_device, three launches, after
  densification and before mapping) from a KeyframeBank that is appended at frame 0, at every
  keyframe_every-th frame and at frame num_frames - 2 (:932) with the pose as estimated then; the mapper
  gathers its per-iteration keyframes from the device-resident draws (GraphMapper.run(device_sequence=...)),
  so frame() still reads nothing back (but see track_cfg.use_depth_loss_thres below).  Randomness comes as 32-bit words from the sequence's numpy stream
  (`draws` records them); PerFrameSlam runs keyframes.select_literal on the same words.  The two deliberate
  differences from the reference (the random-word mapping, distinct pixels in one 1e-4 m cell are kept) are
  stated in splatam_amd/keyframes.py and include/gsr_glue.h.

track_cfg.use_depth_loss_thres (the reference's iPhone and ScanNet++ configurations; scripts/splatam.py:745-758):
a frame whose last tracking iteration's depth loss is not below track_cfg.depth_loss_thres tracks for
tracking_iters more iterations, once.  The depth loss is a sum over the TRACKING frame's pixels (as in the reference,
whose loss is formed on tracking_curr_data), so with a tracking resolution the threshold is resolution-dependent:
a quarter of the pixels give about a quarter of the sum.  Both loops then build their trackers with loss_terms=True and pass the
threshold to GraphTracker.track_frame, which reads that one float per tracked frame -- the only host read of
frame(), and only with the option on (the reference reads the loss in every iteration).  tracking_iters_run
lists, per frame() call, the tracking iterations run (0 for frame 0, which is not tracked): an entry of
2 * tracking_iters is one of the reference's "Extra Tracking Iters Frames".

The realtime loop (scripts/splatam_realtime.py) is the same sequence fed frame by frame: `num_frames` fixes the
pose columns while the frame list grows, SlamSequence.push(im, depth, w2c=None) appends a frame and runs it,
a frame with `w2c` (its pose relative to frame 0, tracking.use_gt_poses, :812-821) is not tracked
(write_given_pose), `map_every` (:844) maps every that-many-th frame, `median_thr` / `median_scale` are
add_new_gaussians' threshold there (:444-453; densify.depth_threshold, gsr_densify_frame_capped) and
SlamSequence(params=None) builds the map from the first frame on the device (init_map_device: gsr_init_frame).

That loop's frames arrive as the sensor delivers them (scripts/ros_handler.py:402-411): an interleaved uint8 image,
a uint16 depth image and an odometry pose.  SlamSequence.push_raw(rgb_u8, depth_u16, pose=None, w2c=None) takes
exactly that (png_depth_scale, max_depth): one gsr_ingest_frame launch (splatam_amd.ingest) writes the float
frame and, under track_size / densify_size, the small frames -- no gsr_resize_frame launch for such a frame --
and ingest.odometry_w2c makes the pose relative to the first one on the host.  Raw frames given at construction
({"rgb_u8", "depth_u16"[, "pose"]}) are ingested before anything reads them.  arrival_report=True keeps the
reference's on-arrival PSNR record (:431-446, 473-481) in `arrival`: every frame after the first rendered at its
pose before its densification and mapping, one row of evaluate.COLUMNS each, nothing read back.

The active-mapping node around that loop scores candidate views after every frame (scripts/ros_handler.py:251-359,
807-836): SlamSequence.view_scorer builds fisher.SequenceFisher graphs on the padded map once, fit_visited and
view_gains replay them on the map as it stands -- nothing on the frame() / push() path changes, and the scorer's
Monte-Carlo draws come from a stream of its own (`draws` and every result of the sequence are untouched).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .densify import ROW_KEYS, check_densify_args, default_threshold, densify_device, depth_threshold, \
    init_frame_device, init_literal
from .densify import make_workspace as make_densify_workspace
from .keyframes import KeyframeBank, WordFeed, draw_words, make_workspace, pose_w2c, select_device, \
    select_literal, words_tensor
from .mapper import GAUSS_KEYS, GraphMapper
from .ingest import ingest_device, odometry_w2c
from .resize import check_track_args, resize_device, resized_camera, scale_intrinsics
from .slam import MappingConfig, TrackingConfig, build_rotation, color_key, matrix_to_quaternion, \
    transform_to_frame, transformed_params2depthplussilhouette
from .tracker import GraphTracker

# dead rows: finite values (the pose-fused backward forms every row's pose partials, zero for culled rows)
_DEAD = {"means3D": 0.0, "rgb_colors": 0.0, "logit_opacities": -20.0, "log_scales": -10.0}


def pad_map(params: dict, capacity: int) -> tuple[dict, torch.Tensor, torch.Tensor]:
    """(padded params, alive uint8 [capacity + 1], n_live int64 [1]): every per-Gaussian tensor copied into
    `capacity + 1` rows (the last one a scatter sink that is never live), the camera tensors as they are."""
    P = params["means3D"].shape[0]
    if P > capacity:
        raise ValueError(f"capacity {capacity} < the map's {P} Gaussians")
    dev = params["means3D"].device
    out = {}
    for k, v in params.items():
        if k in ("cam_unnorm_rots", "cam_trans") or not torch.is_tensor(v) or v.dim() == 0 or v.shape[0] != P:
            out[k] = v
            continue
        t = torch.empty((capacity + 1,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
        if k == "unnorm_rotations":
            t.zero_()
            t[:, 0] = 1.0
        else:
            t.fill_(_DEAD.get(k, 0.0))
        t[:P] = v.detach()
        out[k] = t
    alive = torch.zeros(capacity + 1, dtype=torch.uint8, device=dev)
    alive[:P] = 1
    return out, alive, torch.full((1,), P, dtype=torch.int64, device=dev)


def initialize_camera_pose(params: dict, t: int, forward_prop: bool = True):
    """initialize_camera_pose (scripts/splatam.py:429-448): the constant-velocity model from t - 1 and t - 2,
    else the previous pose; device tensor ops only."""
    with torch.no_grad():
        q, tr = params["cam_unnorm_rots"], params["cam_trans"]
        if t > 1 and forward_prop:
            r1, r2 = F.normalize(q[..., t - 1].detach()), F.normalize(q[..., t - 2].detach())
            q[..., t] = F.normalize(r1 + (r1 - r2)).detach()
            t1, t2 = tr[..., t - 1].detach(), tr[..., t - 2].detach()
            tr[..., t] = (t1 + (t1 - t2)).detach()
        else:
            q[..., t] = q[..., t - 1].detach()
            tr[..., t] = tr[..., t - 1].detach()


def frame_pointcloud(params: dict, curr: dict, t: int, intrinsics) -> dict:
    """get_pointcloud + initialize_new_params (scripts/splatam.py:73-124,356-381; projective scales, isotropic)
    for EVERY pixel of the frame: the new Gaussian each pixel would add (world-frame mean from the depth and the
    pose of column t, the pixel's colour, log_scale = log(sqrt((z / mean focal)^2)), opacity logit 0, identity
    rotation)."""
    im, depth = curr["im"], curr["depth"]
    H, W = im.shape[1], im.shape[2]
    fx, fy, cx, cy = intrinsics
    dev = im.device
    with torch.no_grad():
        rot = F.normalize(params["cam_unnorm_rots"][..., t].detach())
        w2c = torch.eye(4, device=dev, dtype=torch.float32)
        w2c[:3, :3] = build_rotation(rot)
        w2c[:3, 3] = params["cam_trans"][..., t].detach()
        # c2w: the rigid transform's closed-form inverse [R^T, -R^T t] (the reference's torch.inverse forms the
        # same matrix by LU; both SplaTAM forms here use this one)
        c2w = torch.eye(4, device=dev, dtype=torch.float32)
        rt = w2c[:3, :3].transpose(0, 1)
        c2w[:3, :3] = rt
        c2w[:3, 3] = -(rt @ w2c[:3, 3])
        xg, yg = torch.meshgrid(torch.arange(W, device=dev).float(), torch.arange(H, device=dev).float(), indexing="xy")
        xx, yy = ((xg - cx) / fx).reshape(-1), ((yg - cy) / fy).reshape(-1)
        z = depth[0].reshape(-1)
        pts4 = torch.stack((xx * z, yy * z, z, torch.ones_like(z)), dim=-1)
        pts = (c2w @ pts4.T).T[:, :3]
        mean3_sq_dist = (z / ((fx + fy) / 2)) ** 2
        n = pts.shape[0]
        return {"means3D": pts.contiguous(), "rgb_colors": im.permute(1, 2, 0).reshape(-1, 3).contiguous(),
                "unnorm_rotations": torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(n, 1),
                "logit_opacities": torch.zeros(n, 1, device=dev),
                "log_scales": torch.log(torch.sqrt(mean3_sq_dist))[..., None].contiguous()}


def identity_poses(num_frames: int, device) -> dict:
    """initialize_params' camera tensors: the identity quaternion [1, 4, num_frames] and a zero translation
    [1, 3, num_frames] in every column (poses relative to frame 0)."""
    q = torch.zeros(1, 4, int(num_frames), dtype=torch.float32, device=device)
    q[:, 0] = 1.0
    return {"cam_unnorm_rots": q, "cam_trans": torch.zeros(1, 3, int(num_frames), dtype=torch.float32, device=device)}


def init_map_literal(frame: dict, w2c: torch.Tensor, intrinsics, num_frames: int) -> dict:
    """initialize_first_timestep's map (scripts/splatam_realtime.py:229-237) in torch ops: frame_pointcloud's
    rows through the first frame's w2c [4,4] for the pixels with a measured depth, in row-major order, and
    identity_poses.  The rows are formed as gsr_init_frame's contract states them (densify.init_literal:
    elementwise float32 ops, the matrix product as left-to-right sums, true divisions), so the kernel forms the
    same bits on any device (log_scales up to logf).  One host synchronisation (the boolean mask)."""
    out, _, _ = init_literal(frame, w2c, intrinsics)
    out.update(identity_poses(num_frames, frame["depth"].device))
    return out


def init_map_device(frame: dict, w2c: torch.Tensor, intrinsics, num_frames: int, capacity: int, overflow=None,
                    workspace=None) -> tuple[dict, torch.Tensor, torch.Tensor]:
    """(params, alive, n_live): init_map_literal's map as a capacity-padded one without a host read -- pad_map's
    dead rows, filled from row 0 by gsr_init_frame (densify.init_frame_device, two launches) -- and
    identity_poses.  overflow (one byte, device): set when the frame has more measured pixels than capacity."""
    depth = frame["depth"]
    dev, H, W = depth.device, int(depth.shape[-2]), int(depth.shape[-1])
    empty = {k: torch.zeros(0, c, dtype=torch.float32, device=dev) for k, c in zip(ROW_KEYS, (3, 3, 4, 1, 1))}
    params, alive, n_live = pad_map(empty, int(capacity))
    params.update(identity_poses(num_frames, dev))
    overflow = torch.zeros(1, dtype=torch.bool, device=dev) if overflow is None else overflow
    workspace = make_densify_workspace(H, W, dev) if workspace is None else workspace
    init_frame_device(params, alive, n_live, overflow, frame, w2c.to(torch.float32).contiguous(), intrinsics,
                      capacity, workspace)
    return params, alive, n_live


def write_given_pose(params: dict, t: int, w2c: torch.Tensor):
    """A frame whose pose is known (tracking.use_gt_poses, scripts/splatam_realtime.py:812-821): w2c [4,4], the
    pose relative to frame 0, into column t -- matrix_to_quaternion of its rotation and its translation.
    Device tensor ops only."""
    with torch.no_grad():
        params["cam_unnorm_rots"][..., t] = matrix_to_quaternion(w2c[:3, :3].unsqueeze(0).detach())
        params["cam_trans"][..., t] = w2c[:3, 3].detach()


def non_presence_mask(depth_sil: torch.Tensor, gt_depth: torch.Tensor, sil_thres: float, median_thr=None,
                      median_scale: float = 50.0) -> torch.Tensor:
    """add_new_gaussians' pixel selection (scripts/splatam.py:391-410), flattened: silhouette below sil_thres,
    or rendered depth behind the measured depth by more than 50x the median depth error; valid depth only.
    median_thr / median_scale: the realtime loop's threshold (densify.depth_threshold; no host read)."""
    sil = depth_sil[1]
    gt = gt_depth[0]
    rd = depth_sil[0]
    err = torch.abs(gt - rd) * (gt > 0)
    thr = 50 * err.median() if default_threshold(median_thr, median_scale) else \
        depth_threshold(err.median(), median_thr, median_scale)
    m = (sil < sil_thres) | ((rd > gt) & (err > thr))
    return (m & (gt > 0)).reshape(-1)


def render_depth_sil(params: dict, curr: dict, t: int, alive=None, capacity: int = 0, status=None):
    """The depth / silhouette render of add_new_gaussians (transform_to_frame + the [z, 1, z^2] rendervars,
    slam_helpers.py:234-304) through the rasterizer: static-capacity with the alive mask when given."""
    from .rasterizer import GaussianRasterizer, rasterize_gaussians_dual
    with torch.no_grad():
        tg = transform_to_frame(params, t, gaussians_grad=False, camera_grad=False)
        rv = transformed_params2depthplussilhouette(params, curr["w2c"], tg)
        if alive is None and capacity <= 0:
            ds, _, _ = GaussianRasterizer(raster_settings=curr["cam"])(**rv)
            return ds
        _, ds, _, _ = rasterize_gaussians_dual(rv["means3D"], torch.zeros_like(rv["means3D"]), None,
                                               rv["colors_precomp"], rv["colors_precomp"], rv["opacities"],
                                               rv["scales"], rv["rotations"], None, curr["cam"], capacity, status,
                                               grad2_channels=1, alive=alive)
        return ds


def add_new_gaussians_literal(params: dict, curr: dict, t: int, intrinsics, sil_thres: float = 0.5, median_thr=None,
                              median_scale: float = 50.0) -> dict:
    """add_new_gaussians (scripts/splatam.py:384-426) on an unpadded map: the selected pixels' Gaussians
    appended with torch.cat (the reference's reallocation; one host synchronisation for the selection).
    Returns the new params dict (Gaussian tensors new leaves; the camera tensors as they were)."""
    ds = render_depth_sil(params, curr, t)
    mask = non_presence_mask(ds, curr["depth"], sil_thres, median_thr, median_scale)
    new = frame_pointcloud(params, curr, t, intrinsics)
    out = dict(params)
    for k, v in new.items():
        out[k] = torch.cat((params[k].detach(), v[mask]), dim=0).requires_grad_(params[k].requires_grad)
    return out


def add_new_gaussians_device(params: dict, curr: dict, t: int, intrinsics, sil_thres: float = 0.5, median_thr=None,
                             median_scale: float = 50.0) -> dict:
    """add_new_gaussians on an unpadded map through the kernel of the padded one: the unpadded silhouette
    render, gsr_densify_frame (splatam_amd.densify.densify_device) on a throw-away padded copy with room
    for every pixel, and the rows up to n_live sliced out with one host read -- what torch.cat would hold,
    so the per-frame loop stays the bitwise comparison form of SlamSequence(densify_mode="device")."""
    ds = render_depth_sil(params, curr, t)
    H, W = ds.shape[-2], ds.shape[-1]
    capacity = params["means3D"].shape[0] + H * W
    dev = ds.device
    with torch.no_grad():
        padded, alive, n_live = pad_map({k: params[k] for k in ROW_KEYS}, capacity)
        overflow = torch.zeros(1, dtype=torch.bool, device=dev)
        densify_device(padded, alive, n_live, overflow, curr, pose_w2c(params, t), intrinsics, sil_thres, capacity,
                       ds.contiguous(), make_densify_workspace(H, W, dev), median_thr=median_thr,
                       median_scale=median_scale)
        n = int(n_live.item())
    out = dict(params)
    for k in ROW_KEYS:
        out[k] = padded[k][:n].clone().requires_grad_(params[k].requires_grad)
    return out


def densify_static(params: dict, alive: torch.Tensor, n_live: torch.Tensor, overflow: torch.Tensor, curr: dict,
                   t: int, intrinsics, sil_thres: float, capacity: int, bin_capacity: int, status, median_thr=None,
                   median_scale: float = 50.0):
    """add_new_gaussians on a capacity-padded map, without a host synchronisation: the selected pixels'
    Gaussians (frame_pointcloud) land in rows n_live + rank, every other pixel writes to the sink row
    `capacity`; alive marks the new rows, n_live grows (clamped; `overflow` set when the map is full)."""
    ds = render_depth_sil(params, curr, t, alive, bin_capacity, status)
    with torch.no_grad():
        mask = non_presence_mask(ds, curr["depth"], sil_thres, median_thr, median_scale)
        new = frame_pointcloud(params, curr, t, intrinsics)
        incl = torch.cumsum(mask.to(torch.int64), 0)
        dest = n_live + incl - 1
        ok = mask & (dest < capacity)
        dest = torch.where(ok, dest, torch.full_like(dest, capacity))
        for k, v in new.items():
            params[k].data.index_put_((dest,), v)
        alive.index_put_((dest,), ok.to(torch.uint8))
        total = n_live + incl[-1:]
        overflow.logical_or_(total > capacity)
        n_live.copy_(torch.clamp(total, max=capacity))


def compact_static(params: dict, alive: torch.Tensor, n_live: torch.Tensor, capacity: int):
    """remove_points (utils/slam_external.py:141-163) on a capacity-padded map, without a host
    synchronisation or a reallocation: the live rows move, in order, to the front (their rank among the live
    rows; the dead ones to the sink row), alive becomes the prefix [0, count), n_live the count.  The map's
    rows are then those of the compacted reference map, in the same order, so the next frame's densified
    rows land where torch.cat puts them."""
    with torch.no_grad():
        keep = alive.bool()
        rank = torch.cumsum(keep.to(torch.int64), 0) - 1
        dest = torch.where(keep, rank, torch.full_like(rank, capacity))
        for k, v in params.items():
            if k in ("cam_unnorm_rots", "cam_trans") or not torch.is_tensor(v) or v.dim() == 0 or \
                    v.shape[0] != capacity + 1:
                continue
            v.data.index_put_((dest,), v.detach().clone())
        count = rank[-1:] + 1
        alive.copy_((torch.arange(capacity + 1, device=alive.device) < count).to(torch.uint8))
        n_live.copy_(count)


def _check_policy(keyframe_policy: str, window: int):
    if keyframe_policy not in ("window", "overlap"):
        raise ValueError(f"keyframe_policy {keyframe_policy!r}: 'window' or 'overlap'")
    if keyframe_policy == "overlap" and window < 2:
        raise ValueError("keyframe_policy 'overlap' needs window >= 2 (the last keyframe and the current frame)")


class _SequenceBase:
    """What SlamSequence and PerFrameSlam share: the loop's options, the keyframe dicts, the densification frame,
    the "window" policy's window, both policies' keyframe rule and an "overlap" frame's random-word counts."""

    OPTIONS = ("frames", "cam", "w2c", "intrinsics", "bin_capacity", "tracking_iters", "mapping_iters", "track_replay",
               "window", "keyframe_every", "sil_thres", "track_cfg", "map_cfg", "prune", "scene_radius",
               "keyframe_policy", "overlap_pixels", "densify_mode", "densify_frames", "densify_cam",
               "densify_intrinsics", "median_thr", "median_scale", "num_frames", "map_every", "track_frames",
               "track_cam", "track_size", "densify_size", "png_depth_scale", "max_depth", "arrival_report")

    def _set_options(self, args: dict):
        """Stores the constructor arguments both classes take (OPTIONS, out of the constructor's locals()) as
        attributes of their names, validated, and starts the keyframe list with frame 0."""
        for k in self.OPTIONS:
            setattr(self, k, args[k])
        _check_policy(self.keyframe_policy, self.window)
        if self.num_frames is not None and not 1 <= len(self.frames) <= int(self.num_frames):
            raise ValueError(f"num_frames {self.num_frames}: between 1 and num_frames frames to start with")
        if int(self.map_every) < 1:
            raise ValueError("map_every >= 1")
        premade = self._ingest_given()
        check_densify_args(self.densify_mode, self.densify_frames, self.densify_cam, self.densify_intrinsics,
                           self.frames)
        check_track_args(self.track_frames, self.track_cam, self.frames)
        self._set_sizes(premade)
        self.overlap_pixels = int(self.overlap_pixels)
        if self.scene_radius is None:  # initialize_first_timestep: max depth / scene_radius_depth_ratio (3, the config's)
            self.scene_radius = self.frames[0]["depth"].max() / 3.0
        self.keyframes = [self._kf(0)]
        self.tracking_iters_run = []  # per frame() call: the tracking iterations run (0: frame 0, not tracked)

    def _owns_small_frames(self) -> bool:
        """Whether the caller gives the small frames (track_frames / densify_frames without track_size /
        densify_size): such a capture is not fed raw frames."""
        return (self.track_frames is not None and self.track_size is None) or \
            (self.densify_frames is not None and self.densify_size is None)

    def _ingest_raw(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor) -> tuple:
        """(frame, tracking frame, densification frame) of a raw sensor frame (splatam_amd.ingest: uint8 [H,W,3],
        uint16 [H,W]) under png_depth_scale / max_depth and track_size / densify_size (None where the size is not
        set): one gsr_ingest_frame launch for all of them, nothing read back."""
        if self.png_depth_scale is None:
            raise ValueError("a raw frame needs png_depth_scale (the sensor units per metre)")
        ts, ds = self.track_size, self.densify_size
        sizes = [s for s in (ts, ds) if s is not None]
        out = ingest_device(rgb_u8, depth_u16, self.png_depth_scale, self.max_depth, *sizes)
        if not sizes:
            return out, None, None
        smalls = list(out[1:])
        return out[0], (smalls.pop(0) if ts is not None else None), (smalls.pop(0) if ds is not None else None)

    def _ingest_given(self):
        """Raw frames given at construction ({"rgb_u8", "depth_u16"[, "pose"]} each, with png_depth_scale): the
        frame list becomes their float frames (a new list), before anything reads a frame.  Returns per frame
        the (tracking frame, densification frame) the same launch made, for _set_sizes; None for float frames.
        The first frame's "pose" (x, y, z, qx, qy, qz, qw), when given, is what push_raw's poses are relative to."""
        self.initial_pose = None
        raw = ["rgb_u8" in f for f in self.frames]
        if not any(raw):
            return None
        if not all(raw):
            raise ValueError("frames: raw ({'rgb_u8', 'depth_u16'}) or float ({'im', 'depth'}), not both")
        if self._owns_small_frames():
            raise ValueError("raw frames: a capture with track_frames / densify_frames owns its small frames")
        given = self.frames
        made = [self._ingest_raw(f["rgb_u8"], f["depth_u16"]) for f in given]
        self.frames = [m[0] for m in made]
        if given[0].get("pose") is not None:
            self.initial_pose = np.array(given[0]["pose"], dtype=np.float64)
        return [m[1:] for m in made]

    def _set_sizes(self, premade=None):
        """track_size / densify_size (h, w): the sequence makes the small frames itself -- the camera (and the
        densification intrinsics) through splatam_amd.resize, the frames given so far by one gsr_resize_frame
        launch each (_make_small; `premade`: _ingest_given's, for raw frames, whose ingest launch made them).
        Exclusive with track_frames / densify_frames."""
        if self.track_size is not None and self.track_frames is not None:
            raise ValueError("track_size: exclusive with track_frames / track_cam")
        if self.densify_size is not None and self.densify_frames is not None:
            raise ValueError("densify_size: exclusive with densify_frames / densify_cam / densify_intrinsics")
        if self.track_size is None and self.densify_size is None:
            return
        d0 = self.frames[0]["depth"]
        H, W, dev = int(d0.shape[-2]), int(d0.shape[-1]), d0.device
        w2c = None if self.w2c is None else self.w2c.detach().cpu()
        if self.track_size is not None:
            self.track_size = tuple(int(v) for v in self.track_size)
            self.track_cam = resized_camera(W, H, self.intrinsics, *self.track_size, dev, w2c=w2c)
            self.track_frames = []
        if self.densify_size is not None:
            self.densify_size = tuple(int(v) for v in self.densify_size)
            self.densify_cam = resized_camera(W, H, self.intrinsics, *self.densify_size, dev, w2c=w2c)
            self.densify_intrinsics = scale_intrinsics(self.intrinsics, H, W, *self.densify_size)
            self.densify_frames = []
        for i, f in enumerate(self.frames):
            tf, df = self._make_small(f) if premade is None else premade[i]
            if tf is not None:
                self.track_frames.append(tf)
            if df is not None:
                self.densify_frames.append(df)

    def _make_small(self, frame: dict) -> tuple:
        """(tracking frame, densification frame) of a full frame under track_size / densify_size (None where
        the size is not set): one gsr_resize_frame launch for both, nothing read back."""
        ts, ds = self.track_size, self.densify_size
        if ts is not None and ds is not None:
            return resize_device(frame, ts, ds)
        if ts is not None:
            return resize_device(frame, ts), None
        return None, (resize_device(frame, ds) if ds is not None else None)

    def _depth_loss_thres(self):
        """GraphTracker.track_frame's depth_loss_thres: the configured threshold, or None (option off)."""
        cfg = self.track_cfg
        return float(cfg.depth_loss_thres) if cfg.use_depth_loss_thres else None

    def _n_frames(self) -> int:
        """The capture's length: num_frames when given (the frame list may still be growing), else the list's."""
        return len(self.frames) if self.num_frames is None else int(self.num_frames)

    def _maps(self, t: int) -> bool:
        """Whether frame t densifies and maps (map_every, scripts/splatam_realtime.py:844): frame 0 always."""
        return t == 0 or (t + 1) % int(self.map_every) == 0

    def _append_frame(self, im: torch.Tensor, depth: torch.Tensor, densify_frame=None, track_frame=None,
                      made=None) -> int:
        """A frame that arrived: appended to the frame list (and its densification frame to densify_frames, its
        tracking frame to track_frames, when the capture has those; under densify_size / track_size the sequence
        makes them here, _make_small, and takes none -- unless `made`, the (tracking frame, densification frame)
        _ingest_raw's launch made already).  Returns its index; ValueError beyond num_frames (the pose columns)."""
        t = len(self.frames)
        if self.num_frames is None or t >= int(self.num_frames):
            raise ValueError(f"frame {t}: the sequence holds num_frames = {self.num_frames} frames")
        if (densify_frame is not None and self.densify_size is not None) or \
                (track_frame is not None and self.track_size is not None):
            raise ValueError("densify_size / track_size: the sequence makes that frame itself")
        if self.densify_size is None and (densify_frame is None) != (self.densify_frames is None):
            raise ValueError("densify_frame: one per frame when the capture has densify_frames, else none")
        if self.track_size is None and (track_frame is None) != (self.track_frames is None):
            raise ValueError("track_frame: one per frame when the capture has track_frames, else none")
        made_t, made_d = self._make_small({"im": im, "depth": depth}) if made is None else made
        track_frame = made_t if track_frame is None else track_frame
        densify_frame = made_d if densify_frame is None else densify_frame
        self.frames.append({"im": im, "depth": depth})
        if densify_frame is not None:
            self.densify_frames.append(densify_frame)
        if track_frame is not None:
            self.track_frames.append(track_frame)
        return t

    def _push_raw_frame(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor, pose=None, w2c=None) -> tuple:
        """push_raw's intake: the checks, the one gsr_ingest_frame launch (_ingest_raw: the full frame and the
        small ones, so _make_small is not called for this frame), the _append_frame bookkeeping and the pose.
        Returns (t, w2c): `pose` (x, y, z, qx, qy, qz, qw) through ingest.odometry_w2c against the first pose
        pushed (or the first raw frame's "pose"), on its way to the device by a non-blocking copy."""
        if self.png_depth_scale is None:
            raise ValueError("push_raw needs png_depth_scale (the sensor units per metre)")
        if pose is not None and w2c is not None:
            raise ValueError("push_raw: pose or w2c, not both")
        if self._owns_small_frames():
            raise ValueError("push_raw: a capture with track_frames / densify_frames owns its small frames "
                             "(push_frames)")
        if self.num_frames is None or len(self.frames) >= int(self.num_frames):
            raise ValueError(f"frame {len(self.frames)}: the sequence holds num_frames = {self.num_frames} frames")
        frame, tf, df = self._ingest_raw(rgb_u8, depth_u16)
        t = self._append_frame(frame["im"], frame["depth"], made=(tf, df))
        if pose is not None:
            if self.initial_pose is None:
                self.initial_pose = np.array(pose, dtype=np.float64)
            w2c = odometry_w2c(self.initial_pose, pose, device=frame["depth"].device)
        return t, w2c

    def _kf(self, t: int) -> dict:
        return {"cam": self.cam, "w2c": self.w2c, "im": self.frames[t]["im"], "depth": self.frames[t]["depth"], "id": t}

    def _track_curr(self, t: int) -> dict:
        """What the tracker renders and compares against for frame t: the frame itself, or the tracking
        resolution's (track_frames / track_cam, scripts/splatam.py:588-607, 680-687); w2c stays the first frame's."""
        f, cam = (self.frames[t], self.cam) if self.track_frames is None else (self.track_frames[t], self.track_cam)
        return {"cam": cam, "w2c": self.w2c, "im": f["im"], "depth": f["depth"]}

    def _densify_kf(self, t: int) -> tuple[dict, tuple]:
        """The frame densification reads and its intrinsics: the tracking frame, or the densification
        resolution's (densify_frames / densify_cam / densify_intrinsics, scripts/splatam.py:801-812)."""
        if self.densify_frames is None:
            return self._kf(t), self.intrinsics
        f = self.densify_frames[t]
        return dict(self._kf(t), cam=self.densify_cam, im=f["im"], depth=f["depth"]), self.densify_intrinsics

    def _window(self, t: int) -> list:  # "window": the last window - 1 keyframes plus frame t
        return self.keyframes[-(self.window - 1):] + ([self._kf(t)] if self.keyframes[-1]["id"] != t else [])

    def _is_keyframe(self, t: int) -> bool:
        """Whether frame t joins the keyframes after its mapping: every keyframe_every-th frame
        (scripts/splatam.py:907-913; frame 0 is one from the start) and, "overlap" (:932), frames 0 and num_frames - 2."""
        every = (t + 1) % self.keyframe_every == 0
        if self.keyframe_policy == "overlap":
            return every or t in (0, self._n_frames() - 2)
        return every and t > 0

    def _word_counts(self, n_kf: int) -> tuple[int, int, int]:
        """An "overlap" frame's random words with n_kf keyframes: the sample's, the candidate keyframes' keys, and
        all of them (with one per mapping iteration)."""
        S, n_cand = self.overlap_pixels, max(n_kf - 1, 0)
        return S, n_cand, S + n_cand + self.mapping_iters


class SlamSequence(_SequenceBase):
    """Frames of SplaTAM's loop on a capacity-padded map with one GraphTracker and one GraphMapper.

    params: the initial map (SplaTAM's init from frame 0; isotropic, rgb colours) with one pose column per frame;
    frames: per frame {"im", "depth"} targets (all sharing `cam` / `w2c`, the first frame's, like the reference);
    intrinsics (fx, fy, cx, cy).  frame(t) runs one frame; run(frames) a range of them; push(im, depth) one that
    arrives (num_frames given).  params None: the map is init_map_device's, from frames[0].
    track_frames / track_cam: the tracker's frames and camera at a resolution of their own (everything else
    keeps `frames`); track_size / densify_size (h, w): the sequence makes the tracking / densification frames
    and cameras itself (splatam_amd.resize)."""

    def __init__(self, params: dict, frames: list, cam, w2c, intrinsics, capacity: int, bin_capacity: int,
                 tracking_iters: int = 40, mapping_iters: int = 60, track_replay: int = 20, window: int = 8,
                 keyframe_every: int = 5, sil_thres: float = 0.5, track_cfg: TrackingConfig = TrackingConfig(),
                 map_cfg: MappingConfig = MappingConfig(), prune: bool | None = None, seed: int = 0,
                 scene_radius=None, keyframe_policy: str = "window", overlap_pixels: int = 1600,
                 densify_mode: str = "torch", densify_frames=None, densify_cam=None, densify_intrinsics=None,
                 median_thr=None, median_scale: float = 50.0, num_frames: int | None = None, map_every: int = 1,
                 track_frames=None, track_cam=None, track_size=None, densify_size=None, png_depth_scale=None,
                 max_depth=None, arrival_report: bool = False):
        if params is not None and (color_key(params) != "rgb_colors" or params["log_scales"].shape[1] != 1):
            raise ValueError("SlamSequence: SplaTAM's isotropic rgb map (the tracking fast path's form)")
        if tracking_iters % track_replay:
            raise ValueError("tracking_iters must be a multiple of track_replay")
        self._set_options(locals())
        frames = self.frames  # (raw frames given: their float frames, _ingest_given)
        self.bin_capacity, self.seed = int(bin_capacity), seed
        self.rng = np.random.RandomState(seed)
        self.draws = []  # per frame: the mapper's keyframe draws (window indices; None: the frame did not map); "overlap": the random words
        dev = frames[0]["depth"].device if params is None else params["means3D"].device
        if keyframe_policy == "overlap":
            f0 = frames[0]
            self.bank = KeyframeBank(f0["im"].shape, f0["depth"].shape, dev)
            self.feed = WordFeed(dev)
            self.kf_workspace = make_workspace(f0["depth"].shape[-2], self.overlap_pixels, dev)
            self.selections = []  # per frame: select_device's outputs (device tensors; nothing is read here)
        self.overflow = torch.zeros(1, dtype=torch.bool, device=dev)
        self.dstatus = torch.zeros(4, dtype=torch.int32, device=dev)
        if densify_mode == "device":
            d0 = (self.densify_frames if self.densify_frames is not None else frames)[0]["depth"]
            self.densify_workspace = make_densify_workspace(d0.shape[-2], d0.shape[-1], dev)
        if arrival_report:
            from . import evaluate as ev
            d0 = frames[0]["depth"]
            self.arrival = torch.full((self._n_frames(), 8), float("nan"), dtype=torch.float32, device=dev)
            self.arrival_workspace = ev.make_workspace(d0.shape[-2], d0.shape[-1], dev, ms_ssim=False)
            self.arrival_status = torch.zeros(4, dtype=torch.int32, device=dev)
        padded = None
        if params is None:  # the map is born from frame 0 (initialize_first_timestep), on the device
            kf, intr = self._densify_kf(0)
            padded = init_map_device(kf, w2c, intr, self._n_frames(), int(capacity), overflow=self.overflow,
                                     workspace=getattr(self, "densify_workspace", None))
            params = padded[0]
        self._build(params, int(capacity), padded)

    def _build(self, params: dict, capacity: int, padded=None):
        """The padded map of `params` (its per-Gaussian rows live; `padded`: pad_map's triple, when the caller
        built it) and the tracker / mapper graphs over it."""
        self._retire_scorer()
        self.capacity = capacity
        self.params, self.alive, self.n_live = pad_map(params, self.capacity) if padded is None else padded
        for k in GAUSS_KEYS + ("rgb_colors",):
            self.params[k].requires_grad_(True)
        q, tr = params["cam_unnorm_rots"], params["cam_trans"]
        self.params["cam_unnorm_rots"] = q.detach().clone()
        self.params["cam_trans"] = tr.detach().clone()
        # the tracker's pose slot (one column) and targets: filled per frame; the map tensors as detached views
        # (the same storage: every replay reads the current map; tracking differentiates the pose only)
        self.slot = {k: (v.detach() if k in GAUSS_KEYS + ("rgb_colors",) else v) for k, v in self.params.items()}
        self.slot["cam_unnorm_rots"] = q[..., :1].detach().clone().requires_grad_(True)
        self.slot["cam_trans"] = tr[..., :1].detach().clone().requires_grad_(True)
        c0 = self._track_curr(0)  # (the tracking resolution's frame and camera, when the capture has those)
        self.slot_curr = dict(c0, im=c0["im"].clone(), depth=c0["depth"].clone())
        self.tracker = GraphTracker(self.slot, self.slot_curr, 0, iters_per_graph=self.track_replay,
                                    cfg=self.track_cfg, warmup_iters=1, fuse_pose=True, alive=self.alive,
                                    capacity=self.bin_capacity, loss_terms=self.track_cfg.use_depth_loss_thres)
        self.mapper = GraphMapper(self.params, self.keyframes, iters_per_graph=self.mapping_iters, cfg=self.map_cfg,
                                  seed=self.seed, prune=self.prune, scene_radius=self.scene_radius,
                                  alive=self.alive, capacity=self.bin_capacity)
        if self.keyframe_policy == "overlap":
            self.mapper.set_keyframe_bank(self.bank.im, self.bank.depth)

    def ensure_headroom(self, free: int) -> bool:
        """One host read of n_live: when fewer than `free` rows are left, move the map into a larger buffer
        (max(2 x capacity, n_live + free) rows) and rebuild the two graphs -- the live rows and their order
        unchanged, so the results are the same bits.  Every per-Gaussian launch covers the whole capacity
        (bench.py's sequence leg: 45.6 frames/s at 342 k rows, 27.1 at 1.84 M for the same 293 k live
        Gaussians), so size it to the map and grow on demand.  Returns True when it grew (a cached view scorer
        is then stale: the next scoring call rebuilds it, counted in scorer_captures)."""
        n = int(self.n_live.item())
        if self.capacity - n >= free:
            return False
        self._build(self.live_params(), max(2 * self.capacity, n + int(free)))
        return True

    def track(self, t: int):
        """initialize_camera_pose, then tracking_iters iterations from the pose slot (best candidate written
        back into column t); with track_cfg.use_depth_loss_thres, once more unless the depth loss fell below the
        threshold (one host read).  Returns the iterations run."""
        p = self.params
        initialize_camera_pose(p, t)
        with torch.no_grad():
            self.slot["cam_unnorm_rots"][..., 0] = p["cam_unnorm_rots"][..., t]
            self.slot["cam_trans"][..., 0] = p["cam_trans"][..., t]
            curr = self._track_curr(t)
            self.slot_curr["im"].copy_(curr["im"])
            self.slot_curr["depth"].copy_(curr["depth"])
        ran = self.tracker.track_frame(self.tracking_iters, check=False, depth_loss_thres=self._depth_loss_thres())
        with torch.no_grad():
            p["cam_unnorm_rots"][..., t] = self.slot["cam_unnorm_rots"][..., 0]
            p["cam_trans"][..., t] = self.slot["cam_trans"][..., 0]
        return ran

    def densify(self, t: int):
        """add_new_gaussians without a host read.  densify_mode "torch": densify_static; "device": the
        silhouette render, then splatam_amd.densify.densify_device (one call, only the new rows written)."""
        kf, intr = self._densify_kf(t)
        if self.densify_mode == "torch":
            densify_static(self.params, self.alive, self.n_live, self.overflow, kf, t, intr,
                           self.sil_thres, self.capacity, self.bin_capacity, self.dstatus, self.median_thr,
                           self.median_scale)
            return
        ds = render_depth_sil(self.params, kf, t, self.alive, self.bin_capacity, self.dstatus)
        densify_device(self.params, self.alive, self.n_live, self.overflow, kf, pose_w2c(self.params, t), intr,
                       self.sil_thres, self.capacity, ds, self.densify_workspace, median_thr=self.median_thr,
                       median_scale=self.median_scale)

    def map(self, t: int, sequence=None):
        """The mapping frame over the window (the last window - 1 keyframes + frame t), keyframe draws from the
        sequence's numpy stream (np.random.randint, scripts/splatam.py:851) unless `sequence` is given.
        keyframe_policy "overlap": _map_overlap (`sequence`: the frame's random words)."""
        if self.keyframe_policy == "overlap":
            return self._map_overlap(t, sequence)
        win = self._window(t)
        self.mapper.set_keyframes(win)
        seq = [int(self.rng.randint(0, len(win))) for _ in range(self.mapping_iters)] if sequence is None else sequence
        self.draws.append(seq)
        self.mapper.run(check=False, sequence=seq)
        self._compact_pruned()
        self._add_keyframe(t)

    def _add_keyframe(self, t: int):
        """The keyframe bookkeeping after a frame (scripts/splatam.py:907-913, 932-945), mapped or not."""
        if not self._is_keyframe(t):
            return
        if self.keyframe_policy == "overlap":
            f = self.frames[t]
            if self.bank.append(f["im"], f["depth"], self.params, t):  # (the bank doubled: new tensors)
                self.mapper.set_keyframe_bank(self.bank.im, self.bank.depth)
        else:
            self.keyframes.append(self._kf(t))

    def _compact_pruned(self):
        if self.mapper.prune_at:  # the frame's pruned Gaussians removed for good (in place, no sync)
            compact_static(self.params, self.alive, self.n_live, self.capacity)

    def _map_overlap(self, t: int, words=None):
        """The mapping frame under the overlap policy, without a host read: the frame into the bank's last
        row, the frame's random words (overlap_pixels for the sample, one key per candidate keyframe,
        one per mapping iteration) to the device, select_device, the mapper's replay from its draws, and the
        keyframe bookkeeping of scripts/splatam.py:932-945."""
        bank, f = self.bank, self.frames[t]
        bank.set_current(f["im"], f["depth"])
        S, n_cand, total = self._word_counts(bank.n)
        words = draw_words(self.rng, total) if words is None else \
            np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
        if words.shape != (total,):
            raise ValueError(f"frame {t}: {total} random words")
        self.draws.append(words)
        w = self.feed.push(words)
        sel = select_device(f["depth"], self.intrinsics, pose_w2c(self.params, t), bank.est_w2c, bank.n,
                            self.window - 2, w[:S], w[S:S + n_cand], w[S + n_cand:], bank.time, t, bank.cur_row,
                            workspace=self.kf_workspace)
        self.selections.append(sel)
        self.mapper.run(check=False, device_sequence=(sel["draw_rows"], sel["draw_times"]))
        self._compact_pruned()
        self._add_keyframe(t)

    def frame(self, t: int, sequence=None, w2c=None):
        """One frame of scripts/splatam.py:697-929: tracking (t > 0), densification (t > 0), mapping.
        w2c (device [4,4], the frame's pose relative to frame 0; tracking.use_gt_poses): the frame is not tracked,
        write_given_pose fills column t (ignored for frame 0, whose column is the identity).  A frame that does
        not map (map_every) does not densify either; its keyframe bookkeeping still runs."""
        ran = 0
        if t > 0:
            if w2c is None:
                ran = self.track(t)
            else:
                write_given_pose(self.params, t, w2c)
            if self.arrival_report:
                self.report_arrival(t)
            if self._maps(t):
                self.densify(t)
        self.tracking_iters_run.append(ran)
        if self._maps(t):
            self.map(t, sequence)
        else:
            self.draws.append(None)
            self._add_keyframe(t)

    def report_arrival(self, t: int):
        """The reference's on-arrival record (scripts/ros_handler.py:431-446, 473-481: gain_psnr_arr's "psnr"):
        frame t rendered at its pose column from the map as it stands BEFORE the frame's densification and
        mapping (one evaluate.render_frame: the static forward under the alive mask), and the metrics of render
        against frame under the valid-depth mask (one evaluate.frame_metrics, no MS-SSIM) into row t of
        `arrival` [num_frames, 8] (evaluate.COLUMNS; NaN where nothing was reported: frame 0, the MS-SSIM
        column).  Nothing is read back.  The gains of the same record are view_gains'."""
        from . import evaluate as ev
        f = self.frames[t]
        im, ds = ev.render_frame(self.params, t, self.cam, self.w2c, self.alive, self.bin_capacity,
                                 self.arrival_status)
        ev.frame_metrics(im, ds, f["im"], f["depth"], self.sil_thres, self.arrival[t], self.arrival_workspace,
                         use_sil_mask=False, ms_ssim=False)

    def run(self, frames=None):
        """frame(t) for every t of `frames` (an iterable; default: the frames in the list that have not run)."""
        for t in (range(len(self.tracking_iters_run), len(self.frames)) if frames is None else frames):
            self.frame(t)

    def push(self, im: torch.Tensor, depth: torch.Tensor, w2c=None, densify_frame=None) -> int:
        """A frame that arrives (the realtime loop, scripts/splatam_realtime.py): appended to the frame list and
        run as frame t = len(frames) - 1, with its pose when `w2c` is given (frame()).  Needs num_frames: the
        pose tensors have that many columns, and a frame beyond them raises ValueError.  densify_frame
        {"im", "depth"}: the frame at the densification resolution, for a capture with densify_frames.
        Under densify_size / track_size the sequence makes the small frames itself (one gsr_resize_frame
        launch) and the caller pushes the full frame alone.  A capture with track_frames goes through
        push_frames.  Returns t.  Nothing is read back (but see track_cfg.use_depth_loss_thres)."""
        return self.push_frames(im, depth, w2c=w2c, densify_frame=densify_frame)

    def push_frames(self, im: torch.Tensor, depth: torch.Tensor, w2c=None, densify_frame=None, track_frame=None) -> int:
        """push() with the frame at the tracking resolution: track_frame {"im", "depth"}, for a capture with
        track_frames (one per frame, by the rule of densify_frame)."""
        t = self._append_frame(im, depth, densify_frame, track_frame)
        self.frame(t, w2c=w2c)
        return t

    def push_raw(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor, pose=None, w2c=None) -> int:
        """push() for the frame as the sensor delivers it (scripts/ros_handler.py:402-411): rgb_u8 [H,W,3] uint8,
        depth_u16 [H,W] uint16 in sensor units (png_depth_scale per metre; max_depth marks far readings -1) --
        splatam_amd.ingest.  One gsr_ingest_frame launch makes the float frame and, under track_size /
        densify_size, the small frames (no gsr_resize_frame launch for this frame); then push_frames'
        bookkeeping and frame(t, w2c=...).  pose: the odometry pose (x, y, z, qx, qy, qz, qw), made relative to
        the first pose pushed (ingest.odometry_w2c; host float64, a non-blocking copy to the device); w2c: as
        in push().  ValueError: both given, no png_depth_scale, or a capture with explicit track_frames /
        densify_frames (those callers own their small frames: push_frames).  Returns t.  Nothing is read back."""
        t, w2c = self._push_raw_frame(rgb_u8, depth_u16, pose, w2c)
        self.frame(t, w2c=w2c)
        return t

    def check(self):
        """One host synchronisation: raises if a binning capacity or the map capacity overflowed."""
        if self.tracker.overflowed() or self.mapper.overflowed() or bool(self.overflow.item()):
            raise RuntimeError("SlamSequence: a binning capacity or the map capacity was exceeded")
        st = [self.dstatus.cpu()] + ([self.arrival_status.cpu()] if self.arrival_report else [])
        if any(int(s[0]) > self.bin_capacity or int(s[1]) != 0 for s in st):
            raise RuntimeError("SlamSequence: the densification (or arrival) render overflowed its binning capacity")

    def evaluate(self, gt_w2c=None, eval_every: int = 1, ms_ssim: bool = True) -> dict:
        """The reference's end-of-run eval() (utils/eval_helpers.py:408-640) of the padded map as it stands
        against the capture: splatam_amd.evaluate.evaluate_sequence with the alive mask (one dual render and
        one row of device metrics per evaluated frame, nothing read back), then the one host read of
        evaluate.summarize.  gt_w2c ([num_frames, 4, 4] or a list): adds "ate_rmse", the estimated
        trajectory being the first frame's w2c and the pose columns of frames 1 .. (:556-575)."""
        from . import evaluate as ev
        status = torch.zeros(4, dtype=torch.int32, device=self.alive.device)
        table, times = ev.evaluate_sequence(self.params, self.frames, self.cam, self.w2c, sil_thres=self.sil_thres,
                                            eval_every=eval_every, use_sil_mask=False, ms_ssim=ms_ssim,
                                            alive=self.alive, bin_capacity=self.bin_capacity, status=status)
        ate = None
        if gt_w2c is not None:
            est = [self.w2c] + [pose_w2c(self.params, t) for t in range(1, len(self.frames))]
            ate = ev.ate_rmse(gt_w2c, est)
        out = ev.summarize(table, times, ate)
        st = status.cpu()
        if int(st[0]) > self.bin_capacity or int(st[1]) != 0:
            raise RuntimeError("SlamSequence.evaluate: a render overflowed its binning capacity")
        out["table"] = table
        return out

    def live_params(self) -> dict:
        """The live rows (slot order) of every per-Gaussian tensor, and the camera tensors."""
        keep = self.alive.bool()
        return {k: (v.detach()[keep] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == keep.shape[0] else v)
                for k, v in self.params.items()}

    # ---- view scoring on the padded map (scripts/ros_handler.py:251-359, 807-836; splatam_amd.fisher) ----

    scorer = None         # the cached ViewScorer (view_scorer)
    scorer_captures = 0   # how often its two graphs were built: once, plus once per ensure_headroom that grew

    def _retire_scorer(self):
        """The map is about to move to other buffers (_build): the cached scorer's graphs read the old ones.
        Its H_train_inv is kept by live row -- the new buffers hold the live rows first, in order -- and the
        next scoring call rebuilds the graphs.  (Called where the host already synchronises.)"""
        sc = self.scorer
        if sc is None or sc.stale:
            return
        sc.stale = True
        sc.carried = sc.gains.H_inv[self.alive.bool()].clone() if sc.fitted else None
        sc.sum = sc.gains = None

    def view_scorer(self, K: int = 16, n_monte: int | None = None, seed: int = 0):
        """The sequence's view scorer: fisher.SequenceFisher graphs (modes "sum" and "gains", K poses per
        launch) on self.params / self.alive / self.cam / self.bin_capacity, built once and cached -- every
        replay sees the map as it then stands, so frames that densify, prune and compact need no rebuild.
        n_monte: fit_visited's Monte-Carlo sample size (the reference's N_monte_carlo); its draws come from the
        scorer's own RandomState(seed), never from the sequence's stream.  Returns the ViewScorer."""
        from .fisher import H_EPS, SequenceFisher
        old = self.scorer
        sc = ViewScorer(int(K), n_monte, seed)
        mk = lambda mode: SequenceFisher(self.params, self.alive, self.cam, sc.K, mode, self.bin_capacity,  # noqa: E731
                                         self.sil_thres)
        sc.sum, sc.gains = mk("sum"), mk("gains")
        if old is not None and old.stale and (old.K, old.n_monte, old.seed) == (sc.K, sc.n_monte, sc.seed):
            sc.rng, sc.used = old.rng, old.used  # the same scorer on new buffers: its stream goes on
            if old.carried is not None:
                with torch.no_grad():
                    sc.gains.H_inv.copy_(torch.reciprocal(torch.zeros_like(sc.gains.H_inv) + H_EPS))
                    sc.gains.H_inv[:old.carried.shape[0]] = old.carried
                sc.fitted = True
        self.scorer = sc
        self.scorer_captures += 1
        return sc

    def _scorer(self):
        sc = self.scorer
        if sc is None:
            return self.view_scorer()
        return self.view_scorer(sc.K, sc.n_monte, sc.seed) if sc.stale else sc

    def visited_w2cs(self) -> list:
        """The poses of the frames run so far, relative to frame 0 ([4,4] device tensors; nothing read back):
        the identity for frame 0, pose_w2c of the estimated (or given) pose column for the others."""
        dev = self.alive.device
        return [torch.eye(4, device=dev) if t == 0 else pose_w2c(self.params, t)
                for t in range(len(self.tracking_iters_run))]

    def fit_visited(self, w2cs=None, n_monte: int | None = None, check: bool = False) -> torch.Tensor:
        """compute_H_visited_inv (scripts/ros_handler.py:807-829) on the map as it stands: H_train_inv =
        reciprocal(H_train + 0.1) over the padded rows [capacity + 1, 4] (a dead row's H_train is +0), H_train
        the sum of the visited poses' Hessians, K per graph launch.  w2cs None: visited_w2cs().  With n_monte
        (default: view_scorer's) and more poses than that, a sample without replacement
        (RandomState.choice, the reference's np.random.choice) from the scorer's own stream; `scorer.used`
        records each call's pose indices.  Nothing is read back unless `check` (raises on a binning overflow)."""
        from .fisher import H_EPS
        sc = self._scorer()
        w2cs = self.visited_w2cs() if w2cs is None else list(w2cs)
        n_monte = sc.n_monte if n_monte is None else int(n_monte)
        idx = list(range(len(w2cs)))
        if n_monte is not None and len(w2cs) > n_monte:
            idx = [int(i) for i in sc.rng.choice(len(w2cs), size=n_monte, replace=False)]
        sc.used.append(idx)
        H = None
        for c in range(0, len(idx), sc.K):
            h = sc.sum.hessian_sum([w2cs[i] for i in idx[c:c + sc.K]], check=check)
            if h is None:
                raise RuntimeError("SlamSequence.fit_visited: a pose overflowed the binning capacity")
            H = h.clone() if H is None else H + h
        with torch.no_grad():
            if H is None:
                H = torch.zeros_like(sc.gains.H_inv)
            torch.reciprocal(H + H_EPS, out=sc.gains.H_inv)
        sc.fitted = True
        return sc.gains.H_inv

    def view_gains(self, w2cs, check: bool = False, **weights) -> torch.Tensor:
        """send_gains' (g_sil, g_eig, gain) of every candidate pose against fit_visited's H_train_inv: float64
        [n,3] on the device, like FisherScorer.view_gains (weights: combine_gains').  K candidates per graph
        launch; nothing is read back unless `check` (raises on a binning overflow)."""
        sc = self._scorer()
        if not sc.fitted:
            raise RuntimeError("fit_visited() first (H_train_inv)")
        w2cs = list(w2cs)
        out = torch.zeros(len(w2cs), 3, dtype=torch.float64, device=self.alive.device)
        for c in range(0, len(w2cs), sc.K):
            g = sc.gains.gains(w2cs[c:c + sc.K], sc.gains.H_inv, check=check, **weights)
            if g is None:
                raise RuntimeError("SlamSequence.view_gains: a pose overflowed the binning capacity")
            out[c:c + g.shape[0]] = g
        return out


class ViewScorer:
    """What SlamSequence.view_scorer caches: the two SequenceFisher graphs (`sum`, `gains`; gains.H_inv holds
    H_train_inv once `fitted`), the Monte-Carlo settings with the scorer's own random stream, and `used`, the
    visited-pose indices of every fit_visited call.  `stale`: the map moved to other buffers; the graphs are
    rebuilt by the next scoring call (`carried`: H_train_inv's live rows until then)."""

    def __init__(self, K: int, n_monte, seed: int):
        self.K, self.n_monte, self.seed = K, (None if n_monte is None else int(n_monte)), seed
        self.rng = np.random.RandomState(seed)
        self.used = []
        self.sum = self.gains = None
        self.fitted, self.stale, self.carried = False, False, None


class PerFrameSlam(_SequenceBase):
    """The same frames in the form a shape-changing map forces on captured graphs: per frame a fresh
    GraphTracker on the frame's pose (probe, warm-up, capture), add_new_gaussians by torch.cat, a fresh
    GraphMapper on the grown map (probe, warm-up, capture) and, after its pruning, compact().  The comparison
    form for SlamSequence (tests/test_gpu_sequence.py; bench.py's sequence leg times both).  bin_capacity None:
    each tracker / mapper probes its own (what a per-frame loop must do); given: every one uses it."""

    def __init__(self, params: dict, frames: list, cam, w2c, intrinsics, tracking_iters: int = 40,
                 mapping_iters: int = 60, track_replay: int = 20, window: int = 8, keyframe_every: int = 5,
                 sil_thres: float = 0.5, track_cfg: TrackingConfig = TrackingConfig(),
                 map_cfg: MappingConfig = MappingConfig(), prune: bool | None = None, scene_radius=None,
                 bin_capacity: int | None = None, keyframe_policy: str = "window", overlap_pixels: int = 1600,
                 densify_mode: str = "torch", densify_frames=None, densify_cam=None, densify_intrinsics=None,
                 median_thr=None, median_scale: float = 50.0, num_frames: int | None = None, map_every: int = 1,
                 track_frames=None, track_cam=None, track_size=None, densify_size=None, png_depth_scale=None,
                 max_depth=None, arrival_report: bool = False):
        self._set_options(locals())
        self.arrival = {}  # arrival_report: per reported frame, evaluate_literal's row of the on-arrival render
        self.kf_list = []  # "overlap": the keyframes in the order appended, each with its est_w2c snapshot
        self.windows = []  # "overlap": per frame, the selected window's time indices
        self.p = {k: v.detach().clone() for k, v in params.items()}

    def frame(self, t: int, sequence, w2c=None):
        p = self.p
        ran = 0
        if t > 0 and w2c is not None:
            write_given_pose(p, t, w2c)
        elif t > 0:
            initialize_camera_pose(p, t)
            tp = dict(p)
            tp["cam_unnorm_rots"] = p["cam_unnorm_rots"][..., t:t + 1].clone().requires_grad_(True)
            tp["cam_trans"] = p["cam_trans"][..., t:t + 1].clone().requires_grad_(True)
            tracker = GraphTracker(tp, self._track_curr(t), 0, iters_per_graph=self.track_replay, cfg=self.track_cfg, warmup_iters=1,
                                   fuse_pose=True, capacity=self.bin_capacity,
                                   loss_terms=self.track_cfg.use_depth_loss_thres)
            ran = tracker.track_frame(self.tracking_iters, depth_loss_thres=self._depth_loss_thres())
            with torch.no_grad():
                p["cam_unnorm_rots"][..., t] = tp["cam_unnorm_rots"][..., 0]
                p["cam_trans"][..., t] = tp["cam_trans"][..., 0]
        if t > 0 and self.arrival_report:  # (SlamSequence.report_arrival's point, in plain renders and torch ops)
            from . import evaluate as ev
            f = self.frames[t]
            self.arrival[t] = ev.evaluate_literal(*ev.render_frame(p, t, self.cam, self.w2c), f["im"], f["depth"],
                                                  self.sil_thres, ms_ssim=False)
        if t > 0 and self._maps(t):
            kf, intr = self._densify_kf(t)
            add = add_new_gaussians_device if self.densify_mode == "device" else add_new_gaussians_literal
            p = add(p, kf, t, intr, self.sil_thres, self.median_thr, self.median_scale)
        self.tracking_iters_run.append(ran)
        if not self._maps(t):
            self._add_keyframe(t)
            return
        mp = {k: (v.detach().requires_grad_(True) if k in GAUSS_KEYS + ("rgb_colors",) else v) for k, v in p.items()}
        if self.keyframe_policy == "overlap":
            win, sequence = self._select_overlap(p, t, sequence)
        else:
            win = self._window(t)
        m = GraphMapper(mp, win, iters_per_graph=self.mapping_iters, cfg=self.map_cfg, seed=0, prune=self.prune,
                        scene_radius=self.scene_radius, capacity=self.bin_capacity)
        m.run(sequence=sequence)
        if m.prune_at:
            mp, _, _ = m.compact()
        self.p = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in mp.items()}
        self._add_keyframe(t)

    def push_raw(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor, sequence=None, pose=None, w2c=None) -> int:
        """SlamSequence.push_raw for this loop: the same intake (one gsr_ingest_frame launch, the bookkeeping,
        the pose), then frame(t, sequence, w2c=...) with the mapper's draws `sequence`.  Needs num_frames."""
        t, w2c = self._push_raw_frame(rgb_u8, depth_u16, pose, w2c)
        self.frame(t, sequence, w2c=w2c)
        return t

    def _add_keyframe(self, t: int):
        if not self._is_keyframe(t):
            return
        if self.keyframe_policy == "overlap":
            self.kf_list.append(dict(self._kf(t), est_w2c=pose_w2c(self.p, t)))
        else:
            self.keyframes.append(self._kf(t))

    def _select_overlap(self, p: dict, t: int, words):
        """keyframes.select_literal on the frame's random words (SlamSequence.draws[t]): the window's keyframe
        dicts and the per-iteration window indices, for the per-frame GraphMapper's host path."""
        dev = p["means3D"].device
        n_kf = len(self.kf_list)
        w = words_tensor(words, dev)
        S, n_cand, total = self._word_counts(n_kf)
        if w.numel() != total:
            raise ValueError(f"frame {t}: {total} random words")
        kf_w2c = torch.stack([kf["est_w2c"].reshape(16) for kf in self.kf_list]) if n_kf else \
            torch.zeros(0, 16, device=dev)
        kf_time = torch.tensor([kf["id"] for kf in self.kf_list], dtype=torch.int64, device=dev)
        sel = select_literal(self.frames[t]["depth"], self.intrinsics, pose_w2c(p, t), kf_w2c, n_kf, self.window - 2,
                             w[:S], w[S:S + n_cand], w[S + n_cand:], kf_time, t, n_kf)
        rows = sel["window"][:int(sel["n_window"])].tolist()
        self.windows.append([t if r == n_kf else self.kf_list[r]["id"] for r in rows])
        return [self._kf(t) if r == n_kf else self.kf_list[r] for r in rows], sel["draw_index"].tolist()
