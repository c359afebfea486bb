"""The per-frame steps of SplaTAM's loop (scripts/splatam.py:697-929) restated on a parameter dict, with no
sequence state: the constant-velocity pose initialisation (initialize_camera_pose, :429-448), a given pose
(write_given_pose), and add_new_gaussians (:384-426) in its parts -- the depth / silhouette render, the pixel
selection, the new Gaussian of every pixel -- and whole, on an unpadded map (by torch.cat: the reference's
reallocation; or through the padded map's kernel).  splatam_amd.padded_map.densify_static is the same step on a
capacity-padded map; SlamSequence and PerFrameSlam (splatam_amd.sequence, splatam_amd.perframe) call these.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .densify import ROW_KEYS, default_threshold, densify_device, depth_threshold
from .densify import make_workspace as make_densify_workspace
from .keyframes import pose_w2c
from .slam import matrix_to_quaternion, transform_to_frame, transformed_params2depthplussilhouette


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


def write_given_pose(params: dict, t: int, w2c: torch.Tensor):
    """A frame whose pose is known (tracking.use_gt_poses, scripts/splatam_realtime.py:812-821): w2c [4,4], the
    pose relative to frame 0, into column t -- matrix_to_quaternion of its rotation and its translation.
    Device tensor ops only."""
    with torch.no_grad():
        params["cam_unnorm_rots"][..., t] = matrix_to_quaternion(w2c[:3, :3].unsqueeze(0).detach())
        params["cam_trans"][..., t] = w2c[:3, 3].detach()


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
        w2c = pose_w2c(params, t)
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
    from .padded_map import pad_map  # (padded_map.densify_static calls this module's parts)
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
