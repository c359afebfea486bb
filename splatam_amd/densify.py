"""SplaTAM's add_new_gaussians (scripts/splatam.py:384-426) for a SLAM sequence that never waits on the host,
at the frame's resolution or at a densification resolution of its own.

The reference selects the pixels the map does not explain (silhouette below the threshold, or rendered depth
behind the measured depth by more than 50x the median depth error), back-projects them and appends one
Gaussian each.  splatam_amd.sequence.densify_static restates that in about two dozen torch launches over every
pixel (a sorting median, an H*W cumsum, a point cloud of every pixel, index_put_ with H*W colliding writes to
a sink row).  Here

* densify_device is the whole step as one call (include/gsr_glue.h: gsr_densify_frame, six
  launches): the median by radix selection on the bit patterns, ranks from ballots and a scan of workgroup
  counts, only the selected pixels write rows.
* densify_literal is the comparison form: the same contract in elementwise torch ops with host
  synchronisations; it runs on CPU tensors too.
* median_thr / median_scale (the realtime loop's add_new_gaussians, scripts/splatam_realtime.py:430-482) send
  densify_device to gsr_densify_frame_capped; depth_threshold is that threshold in torch ops.
* init_frame_device is gsr_init_frame (the first frame's point cloud: every pixel with a measured depth, the last
  two of the six launches); init_literal its comparison form.
* downscale_capture / downscale_camera give the densification frames of the reference's
  `densification_image_height / width` configurations (scripts/splatam.py:191-215, 558-580, 801-812; the dataset
  loader's resize: nearest depth, bilinear colour, scaled intrinsics), for integer factors; splatam_amd.resize
  has the one-launch form for any ratio (gsr_resize_frame).

log_scales is the one output that is not pinned bitwise between the two forms (the device library's logf against
torch.log); everything else is.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ._devcall import backproject_literal, check_rc, f32, require, zero_workspace

ROW_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")


def workspace_bytes(H: int, W: int) -> int:
    from ._lib import lib
    return int(lib.gsr_densify_workspace_bytes(int(H), int(W)))


def make_workspace(H: int, W: int, device) -> torch.Tensor:
    """A zero-filled workspace for densify_device (any smaller image can share it)."""
    return zero_workspace(workspace_bytes(H, W), device)


def mean_focal(fx: float, fy: float) -> np.float32:
    """(fx + fy) / 2 as gsr_densify_frame forms it: in double from the two float32 values, rounded once."""
    return np.float32((float(np.float32(fx)) + float(np.float32(fy))) / 2.0)


def default_threshold(median_thr, median_scale) -> bool:
    """Whether (median_thr, median_scale) are add_new_gaussians' defaults: gsr_densify_frame's 50 x the median."""
    return median_thr is None and float(median_scale) == 50.0


def _map_call(where: str, params: dict, alive, n_live, overflow, curr: dict, w2c_dev, capacity: int, workspace,
              dest, depth_sil=None):
    """The checks densify_device and init_frame_device share, and the arguments both entries end with:
    (H, W, rows..., alive, n_live, overflow, n_added, dest, workspace, stream) as data pointers, and n_added."""
    im, depth = curr["im"], curr["depth"]
    lead = depth if depth_sil is None else depth_sil
    if not lead.is_cuda:
        raise RuntimeError(f"{where}: ROCm devices only (the *_literal functions are the host forms)")
    H, W = int(lead.shape[-2]), int(lead.shape[-1])
    dev, capacity = lead.device, int(capacity)
    rows = [(k, params[k].detach(), torch.float32, (capacity + 1) * c)
            for k, c in zip(ROW_KEYS, (3, 3, 4, 1, 1))]
    checks = [("im", im, torch.float32, 3 * H * W), ("depth", depth, torch.float32, H * W),
              ("w2c", w2c_dev, torch.float32, 16), *rows, ("alive", alive, torch.uint8, capacity + 1),
              ("n_live", n_live, torch.int64, 1)]
    if depth_sil is not None:
        checks.append(("depth_sil", depth_sil, torch.float32, 3 * H * W))
    if dest is not None:
        checks.append(("dest", dest, torch.int32, H * W))
    require(where, dev, checks)
    if overflow.device != dev or overflow.element_size() != 1 or overflow.numel() < 1:
        raise RuntimeError(f"{where}: overflow must be a one-byte tensor on the map's device")
    if im.shape[-2:] != lead.shape[-2:] or depth.shape[-2:] != lead.shape[-2:]:
        raise RuntimeError(f"{where}: the frame and the silhouette render differ in size")
    if workspace.device != dev or workspace.numel() * workspace.element_size() < max(workspace_bytes(H, W), 1):
        raise RuntimeError(f"{where}: workspace too small (make_workspace(H, W))")
    n_added = torch.empty(1, dtype=torch.int64, device=dev)
    tail = (capacity, *(t.data_ptr() for _, t, _, _ in rows), alive.data_ptr(), n_live.data_ptr(),
            overflow.data_ptr(), n_added.data_ptr(), None if dest is None else dest.data_ptr(),
            workspace.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return H, W, tail, n_added


def densify_device(params: dict, alive: torch.Tensor, n_live: torch.Tensor, overflow: torch.Tensor, curr: dict,
                   w2c_dev: torch.Tensor, intrinsics, sil_thres: float, capacity: int, depth_sil: torch.Tensor,
                   workspace: torch.Tensor, dest: torch.Tensor | None = None, median_thr=None,
                   median_scale: float = 50.0) -> torch.Tensor:
    """gsr_densify_frame on the current stream: no host read.  params: the capacity-padded map ([capacity + 1]
    rows; written in place), alive uint8 [capacity + 1], n_live int64 [1], overflow bool / uint8 [1]; curr
    {"im" [3,H,W], "depth" [1,H,W]}; w2c_dev [4,4] (keyframes.pose_w2c); depth_sil [3,H,W] the silhouette render;
    workspace: make_workspace(H, W); dest: int32 [H*W] or None.  median_thr / median_scale: the realtime loop's
    threshold (scripts/splatam_realtime.py:444-453); other than (None, 50) they go to gsr_densify_frame_capped.
    Returns n_added (int64 [1], device)."""
    from ._lib import lib
    H, W, tail, n_added = _map_call("densify_device", params, alive, n_live, overflow, curr, w2c_dev, capacity,
                                    workspace, dest, depth_sil)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    head = (H, W, depth_sil.data_ptr(), curr["im"].data_ptr(), curr["depth"].data_ptr(), fx, fy, cx, cy,
            w2c_dev.data_ptr(), float(sil_thres))
    if default_threshold(median_thr, median_scale):
        check_rc(lib.gsr_densify_frame(*head, *tail), "gsr_densify_frame")
    else:
        check_rc(lib.gsr_densify_frame_capped(*head, *tail, int(median_thr is not None), float(median_thr or 0.0),
                                              float(median_scale)), "gsr_densify_frame_capped")
    return n_added


def init_frame_device(params: dict, alive: torch.Tensor, n_live: torch.Tensor, overflow: torch.Tensor, curr: dict,
                      w2c_dev: torch.Tensor, intrinsics, capacity: int, workspace: torch.Tensor,
                      dest: torch.Tensor | None = None) -> torch.Tensor:
    """gsr_init_frame on the current stream: every pixel of curr with a measured depth appended to the padded map
    (densify_device's tensors, without a silhouette render).  Returns n_added (int64 [1], device)."""
    from ._lib import lib
    H, W, tail, n_added = _map_call("init_frame_device", params, alive, n_live, overflow, curr, w2c_dev, capacity,
                                    workspace, dest)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    check_rc(lib.gsr_init_frame(H, W, curr["im"].data_ptr(), curr["depth"].data_ptr(), fx, fy, cx, cy,
                                w2c_dev.data_ptr(), *tail), "gsr_init_frame")
    return n_added


def depth_threshold(med: torch.Tensor, median_thr=None, median_scale: float = 50.0) -> torch.Tensor:
    """Step 3's thr of gsr_densify_frame_capped (include/gsr_glue.h) from the median (a float32 scalar tensor),
    on the median's device without a host read (the reference branches on `depth_error.median() > median_thr`
    on the host; a NaN median fails the comparison here as there)."""
    dev = med.device
    if median_thr is None:
        return f32(median_scale, dev) * med
    # capped: the product of the two (float32-valued) Python floats, rounded once; else 50 x the median, whatever
    # median_scale is (the reference resets the scale to 50 on that branch: scripts/splatam_realtime.py:450-451)
    capped = f32(float(np.float32(median_scale)) * float(np.float32(median_thr)), dev)
    return torch.where(med > f32(median_thr, dev), capped, f32(50.0, dev) * med)


def _selected_rows(im, gt, mask, w2c, intrinsics) -> tuple[dict, int]:
    """Steps 4-5 of gsr_densify_frame for the pixels of `mask` [H,W], in row-major order (host synchronisation)."""
    dev = gt.device
    fx, fy, cx, cy = (f32(v, dev) for v in intrinsics)
    f = f32(mean_focal(intrinsics[0], intrinsics[1]), dev)
    rowi, coli = torch.nonzero(mask, as_tuple=True)
    z = gt[rowi, coli]
    pw = backproject_literal(coli, rowi, z, fx, fy, cx, cy, w2c)
    q = z / f
    n = int(z.numel())
    rot = torch.zeros(n, 4, dtype=torch.float32, device=dev)
    rot[:, 0] = 1.0
    rows = {"means3D": torch.stack(pw, dim=-1).reshape(n, 3), "rgb_colors": im[:, rowi, coli].T.contiguous(),
            "unnorm_rotations": rot, "logit_opacities": torch.zeros(n, 1, dtype=torch.float32, device=dev),
            "log_scales": torch.log(torch.sqrt(q * q)).reshape(n, 1)}
    return rows, n


def densify_literal(curr: dict, w2c: torch.Tensor, intrinsics, sil_thres: float, depth_sil: torch.Tensor,
                    median_thr=None, median_scale: float = 50.0):
    """gsr_densify_frame's contract (include/gsr_glue.h; with median_thr / median_scale other than (None, 50),
    gsr_densify_frame_capped's) in elementwise float32 torch ops on the tensors' own
    device (CPU included), with host synchronisations (torch.median, boolean masks) and no GEMM: each
    operation forms the stated rounding, so the kernels form the same bits (log_scales up to logf).
    Returns (rows, mask, count): the appended rows' values in row-major pixel order (a dict over ROW_KEYS),
    the selection mask [H*W] (bool) and the number selected -- the caller places rows[: capacity - n_live] at
    n_live."""
    im, gt = curr["im"], curr["depth"][0]
    dev = gt.device
    with torch.no_grad():
        rd, sil = depth_sil[0], depth_sil[1]
        valid = gt > 0
        err = torch.abs(gt - rd) * valid.to(torch.float32)
        med = err.reshape(-1).median()  # the lower median; NaN if any err is NaN
        thr = depth_threshold(med, median_thr, median_scale)
        mask = ((sil < f32(sil_thres, dev)) | ((rd > gt) & (err > thr))) & valid
        rows, n = _selected_rows(im, gt, mask, w2c, intrinsics)
    return rows, mask.reshape(-1), n


def init_literal(curr: dict, w2c: torch.Tensor, intrinsics):
    """gsr_init_frame's contract in densify_literal's terms: every pixel with a measured depth selected.
    Returns (rows, mask, count)."""
    im, gt = curr["im"], curr["depth"][0]
    with torch.no_grad():
        mask = gt > 0
        rows, n = _selected_rows(im, gt, mask, w2c, intrinsics)
    return rows, mask.reshape(-1), n


def downscale_capture(frames: list, intrinsics, factor: int):
    """The densification frames of a capture at 1 / factor of its resolution, as the reference's dataset
    loader resizes a `densification_image_height / width` copy: depth by nearest neighbour, colour bilinear
    (F.interpolate, align_corners False), the intrinsics divided by the factor.  Returns (frames, intrinsics)."""
    factor = int(factor)
    if factor < 1:
        raise ValueError("downscale_capture: factor >= 1")
    out = []
    for fr in frames:
        H, W = int(fr["depth"].shape[-2]), int(fr["depth"].shape[-1])
        if H % factor or W % factor:
            raise ValueError(f"downscale_capture: {H}x{W} is not a multiple of {factor}")
        size = (H // factor, W // factor)
        with torch.no_grad():
            im = F.interpolate(fr["im"][None], size=size, mode="bilinear", align_corners=False)[0]
            depth = F.interpolate(fr["depth"][None], size=size, mode="nearest")[0]
        out.append({"im": im.contiguous(), "depth": depth.contiguous()})
    fx, fy, cx, cy = intrinsics
    return out, (fx / factor, fy / factor, cx / factor, cy / factor)


def downscale_camera(W: int, H: int, intrinsics, factor: int, device, w2c=None):
    """camera_settings(setup_camera(...)) at 1 / factor of a W x H camera with `intrinsics` (those of the full
    resolution): the rasterizer settings of the densification render (scripts/splatam.py:558-580)."""
    from .scenes import setup_camera
    from .slam import camera_settings
    fx, fy, cx, cy = intrinsics
    factor = int(factor)
    if factor < 1 or W % factor or H % factor:
        raise ValueError(f"downscale_camera: {H}x{W} is not a multiple of {factor}")
    return camera_settings(setup_camera(W // factor, H // factor, fx / factor, fy / factor, cx / factor, cy / factor,
                                        w2c=w2c), device)


def check_densify_args(densify_mode: str, densify_frames, densify_cam, densify_intrinsics, frames=None):
    if densify_mode not in ("torch", "device"):
        raise ValueError(f"densify_mode {densify_mode!r}: 'torch' or 'device'")
    given = [a is not None for a in (densify_frames, densify_cam, densify_intrinsics)]
    if any(given) and not all(given):
        raise ValueError("densify_frames, densify_cam and densify_intrinsics must be given together")
    if all(given) and frames is not None and len(densify_frames) != len(frames):
        raise ValueError("densify_frames: one frame per frame of the capture")
