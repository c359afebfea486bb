"""A raw sensor frame into the frame SlamSequence.push() takes: what the reference's intake does op by op on
arrival (scripts/ros_handler.py:402-411, 434-435; datasets/gradslam_datasets/basedataset.py:250-257, 312-316)
-- an interleaved uint8 [H,W,3] image, a uint16 [H,W] depth image in sensor units and an odometry pose as
position plus quaternion become float32 [3,H,W] colour in [0, 1], float32 [1,H,W] depth in metres (far readings
marked -1) and the [4,4] pose relative to frame 0.

* ingest_device is gsr_ingest_frame (include/gsr_glue.h): one launch on the current stream for the float frame
  and, in the same launch, its copies at up to two other sizes (the tracking and the densification frame);
  nothing read back.
* ingest_literal is the same contract in plain ops on the tensors' own device (CPU included): the same bits.
* odometry_w2c turns (x, y, z, qx, qy, qz, qw) into the pose relative to the first one, on the host.

The contract's three roundings (include/gsr_glue.h):
  colour   (float)byte / 255.0f, one correctly rounded float32 division: the 256-entry table
           np.float32(i) / np.float32(255).  torch's CPU `x / 255` forms the same bits; torch's DEVICE `x / 255`
           multiplies by the rounded reciprocal and may differ by one ulp for some bytes -- which is why the
           literal form gathers from the table on every device.
  depth    (float)((double)u / png_depth_scale): numpy's float64 quotient rounded to float32 once.  A true
           float32 division by a float32 scale forms the same bits (the second rounding is innocuous); a
           float32 multiply by the reciprocal, torch's device `/ scale`, does not (249 of the 65,536 readings
           differ at scale 6553.5).  max_depth (the reference's 9.5): d >= max_depth becomes -1.  0 stays 0.
  small    resize's rule (splatam_amd.resize) applied to the float frame: gsr_ingest_frame forms the same bits
           from the bytes.
"""
from __future__ import annotations

import numpy as np
import torch

from ._devcall import check_rc, require
from .resize import _size, empty_frame, resize_literal

COLOUR_TABLE = np.arange(256, dtype=np.float32) / np.float32(255)  # the colour rule, stated once


def _raw_size(rgb_u8: torch.Tensor, depth_u16: torch.Tensor) -> tuple[int, int]:
    if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or depth_u16.dim() != 2 or \
            tuple(depth_u16.shape) != tuple(rgb_u8.shape[:2]):
        raise ValueError("ingest: a raw frame is rgb_u8 [H,W,3] and depth_u16 [H,W]")
    return int(depth_u16.shape[0]), int(depth_u16.shape[1])


def _depth_dtype(depth_u16: torch.Tensor):
    if depth_u16.dtype not in (torch.uint16, torch.int16):
        raise RuntimeError("ingest: depth_u16 must be torch.uint16 (or an int16 view of the same bytes)")
    return depth_u16.dtype


def _scale(png_depth_scale) -> float:
    s = float(png_depth_scale)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"ingest: png_depth_scale {png_depth_scale!r} must be finite and > 0")
    return s


def ingest_device(rgb_u8: torch.Tensor, depth_u16: torch.Tensor, png_depth_scale, max_depth=None, size=None,
                  size2=None, out=None, full: bool = True):
    """gsr_ingest_frame on the current stream: rgb_u8 [H,W,3] (uint8) and depth_u16 [H,W] (torch.uint16; an int16
    tensor is taken as a view of the same bytes, reinterpreted -- both are accepted, for torch builds and callers
    without uint16 device tensors), contiguous, on a ROCm device, at any byte / 2-byte address (slices of a
    larger buffer are fine).  png_depth_scale: sensor units per metre; max_depth: None, or the reading from which
    a depth becomes -1.  size / size2 (h, w): the small frames made in the same launch (size2 needs size);
    full=False: no full-size frame, small frames only.  out: the frame(s) to write, in the order returned, else
    new tensors.  Returns the full frame {"im" [3,H,W], "depth" [1,H,W]}; with sizes a tuple (full, small[,
    small2]); with full=False the small frame, or the pair with size2.  Nothing is read back."""
    from ._lib import lib
    if not depth_u16.is_cuda:
        raise RuntimeError("ingest_device: ROCm devices only (ingest_literal is the host form)")
    H, W = _raw_size(rgb_u8, depth_u16)
    dev = depth_u16.device
    if size is None and size2 is not None:
        raise ValueError("ingest_device: size2 needs size")
    sizes = [_size(s) for s in (size, size2) if s is not None]
    if not full and not sizes:
        raise ValueError("ingest_device: full=False needs a size")
    shapes = ([(H, W)] if full else []) + sizes
    if out is None:
        outs = [empty_frame(s, dev) for s in shapes]
    else:
        outs = [out] if isinstance(out, dict) else list(out)
        if len(outs) != len(shapes):
            raise ValueError("ingest_device: one `out` frame per frame returned")
    checks = [("rgb_u8", rgb_u8, torch.uint8, 3 * H * W), ("depth_u16", depth_u16, _depth_dtype(depth_u16), H * W)]
    for k, ((h, w), o) in enumerate(zip(shapes, outs)):
        checks += [(f"out{k} im", o["im"], torch.float32, 3 * h * w), (f"out{k} depth", o["depth"], torch.float32, h * w)]
    require("ingest_device", dev, checks, exact=[c[0] for c in checks])
    smalls = outs[1:] if full else outs
    args = [outs[0]["im"].data_ptr(), outs[0]["depth"].data_ptr()] if full else [None, None]
    for k in range(2):
        args += [*sizes[k], smalls[k]["im"].data_ptr(), smalls[k]["depth"].data_ptr()] if k < len(sizes) else \
            [0, 0, None, None]
    check_rc(lib.gsr_ingest_frame(H, W, rgb_u8.data_ptr(), depth_u16.data_ptr(), _scale(png_depth_scale),
                                  int(max_depth is not None), float(0.0 if max_depth is None else max_depth), *args,
                                  torch.cuda.current_stream(dev).cuda_stream), "gsr_ingest_frame")
    return outs[0] if len(outs) == 1 else tuple(outs)


def ingest_literal(rgb_u8: torch.Tensor, depth_u16: torch.Tensor, png_depth_scale, max_depth=None, size=None,
                   size2=None):
    """gsr_ingest_frame's contract in plain ops on the tensors' own device, CPU included: the colour gathered from
    the 256-entry table np.float32(i) / np.float32(255) (so device and CPU agree: torch's device `/ 255` is a
    multiply by the reciprocal), the depth (u.double() / scale).float(), max_depth's -1, and resize_literal for
    size / size2.  Returns ingest_device's full-frame forms."""
    H, W = _raw_size(rgb_u8, depth_u16)
    if rgb_u8.dtype != torch.uint8:
        raise RuntimeError("ingest: rgb_u8 must be torch.uint8")
    _depth_dtype(depth_u16)
    if size is None and size2 is not None:
        raise ValueError("ingest_literal: size2 needs size")
    dev = depth_u16.device
    with torch.no_grad():
        table = torch.from_numpy(COLOUR_TABLE).to(dev)
        im = table[rgb_u8.to(torch.int64)].permute(2, 0, 1).contiguous()
        # the 16 bits as an unsigned reading, whichever integer type carries them
        u = depth_u16.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        d = (u.to(torch.float64) / torch.tensor(_scale(png_depth_scale), dtype=torch.float64, device=dev)).to(torch.float32)
        if max_depth is not None:
            thr = torch.tensor(float(max_depth), dtype=torch.float32, device=dev)
            d = torch.where(d >= thr, torch.full_like(d, -1.0), d)
        frame = {"im": im, "depth": d.reshape(1, H, W).contiguous()}
    smalls = [resize_literal(frame, s) for s in (size, size2) if s is not None]
    return frame if not smalls else (frame, *smalls)


def pose_matrix(pose) -> np.ndarray:
    """pose_matrix_from_quaternion (scripts/ros_handler.py:515-520) without scipy: (x, y, z, qx, qy, qz, qw) as
    the float64 [4,4] camera-to-world matrix; the quaternion is normalised, as Rotation.from_quat does."""
    p = np.asarray(pose, dtype=np.float64).reshape(-1)
    if p.shape != (7,):
        raise ValueError("pose: (x, y, z, qx, qy, qz, qw)")
    q = p[3:]
    n = np.sqrt(np.dot(q, q))
    if not (np.isfinite(n) and n > 0):
        raise ValueError("pose: a zero or non-finite quaternion")
    x, y, z, w = q / n
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = p[:3]
    return m


def odometry_w2c(initial_pose, pose, device=None) -> torch.Tensor:
    """The [4,4] float32 pose relative to frame 0 that push(w2c=...) takes, from two odometry poses
    (x, y, z, qx, qy, qz, qw) as scripts/ros_handler.py:202 builds them: pose_matrix of each,
    relative_transformation(initial, pose) = inverse(initial) @ pose (geometryutils.py:413, the general inverse),
    then its inverse (ros_handler.py:438).  Host work in float64 numpy.  device: the result goes there by a
    non-blocking copy through a pinned buffer (nothing is read back, the host does not wait)."""
    rel = np.linalg.inv(pose_matrix(initial_pose)) @ pose_matrix(pose)
    out = torch.from_numpy(np.linalg.inv(rel).astype(np.float32))
    if device is None or torch.device(device).type == "cpu":
        return out
    return out.pin_memory().to(device, non_blocking=True)
