"""A frame's copies at other resolutions: the tracking frame of SplaTAM-S (the reference's tracking_image_height /
width, scripts/splatam.py:517-523, 588-607, 680-687; configs/replica/splatam_s.py) and the densification frame
(densification_image_height / width), with the cameras and intrinsics that go with them.

The reference's dataset loader makes the small frames on the host (datasets/gradslam_datasets/basedataset.py:
224-257: cv2.resize, colour INTER_LINEAR, depth INTER_NEAREST) and scales the intrinsics
(datautils.scale_intrinsics, datautils.py:113-116).  Here

* resize_device is gsr_resize_frame (include/gsr_glue.h): one launch on the current stream for one or two
  output sizes, any ratio, nothing read back.
* resize_literal is the same contract in elementwise float32 torch ops on the tensors' own device (CPU
  included): the same bits.
* scale_intrinsics / resized_camera give the intrinsics and the rasterizer settings of the small frame.

Depth is nearest neighbour (a measured depth, never a blend), colour bilinear with half-pixel centres -- the
sample positions of cv2.INTER_LINEAR and of F.interpolate(mode="bilinear", align_corners=False) -- with the taps
and weights formed exactly from integers.  The deliberate difference from the reference: its loader resizes the
uint8 image (cv2's fixed-point weights, rounded to a byte) before the division by 255, this module resizes the
float image; parity with cv2's uint8 path is not pinned by any test.  densify.downscale_capture /
downscale_camera (integer factors, F.interpolate) stay as they are.
"""
from __future__ import annotations

import torch

from ._devcall import check_rc, require


def _size(size) -> tuple[int, int]:
    h, w = (int(v) for v in size)
    if h < 1 or w < 1:
        raise ValueError(f"resize: size {size!r} must be (h, w) >= 1")
    return h, w


def _frame_size(frame: dict) -> tuple[int, int]:
    im, depth = frame["im"], frame["depth"]
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if im.dim() != 3 or im.shape[0] != 3 or tuple(im.shape[-2:]) != (H, W) or depth.numel() != H * W:
        raise ValueError("resize: a frame is {'im' [3,H,W], 'depth' [1,H,W]}")
    return H, W


def empty_frame(size, device) -> dict:
    """An uninitialised {"im" [3,h,w], "depth" [1,h,w]} (float32) for resize_device's `out`."""
    h, w = _size(size)
    return {"im": torch.empty(3, h, w, dtype=torch.float32, device=device),
            "depth": torch.empty(1, h, w, dtype=torch.float32, device=device)}


def resize_device(frame: dict, size, size2=None, out=None):
    """gsr_resize_frame on the current stream: frame {"im" [3,H,W], "depth" [1,H,W]} (float32, contiguous, on a
    ROCm device) at size (h, w) -- and at size2 in the same launch.  out: the frame to write (with size2: a pair
    of frames), else new tensors.  Returns the small frame, or the pair with size2.  Nothing is read back."""
    from ._lib import lib
    im, depth = frame["im"], frame["depth"]
    if not depth.is_cuda:
        raise RuntimeError("resize_device: ROCm devices only (resize_literal is the host form)")
    H, W = _frame_size(frame)
    dev = depth.device
    sizes = [_size(size)] + ([] if size2 is None else [_size(size2)])
    if out is None:
        outs = [empty_frame(s, dev) for s in sizes]
    else:
        outs = [out] if size2 is None else list(out)
        if len(outs) != len(sizes):
            raise ValueError("resize_device: one `out` frame per size")
    checks = [("im", im, torch.float32, 3 * H * W), ("depth", depth, torch.float32, H * W)]
    for k, ((h, w), o) in enumerate(zip(sizes, outs)):
        checks += [(f"out{k} im", o["im"], torch.float32, 3 * h * w), (f"out{k} depth", o["depth"], torch.float32, h * w)]
    require("resize_device", dev, checks, exact=[c[0] for c in checks])
    args = []
    for k in range(2):
        args += [*sizes[k], outs[k]["im"].data_ptr(), outs[k]["depth"].data_ptr()] if k < len(sizes) else \
            [0, 0, None, None]
    check_rc(lib.gsr_resize_frame(H, W, im.data_ptr(), depth.data_ptr(), *args,
                                  torch.cuda.current_stream(dev).cuda_stream), "gsr_resize_frame")
    return outs[0] if size2 is None else (outs[0], outs[1])


def nearest_index(n_out: int, n_in: int, device=None) -> torch.Tensor:
    """The nearest-neighbour source index of every output sample: floor(i * n_in / n_out), in integers."""
    return (torch.arange(n_out, dtype=torch.int64, device=device) * n_in) // n_out


def linear_taps(n_out: int, n_in: int, device=None):
    """(i0, i1, t) of gsr_resize_frame's bilinear axis (include/gsr_glue.h): the two taps (int64) and the weight
    of the second (float32), from the quotient and remainder of ((2 i + 1) n_in - n_out) / (2 n_out)."""
    i = torch.arange(n_out, dtype=torch.int64, device=device)
    num = (2 * i + 1) * n_in - n_out
    den = 2 * n_out
    pos = num > 0
    i0 = torch.where(pos, num // den, torch.zeros_like(num))
    rem = torch.where(pos, num - i0 * den, torch.zeros_like(num))
    t = rem.to(torch.float32) / torch.tensor(float(den), dtype=torch.float32, device=device)
    return i0, torch.clamp(i0 + 1, max=n_in - 1), t


def _lerp(a: torch.Tensor, b: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """a where t == 0 (the other tap is not read into the result), else a + t * (b - a): each op rounded."""
    return torch.where(t == 0, a, a + t * (b - a))


def resize_literal(frame: dict, size) -> dict:
    """gsr_resize_frame's contract in elementwise float32 torch ops (gathers, one operation per rounding) on the
    frame's own device, CPU included: depth bitwise the source pixel, colour the stated operation order."""
    H, W = _frame_size(frame)
    h, w = _size(size)
    im, depth = frame["im"].to(torch.float32), frame["depth"]
    dev = depth.device
    with torch.no_grad():
        ny, nx = nearest_index(h, H, dev), nearest_index(w, W, dev)
        d = depth.reshape(H, W)[ny[:, None], nx[None, :]].reshape(1, h, w)
        x0, x1, tx = linear_taps(w, W, dev)
        y0, y1, ty = linear_taps(h, H, dev)
        tx, ty = tx[None, None, :], ty[None, :, None]
        top = _lerp(im[:, y0][:, :, x0], im[:, y0][:, :, x1], tx)
        bot = _lerp(im[:, y1][:, :, x0], im[:, y1][:, :, x1], tx)
        out = _lerp(top, bot, ty)
    return {"im": out.contiguous(), "depth": d.contiguous()}


def scale_intrinsics(intrinsics, H: int, W: int, h: int, w: int) -> tuple:
    """datautils.scale_intrinsics (datasets/gradslam_datasets/datautils.py:113-116) from an H x W image to an
    h x w one: fx and cx times w / W, fy and cy times h / H (Python floats, the ratio formed first)."""
    fx, fy, cx, cy = intrinsics
    rw, rh = w / W, h / H
    return fx * rw, fy * rh, cx * rw, cy * rh


def resized_camera(W: int, H: int, intrinsics, h: int, w: int, device, w2c=None):
    """camera_settings(setup_camera(...)) of a W x H camera with `intrinsics` (the full resolution's) resized to
    h x w: the rasterizer settings of the tracking render (scripts/splatam.py:588-607) or of the densification
    render, at any ratio.  At a ratio that is a power of two this is densify.downscale_camera bit for bit."""
    from .scenes import setup_camera
    from .slam import camera_settings
    h, w = _size((h, w))
    fx, fy, cx, cy = scale_intrinsics(intrinsics, H, W, h, w)
    return camera_settings(setup_camera(w, h, fx, fy, cx, cy, w2c=w2c), device)


def check_track_args(track_frames, track_cam, frames=None):
    """The loops' tracking-resolution arguments: given together or not at all, one frame per frame."""
    if (track_frames is None) != (track_cam is None):
        raise ValueError("track_frames and track_cam must be given together")
    if track_frames is not None and frames is not None and len(track_frames) != len(frames):
        raise ValueError("track_frames: one frame per frame of the capture")
