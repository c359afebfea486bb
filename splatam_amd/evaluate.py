"""SplaTAM's end-of-run evaluation (utils/eval_helpers.py:408-640, eval()) for a map and a capture, without a
host read per frame.

The reference renders every evaluated frame twice, forms PSNR, MS-SSIM, LPIPS and the two depth errors with a
dozen torch ops, moves the images to the CPU for pytorch_msssim and reads every metric back (`.cpu()`) as it
goes; the trajectory's ATE follows at the end.  Here

* frame_metrics is one ctypes call (include/gsr_glue.h: gsr_eval_frame; one launch, six with MS-SSIM) that
  writes a frame's metrics into one row of a device table,
* evaluate_sequence renders each evaluated frame once (the dual render: colour plus depth / silhouette, with
  the alive mask on a capacity-padded map) and fills the table; nothing is read back,
* summarize does the one host read and names the columns as the reference names its files (psnr, ssim, rmse,
  l1),
* ate_rmse is evaluate_ate / align (eval_helpers.py:23-77) on N x 3 points: end-of-run host work,
* evaluate_literal / ms_ssim_literal are the comparison form and the fallback: the reference's arithmetic in
  plain torch ops on already-rendered images, CPU tensors included (the role keyframes.select_literal plays).

Differences from eval(), all deliberate:
* no LPIPS: it needs torchmetrics' AlexNet weights, which this project does not ship;
* MS-SSIM is restated from pytorch_msssim's published definition (include/gsr_glue.h states it), not imported:
  the package is not a dependency, and parity with it is not pinned by a test;
* the metrics are formed on the device (float32 per-pixel operations, sums accumulated in float64 in a fixed
  order) where the reference moves the images to the CPU for MS-SSIM and sums in float32;
* no plots, image dumps or wandb.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ._devcall import check_rc, require, zero_workspace
from .keyframes import pose_w2c
from .slam import transform_to_frame, transformed_params2depthplussilhouette, transformed_params2rendervar

COLUMNS = ("psnr", "ms_ssim", "depth_rmse", "depth_l1", "n_valid", "mse_r", "mse_g", "mse_b")
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MIN_SIDE = 160  # the definition needs min(H, W) > (11 - 1) * 2^4


# ------------------------------------------------------------------ device form

def workspace_bytes(H: int, W: int, ms_ssim: bool = True) -> int:
    from ._lib import lib
    return int(lib.gsr_eval_workspace_bytes(int(H), int(W), int(bool(ms_ssim))))


def make_workspace(H: int, W: int, device, ms_ssim: bool = True) -> torch.Tensor:
    """A zero-filled workspace for frame_metrics (one of the largest size serves any sizes on one stream)."""
    n = workspace_bytes(H, W, ms_ssim)
    if n == 0:
        raise RuntimeError(f"make_workspace: {H}x{W} with ms_ssim={bool(ms_ssim)} is not a size gsr_eval_frame takes "
                           f"(MS-SSIM needs min(H, W) > {MS_SSIM_MIN_SIDE})")
    return zero_workspace(n, device)


def frame_metrics(im: torch.Tensor, depth_sil: torch.Tensor, gt_im: torch.Tensor, gt_depth: torch.Tensor,
                  sil_thres: float, row: torch.Tensor, workspace: torch.Tensor, use_sil_mask: bool = False,
                  ms_ssim: bool = True) -> torch.Tensor:
    """gsr_eval_frame on the current stream: no host read, the 8 metrics (COLUMNS) written into `row` (a
    contiguous float32 view of >= 8 elements, e.g. a row of the table).  im, gt_im, depth_sil [3, H, W];
    gt_depth [1, H, W] or [H, W]; workspace: make_workspace(H, W) (zero-filled once)."""
    from ._lib import lib
    if not im.is_cuda:
        raise RuntimeError("frame_metrics: ROCm devices only (evaluate_literal is the host form)")
    if im.dim() != 3 or im.shape[0] != 3:
        raise RuntimeError("frame_metrics: im must be [3, H, W]")
    H, W = int(im.shape[1]), int(im.shape[2])
    dev = im.device
    f32 = torch.float32
    require("frame_metrics", dev, (("im", im, f32, 3 * H * W), ("depth_sil", depth_sil, f32, 3 * H * W),
                                   ("gt_im", gt_im, f32, 3 * H * W), ("gt_depth", gt_depth, f32, H * W),
                                   ("row", row, f32, 8)),
            exact=("im", "depth_sil", "gt_im", "gt_depth"), size="float32 tensor of {n}")
    need = workspace_bytes(H, W, ms_ssim)  # (0: a size the library refuses; its message is the error)
    if workspace.device != dev or not workspace.is_contiguous() or \
            workspace.numel() * workspace.element_size() < need:
        raise RuntimeError("frame_metrics: workspace too small (make_workspace(H, W, device, ms_ssim))")
    rc = lib.gsr_eval_frame(H, W, im.data_ptr(), depth_sil.data_ptr(), gt_im.data_ptr(), gt_depth.data_ptr(),
                            float(sil_thres), int(bool(use_sil_mask)), int(bool(ms_ssim)), workspace.data_ptr(),
                            row.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    check_rc(rc, "gsr_eval_frame")
    return row


def eval_times(num_frames: int, eval_every: int = 1) -> list:
    """The time indices eval() evaluates (:449): frame 0 and every eval_every-th frame."""
    return [t for t in range(int(num_frames)) if t == 0 or (t + 1) % int(eval_every) == 0]


def render_frame(params: dict, t: int, cam, w2c, alive=None, bin_capacity: int = 0, status=None):
    """eval()'s two renders of pose column t (:453-476) as one dual render: (im [3,H,W], depth_sil [3,H,W]).
    bin_capacity > 0: the static forward (no host synchronisation; `status` receives its counters), with the
    alive mask of a capacity-padded map."""
    from .rasterizer import rasterize_gaussians_dual
    with torch.no_grad():
        tg = transform_to_frame(params, t, gaussians_grad=False, camera_grad=False)
        rv = transformed_params2rendervar(params, tg)
        c2 = transformed_params2depthplussilhouette(params, w2c, tg)["colors_precomp"]
        sh = params["shs"].detach() if "shs" in params else None
        col = None if sh is not None else rv["colors_precomp"].detach()
        im, ds, _, _ = rasterize_gaussians_dual(rv["means3D"], torch.zeros_like(rv["means3D"]), sh, col, c2,
                                                rv["opacities"].detach(), rv["scales"].detach(),
                                                rv["rotations"], None, cam, int(bin_capacity), status, alive=alive)
    return im, ds


def evaluate_sequence(params: dict, frames: list, cam, w2c, sil_thres: float = 0.5, eval_every: int = 1,
                      use_sil_mask: bool = False, ms_ssim: bool = True, alive=None, bin_capacity: int = 0,
                      status=None, table=None):
    """eval()'s per-frame loop (:431-514) on the stream: for frame 0 and every eval_every-th frame of `frames`
    ({"im", "depth"} each), transform_to_frame, one dual render and frame_metrics into that frame's row.
    Returns (table [n_evaluated, 8] float32 on the device, COLUMNS; the evaluated time indices).  No host read
    inside when bin_capacity > 0 (the static forward; check `status`, device int32 [4], afterwards like any
    static render); alive: the mask of a capacity-padded map (needs bin_capacity > 0).  use_sil_mask: the
    reference's `mapping_iters == 0 and not add_new_gaussians`."""
    times = eval_times(len(frames), eval_every)
    dev = params["means3D"].device
    f0 = frames[0]
    H, W = int(f0["im"].shape[-2]), int(f0["im"].shape[-1])
    if table is None:
        table = torch.full((len(times), 8), float("nan"), dtype=torch.float32, device=dev)
    if table.shape != (len(times), 8) or table.dtype != torch.float32 or not table.is_contiguous():
        raise RuntimeError(f"evaluate_sequence: table must be a contiguous float32 [{len(times)}, 8] tensor")
    if bin_capacity > 0 and status is None:
        status = torch.zeros(4, dtype=torch.int32, device=dev)
    ws = make_workspace(H, W, dev, ms_ssim)
    for i, t in enumerate(times):
        im, ds = render_frame(params, t, cam, w2c, alive, bin_capacity, status)
        frame_metrics(im, ds, frames[t]["im"], frames[t]["depth"], sil_thres, table[i], ws, use_sil_mask, ms_ssim)
    return table, times


def summarize(table: torch.Tensor, times=None, ate=None) -> dict:
    """The one host read: the table's columns as numpy arrays under the reference's names (psnr.txt, ssim.txt,
    rmse.txt, l1.txt -> "psnr", "ssim", "rmse", "l1"; "rmse" is the reference's per-pixel sqrt(x^2), a mean
    absolute error like "l1") and their means ("avg_psnr", ... as eval() prints them), plus "n_valid", "mse"
    [n, 3], "times" and "ate_rmse" when given.  No "lpips": it needs AlexNet weights this project does not
    ship."""
    a = table.detach().cpu().numpy()
    out = {"psnr": a[:, 0], "ssim": a[:, 1], "rmse": a[:, 2], "l1": a[:, 3], "n_valid": a[:, 4], "mse": a[:, 5:8]}
    for k in ("psnr", "ssim", "rmse", "l1"):
        out["avg_" + k] = float(out[k].mean()) if len(a) else float("nan")
    if times is not None:
        out["times"] = list(times)
    if ate is not None:
        out["ate_rmse"] = float(ate)
    return out


# ------------------------------------------------------------------ trajectory

def poses_w2c(cam_unnorm_rots: torch.Tensor, cam_trans: torch.Tensor) -> torch.Tensor:
    """[N, 4, 4] world-to-camera matrices of pose tensors [1, 4, N] / [1, 3, N] (eval():565-569)."""
    p = {"cam_unnorm_rots": cam_unnorm_rots, "cam_trans": cam_trans}
    return torch.stack([pose_w2c(p, t) for t in range(cam_unnorm_rots.shape[-1])])


def _points(w2c_list) -> np.ndarray:
    m = [(p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)) for p in w2c_list]
    return np.stack(m).astype(np.float64)


def ate_rmse(gt_w2c, est_w2c) -> float:
    """evaluate_ate / align (eval_helpers.py:23-77) on the translation columns of two equally long lists of
    world-to-camera matrices: Horn's closed-form alignment of the ground-truth points onto the estimated
    ones (S = diag(1, 1, -1) when det(U) det(Vh) < 0), then the MEAN translational error -- as the
    reference computes, despite the name.  Ground-truth poses with a NaN are skipped after the first
    (eval():561-572).  Host work in float64."""
    gt, est = _points(gt_w2c), _points(est_w2c)
    if gt.shape != est.shape or gt.ndim != 3 or gt.shape[1:] != (4, 4):
        raise ValueError("ate_rmse: two equally long lists of 4x4 matrices")
    keep = [i for i in range(gt.shape[0]) if i == 0 or not np.isnan(gt[i]).any()]
    model, data = gt[keep, :3, 3].T, est[keep, :3, 3].T  # 3 x n
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    Wm = mz @ dz.T  # sum of outer(model_i, data_i)
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    trans = data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True)
    err = rot @ model + trans - data
    return float(np.sqrt((err * err).sum(0)).mean())


# ------------------------------------------------------------------ literal form

def _gauss_window(dtype, device) -> torch.Tensor:
    """pytorch_msssim's _fspecial_gauss_1d(11, 1.5)."""
    c = torch.arange(11, dtype=dtype, device=device) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _ssim_cs(X: torch.Tensor, Y: torch.Tensor, win: torch.Tensor, data_range: float):
    C = X.shape[1]
    wh, ww = win.reshape(1, 1, 11, 1).repeat(C, 1, 1, 1), win.reshape(1, 1, 1, 11).repeat(C, 1, 1, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, wh, groups=C), ww, groups=C)  # noqa: E731 (valid, along H then W)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(X * X) - mu1_sq, filt(Y * Y) - mu2_sq, filt(X * Y) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ms_ssim_literal(X: torch.Tensor, Y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """pytorch_msssim.ms_ssim(X, Y, data_range, size_average=True) restated from its published definition with
    F.conv2d / F.avg_pool2d (include/gsr_glue.h states it): X, Y [N, C, H, W]; a scalar tensor."""
    if X.shape != Y.shape or X.dim() != 4:
        raise ValueError("ms_ssim_literal: two [N, C, H, W] images of one shape")
    if min(X.shape[-2:]) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"ms_ssim_literal: the image's smaller side must exceed {MS_SSIM_MIN_SIDE} "
                         "(four downsamplings of an 11-tap window)")
    win = _gauss_window(X.dtype, X.device)
    w = torch.tensor(MS_SSIM_WEIGHTS, dtype=X.dtype, device=X.device)
    mcs = []
    for level in range(5):
        ssim_c, cs = _ssim_cs(X, Y, win, data_range)
        if level < 4:
            mcs.append(torch.relu(cs))
            pad = [s % 2 for s in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    vals = torch.stack(mcs + [torch.relu(ssim_c)], dim=0)  # [level, N, C]
    return torch.prod(vals ** w.view(-1, 1, 1), dim=0).mean()


def evaluate_literal(im: torch.Tensor, depth_sil: torch.Tensor, gt_im: torch.Tensor, gt_depth: torch.Tensor,
                     sil_thres: float, use_sil_mask: bool = False, ms_ssim: bool = True) -> torch.Tensor:
    """One frame of eval() (:466-512) in plain torch ops on already-rendered images, on the tensors' own device
    (CPU included): the row frame_metrics writes (COLUMNS), as a float32 [8] tensor.  ms_ssim=False leaves
    that column NaN; ms_ssim=True raises for min(H, W) <= 160."""
    with torch.no_grad():
        gt_depth = gt_depth.reshape(1, *gt_depth.shape[-2:])
        rastered_depth = depth_sil[0:1]
        valid = gt_depth > 0
        rastered_depth = rastered_depth * valid
        presence = depth_sil[1] > sil_thres
        if use_sil_mask:
            wi, wg = im * presence * valid, gt_im * presence * valid
        else:
            wi, wg = im * valid, gt_im * valid
        mse = ((wi - wg) ** 2).view(wi.shape[0], -1).mean(1, keepdim=True)  # calc_psnr (slam_external.py:49-51)
        psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
        ssim = ms_ssim_literal(wi.unsqueeze(0), wg.unsqueeze(0), 1.0) if ms_ssim else \
            torch.full((), float("nan"), device=im.device)
        d = rastered_depth - gt_depth
        if use_sil_mask:
            d = d * presence
        rmse = (torch.sqrt(d ** 2) * valid).sum() / valid.sum()
        l1 = (torch.abs(d) * valid).sum() / valid.sum()
        return torch.stack([psnr, ssim.to(psnr.dtype), rmse, l1, valid.sum().to(psnr.dtype), mse[0, 0], mse[1, 0],
                            mse[2, 0]]).to(torch.float32)
