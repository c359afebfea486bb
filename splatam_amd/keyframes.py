"""SplaTAM's overlap keyframe selection (utils/keyframe_selection.py, scripts/splatam.py:820-837) for a SLAM
sequence that never waits on the host.

The reference back-projects a random sample of the current depth image, projects it into every keyframe but
the last, keeps the keyframes that see any of it, maps over a random `mapping_window_size - 2` of those plus
the last keyframe and the current frame, and draws one of that window per mapping iteration.  Its form reads
the device several times per frame (torch.where, unique, one comparison per keyframe).  Here

* KeyframeBank holds the keyframes on the device: images and depths [cap + 1, ...] (the last row the current
  frame), each keyframe's est_w2c as snapshotted from its pose column when it was appended (:932-945) and
  its time index.  The count is host-known (the bookkeeping is deterministic), the bank doubles on the host.
* select_device runs the whole selection as three launches (include/gsr_glue.h: gsr_keyframe_select) and
  leaves the window and the per-iteration draws on the device, ready for torch.index_select.
* select_literal is the comparison form: the same semantics in plain torch ops with host synchronisations,
  on the same random words; it runs on CPU tensors too.

Two deliberate differences from the reference (both stated in include/gsr_glue.h):
* randomness comes as 32-bit words: sample j takes the valid pixel of rank (u_pix[j] * n_valid) >> 32, the
  window is the first k eligible keyframes in (perm_key, index) order, draw i is (u_draw[i] * n_window) >> 32
  -- the reference's torch.randint / np.random.permutation / np.random.randint have bounds only the device
  knows.  The distributions are the same (uniform, up to the 2^-32 granularity of a word).
* the reference drops every sample whose world point, rounded to 1e-4 m, another sample shares: all copies of
  a pixel drawn twice (dropped here too) but also two distinct pixels in one 1e-4 m cell (kept here).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ._devcall import backproject_literal, check_rc, f32, require, zero_workspace
from .slam import build_rotation

EDGE = 20  # keyframe_selection_overlap's image border


def pose_w2c(params: dict, t: int) -> torch.Tensor:
    """The [4, 4] world-to-camera matrix of pose column t (scripts/splatam.py:823-827; device ops only)."""
    with torch.no_grad():
        q = params["cam_unnorm_rots"]
        w2c = torch.eye(4, device=q.device, dtype=torch.float32)
        w2c[:3, :3] = build_rotation(F.normalize(q[..., t].detach()))
        w2c[:3, 3] = params["cam_trans"][..., t].detach()
    return w2c


def draw_words(rng: np.random.RandomState, n: int) -> np.ndarray:
    """n random 32-bit words (uint32) from a numpy stream."""
    return rng.randint(0, 1 << 32, size=int(n), dtype=np.uint64).astype(np.uint32)


def words_tensor(words, device=None) -> torch.Tensor:
    """32-bit words as an int32 tensor carrying their bits (the form both selections take)."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    return torch.from_numpy(w.view(np.int32).copy()).to(device if device is not None else "cpu")


def _u64(words: torch.Tensor) -> torch.Tensor:
    return words.to(torch.int64) & 0xFFFFFFFF


class WordFeed:
    """Random words to the device without a blocking copy: a small ring of pinned buffers, a non-blocking
    copy each and an event that guards the buffer's reuse (GraphMapper._load's pattern)."""

    def __init__(self, device, ring: int = 4):
        self.device, self.ring = device, int(ring)
        self._host = [None] * self.ring
        self._event = [None] * self.ring
        self._i = 0

    def push(self, words: np.ndarray) -> torch.Tensor:
        i, n = self._i, int(words.shape[0])
        self._i = (i + 1) % self.ring
        if self._event[i] is not None:
            self._event[i].synchronize()  # (a copy enqueued `ring` pushes ago)
        if self._host[i] is None or self._host[i].numel() < n:
            self._host[i] = torch.empty(max(n, 64), dtype=torch.int32, pin_memory=True)
        self._host[i][:n] = torch.from_numpy(words.view(np.int32))
        dst = torch.empty(n, dtype=torch.int32, device=self.device)
        dst.copy_(self._host[i][:n], non_blocking=True)
        self._event[i] = torch.cuda.Event()
        self._event[i].record()
        return dst


class KeyframeBank:
    """The keyframes of a sequence on the device.  Rows 0 .. n - 1 are the keyframes in the order they were
    appended; row `cap` (the last) holds the current frame.  est_w2c [cap, 16] and time [cap] (int64) are the
    tables gsr_keyframe_select reads."""

    def __init__(self, im_shape, depth_shape, device, capacity: int = 16):
        self.device = device
        self.cap, self.n = int(capacity), 0
        self.im = torch.zeros((self.cap + 1,) + tuple(im_shape), device=device)
        self.depth = torch.zeros((self.cap + 1,) + tuple(depth_shape), device=device)
        self.est_w2c = torch.zeros(self.cap, 16, device=device)
        self.time = torch.zeros(self.cap, dtype=torch.int64, device=device)
        self.times = []  # the host's copy of the time indices

    @property
    def cur_row(self) -> int:
        return self.cap

    def _grow(self):
        cap = 2 * self.cap
        im = torch.zeros((cap + 1,) + tuple(self.im.shape[1:]), device=self.device)
        depth = torch.zeros((cap + 1,) + tuple(self.depth.shape[1:]), device=self.device)
        est = torch.zeros(cap, 16, device=self.device)
        time = torch.zeros(cap, dtype=torch.int64, device=self.device)
        im[:self.cap], depth[:self.cap] = self.im[:self.cap], self.depth[:self.cap]
        im[cap], depth[cap] = self.im[self.cap], self.depth[self.cap]
        est[:self.cap], time[:self.cap] = self.est_w2c, self.time
        self.im, self.depth, self.est_w2c, self.time, self.cap = im, depth, est, time, cap

    def set_current(self, im: torch.Tensor, depth: torch.Tensor):
        with torch.no_grad():
            self.im[self.cap].copy_(im)
            self.depth[self.cap].copy_(depth)

    def append(self, im: torch.Tensor, depth: torch.Tensor, params: dict, t: int) -> bool:
        """Frame t becomes keyframe n: its image, depth, time index and est_w2c -- the pose column as it is
        NOW (the reference's snapshot, :932-945; later mapping does not move it).  Returns True when the
        bank grew (its tensors are new ones)."""
        grew = self.n == self.cap
        if grew:
            self._grow()
        with torch.no_grad():
            self.im[self.n].copy_(im)
            self.depth[self.n].copy_(depth)
            self.est_w2c[self.n].copy_(pose_w2c(params, t).reshape(16))
            self.time[self.n] = int(t)
        self.times.append(int(t))
        self.n += 1
        return grew


def _outputs(n_kf: int, k_select: int, S: int, n_draws: int, device, pixels: bool) -> dict:
    i32 = dict(dtype=torch.int32, device=device)
    return {"overlap": torch.empty(max(n_kf - 1, 0), **i32), "n_points": torch.empty(1, **i32),
            "window": torch.empty(k_select + 2, **i32), "n_window": torch.empty(1, **i32),
            "draw_rows": torch.empty(n_draws, dtype=torch.int64, device=device),
            "draw_times": torch.empty(n_draws, dtype=torch.int64, device=device),
            "pixels": torch.empty(S, **i32) if pixels else None}


def workspace_bytes(H: int, S: int) -> int:
    from ._lib import lib
    return int(lib.gsr_keyframe_workspace_bytes(int(H), int(S)))


def make_workspace(H: int, S: int, device) -> torch.Tensor:
    """A zero-filled workspace for select_device (any smaller H / S can share it)."""
    return zero_workspace(workspace_bytes(H, S), device)


def select_device(depth: torch.Tensor, intrinsics, w2c: torch.Tensor, kf_w2c: torch.Tensor, n_kf: int, k_select: int,
                  u_pix: torch.Tensor, perm_key: torch.Tensor, u_draw: torch.Tensor, kf_time: torch.Tensor,
                  time_idx: int, cur_row: int, workspace: torch.Tensor | None = None, out: dict | None = None,
                  pixels: bool = False) -> dict:
    """gsr_keyframe_select on the current stream: no host read, every result a device tensor (see the module
    docstring and include/gsr_glue.h).  depth [H, W] or [1, H, W]; w2c [4, 4]; kf_w2c [>= n_kf, 16]; kf_time
    [>= n_kf] int64; u_pix / perm_key / u_draw: int32 tensors carrying 32-bit words (perm_key at least
    n_kf - 1 of them).  workspace: make_workspace(H, S) (zero-filled once; None allocates one), out: the
    dict of a previous call to write into again."""
    from ._lib import lib
    if not depth.is_cuda:
        raise RuntimeError("select_device: ROCm devices only (select_literal is the host form)")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    dev = depth.device
    n_kf, k_select, S, n_draws = int(n_kf), int(k_select), int(u_pix.numel()), int(u_draw.numel())
    require("select_device", dev, (("depth", depth, torch.float32, H * W), ("w2c", w2c, torch.float32, 16),
                                   ("kf_w2c", kf_w2c, torch.float32, 16 * n_kf), ("kf_time", kf_time, torch.int64, n_kf),
                                   ("u_pix", u_pix, torch.int32, S),
                                   ("perm_key", perm_key, torch.int32, max(n_kf - 1, 0)),
                                   ("u_draw", u_draw, torch.int32, n_draws)))
    if workspace is None:
        workspace = make_workspace(H, S, dev)
    if workspace.device != dev or workspace.numel() * workspace.element_size() < workspace_bytes(H, S):
        raise RuntimeError("select_device: workspace too small (make_workspace(H, S))")
    if out is None:
        out = _outputs(n_kf, k_select, S, n_draws, dev, pixels)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    px = out.get("pixels")
    rc = lib.gsr_keyframe_select(H, W, depth.data_ptr(), fx, fy, cx, cy, w2c.data_ptr(), kf_w2c.data_ptr(), n_kf,
                                 k_select, S, u_pix.data_ptr(), perm_key.data_ptr(), n_draws, u_draw.data_ptr(),
                                 kf_time.data_ptr(), int(time_idx), int(cur_row), workspace.data_ptr(),
                                 out["overlap"].data_ptr(), out["n_points"].data_ptr(), out["window"].data_ptr(),
                                 out["n_window"].data_ptr(), out["draw_rows"].data_ptr(),
                                 out["draw_times"].data_ptr(), None if px is None else px.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    check_rc(rc, "gsr_keyframe_select")
    return out


def select_literal(depth: torch.Tensor, intrinsics, w2c: torch.Tensor, kf_w2c: torch.Tensor, n_kf: int, k_select: int,
                   u_pix: torch.Tensor, perm_key: torch.Tensor, u_draw: torch.Tensor, kf_time: torch.Tensor,
                   time_idx: int, cur_row: int) -> dict:
    """select_device's semantics in plain torch ops, on the tensors' own device (CPU included), with host
    synchronisations where the reference has them.  Every float operation is an elementwise float32 op in the
    order include/gsr_glue.h states, so the kernels form the same bits."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    dev = depth.device
    n_kf, k_select, S, n_draws = int(n_kf), int(k_select), int(u_pix.numel()), int(u_draw.numel())
    n_cand = max(n_kf - 1, 0)
    fx, fy, cx, cy = (f32(v, dev) for v in intrinsics)
    with torch.no_grad():
        flat = depth.reshape(-1)
        valid = torch.nonzero(flat > 0)[:, 0]  # row-major, torch.where's order (host synchronisation)
        n_valid = int(valid.numel())
        if n_valid == 0 or S == 0:
            pix = torch.full((S,), -1, dtype=torch.int64, device=dev)
            keep = torch.zeros(S, dtype=torch.bool, device=dev)
            pw = [torch.zeros(S, device=dev)] * 3
        else:
            r = (_u64(u_pix) * n_valid) >> 32
            pix = valid[r]
            row, col = torch.div(pix, W, rounding_mode="floor"), pix % W
            pw = backproject_literal(col, row, flat[pix], fx, fy, cx, cy, w2c)
            twice = (r[:, None] == r[None, :]).sum(dim=1) > 1
            origin = (torch.round(pw[0] * 1e4) == 0) & (torch.round(pw[1] * 1e4) == 0) & \
                (torch.round(pw[2] * 1e4) == 0)
            keep = ~twice & ~origin
        if n_cand > 0:
            k = kf_w2c[:n_cand].reshape(n_cand, 16).to(torch.float32)
            c = lambda i: k[:, i:i + 1]  # noqa: E731
            wx, wy, wz = (p[None, :] for p in pw)
            px = c(0) * wx + c(1) * wy + c(2) * wz + c(3)
            py = c(4) * wx + c(5) * wy + c(6) * wz + c(7)
            pz = c(8) * wx + c(9) * wy + c(10) * wz + c(11)
            zz = pz + f32(1e-5, dev)
            u = (fx * px + cx * pz) / zz
            v = (fy * py + cy * pz) / zz
            inside = (u > EDGE) & (u < W - EDGE) & (v > EDGE) & (v < H - EDGE) & (zz > 0) & keep[None, :]
            overlap = inside.sum(dim=1).to(torch.int32)
        else:
            overlap = torch.zeros(0, dtype=torch.int32, device=dev)
        keys = _u64(perm_key[:n_cand]).tolist()
        eligible = sorted((keys[i], i) for i in torch.nonzero(overlap > 0)[:, 0].tolist())
        win = [i for _, i in eligible[:k_select]]
        if n_kf > 0:
            win.append(n_kf - 1)
        win.append(int(cur_row))
        n_window = len(win)
        window = torch.tensor(win + [-1] * (k_select + 2 - n_window), dtype=torch.int32, device=dev)
        idx = (_u64(u_draw) * n_window) >> 32
        rows = window.to(torch.int64)[idx]
        times = torch.full_like(rows, int(time_idx))
        if n_kf > 0:
            is_kf = rows != int(cur_row)
            times = torch.where(is_kf, kf_time[:n_kf][rows.clamp(max=n_kf - 1)], times)
    return {"overlap": overlap, "n_points": keep.sum().to(torch.int32).reshape(1), "window": window,
            "n_window": torch.tensor([n_window], dtype=torch.int32, device=dev), "draw_rows": rows,
            "draw_times": times, "pixels": pix.to(torch.int32), "draw_index": idx}
