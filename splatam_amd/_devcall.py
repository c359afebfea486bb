"""What the sequence steps' device calls (keyframes.select_device, evaluate.frame_metrics, densify.densify_device)
and their *_literal comparison forms share."""
from __future__ import annotations

import torch


def zero_workspace(nbytes: int, device) -> torch.Tensor:
    """A zero-filled (once: include/gsr_glue.h) workspace of at least nbytes."""
    return torch.zeros((int(nbytes) + 3) // 4, dtype=torch.int32, device=device)


def require(where: str, device, checks, exact=(), size: str = "{dt} tensor of >= {n}"):
    """The tensors a call reads through data_ptr, as (name, tensor, dtype, numel): contiguous, of that dtype, on
    `device`, with at least numel elements (the names in `exact`: exactly).  One call for all of them: this runs
    on every step, between the caller's events.  size: how the message words the dtype and the count."""
    for name, t, dt, n in checks:
        if t.dtype != dt or t.device != device or not t.is_contiguous() or \
                (t.numel() != n if name in exact else t.numel() < n):
            raise RuntimeError(f"{where}: {name} must be a contiguous {size.format(dt=dt, n=n)} elements on {device}")


def check_rc(rc: int, what: str):
    """include/gsr.h: negative return values are errors, gsr_last_error() gives the message.  (The forward calls
    return num_rendered >= 0; the sequence steps return GSR_OK or an error, never a positive value.)"""
    if rc < 0:
        from ._lib import lib
        raise RuntimeError(f"{what}: {lib.gsr_last_error().decode(errors='replace')}")


TILE_SORT_CAP = 4096  # longest tile list the static mode handles (render_fwd's per-tile sort)


def capacity_from_probes(probes, headroom: float, min_extra: int) -> int:
    """The static binning capacity for frames that probed as `probes` ((num_rendered, longest tile list) each):
    headroom times the largest num_rendered plus min_extra.  A tile list over TILE_SORT_CAP is refused."""
    longest = max(p[1] for p in probes)
    if longest > TILE_SORT_CAP:
        raise RuntimeError(f"a tile list of {longest} > {TILE_SORT_CAP}: use the eager (synchronous) path")
    return max(1, int(headroom * max(p[0] for p in probes)) + int(min_extra))


def status_overflowed(status: torch.Tensor, capacity: int) -> bool:
    """True if any row of a static-mode status tensor [iters, 4] (sticky across replays, include/gsr.h) shows more
    instances than `capacity`, a tile list over TILE_SORT_CAP or a prefiltered violation.  One host sync."""
    st = status.cpu()
    return bool((st[:, 0] > capacity).any() or (st[:, 2] > TILE_SORT_CAP).any() or (st[:, 1] != 0).any())


def f32(v, device) -> torch.Tensor:
    """v as a float32 scalar tensor (an elementwise op with it rounds like the kernels' float)."""
    return torch.tensor(float(v), dtype=torch.float32, device=device)


def backproject_literal(col, row, z, fx, fy, cx, cy, w2c: torch.Tensor) -> list:
    """The world points [x, y, z] of pixels (col, row) at depths z through the rigid inverse [R^T, -R^T t] of w2c
    in elementwise float32 ops, every sum left to right: the order include/gsr_glue.h states and the kernels'
    backproject keeps.  fx, fy, cx, cy: f32 scalars."""
    x = (col.to(torch.float32) - cx) / fx * z
    y = (row.to(torch.float32) - cy) / fy * z
    m = w2c.reshape(-1).to(torch.float32)
    pw = []
    for a in range(3):
        ra, rb, rc = m[a], m[4 + a], m[8 + a]
        ta = -(ra * m[3] + rb * m[7] + rc * m[11])
        pw.append(ra * x + rb * y + rc * z + ta)
    return pw
