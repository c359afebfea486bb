"""gsr_resize_frame on the GPU against the numpy restatements (tests/resize_ref.py): the six size pairs of
tests/test_resize_cpu.py (a partial last block, a 12-pixel output, x and y ratios that differ, the identity), two
outputs in one launch, untouched skipped and guard memory, and NaN / unmeasured pixels.

Depth is bitwise the restatement's.  Colour is within four times the float32 restatement's own largest distance
from the float64 one, measured per case and printed beside the kernel's distance (the factor leaves room for a
fused multiply-add where numpy rounds twice); the identity is bitwise the input."""
import numpy as np
import pytest
import torch

import resize_ref as rr
from splatam_amd import resize as rz

pytestmark = pytest.mark.gpu

PAIRS = rr.SIZE_PAIRS
IDS = [f"{H}x{W}-{h}x{w}" for (H, W), (h, w) in PAIRS]
SENTINEL = -7.25


def _frame(im, depth, dev):
    return {"im": torch.from_numpy(im).to(dev), "depth": torch.from_numpy(depth).to(dev)}


def _np(frame):
    return frame["im"].cpu().numpy(), frame["depth"].cpu().numpy()


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_kernel_against_restatement(cuda, src, dst):
    im, depth = rr.make_frame(*src, seed=2)
    ref64, _ = rr.restate64(im, depth, dst)
    ref32, ref_d = rr.restate32(im, depth, dst)
    out = rz.resize_device(_frame(im, depth, cuda), dst)
    torch.cuda.synchronize()
    got, got_d = _np(out)
    assert got.shape == (3, *dst) and got_d.shape == (1, *dst)
    assert np.array_equal(rr.bits(got_d), rr.bits(ref_d))
    own, dist = rr.max_distance(ref32, ref64), rr.max_distance(got, ref64)
    same = np.array_equal(rr.bits(got), rr.bits(ref32))
    print(f"{src} -> {dst}: float32 restatement {own:.3e} from float64, kernel {dist:.3e} (bound {4 * own:.3e}); "
          f"kernel bitwise the float32 restatement: {same}")
    assert dist <= 4 * own
    if src == dst:
        assert np.array_equal(rr.bits(got), rr.bits(im))
    lit = rz.resize_literal(_frame(im, depth, cuda), dst)  # the torch form on the device's own tensors
    assert torch.equal(lit["depth"], out["depth"])
    assert rr.max_distance(lit["im"].cpu().numpy(), ref64) <= 4 * own


def _raw(frame, outs, dev):
    """gsr_resize_frame itself: outs two entries, each None (absent) or (h, w, im buffer, depth buffer)."""
    from splatam_amd._lib import lib
    H, W = frame["depth"].shape[-2:]
    args = []
    for o in outs:
        args += [0, 0, None, None] if o is None else [o[0], o[1], o[2].data_ptr(), o[3].data_ptr()]
    rc = lib.gsr_resize_frame(int(H), int(W), frame["im"].data_ptr(), frame["depth"].data_ptr(), *args,
                              torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.gsr_last_error()


def _guarded(h, w, dev):
    """An output's two buffers with one guard row behind each, all sentinels."""
    return (h, w, torch.full((3 * h * w + w,), SENTINEL, device=dev), torch.full((h * w + w,), SENTINEL, device=dev))


def test_two_outputs_in_one_call(cuda):
    (H, W), a, b = (37, 61), (13, 29), (30, 40)
    im, depth = rr.make_frame(H, W, seed=4)
    f = _frame(im, depth, cuda)
    one_a, one_b = rz.resize_device(f, a), rz.resize_device(f, b)
    two_a, two_b = rz.resize_device(f, a, b)
    into = (rz.empty_frame(a, cuda), rz.empty_frame(b, cuda))
    assert rz.resize_device(f, a, b, out=into)[0] is into[0]
    for x, y, z in ((one_a, two_a, into[0]), (one_b, two_b, into[1])):
        assert torch.equal(x["im"], y["im"]) and torch.equal(x["depth"], y["depth"])
        assert torch.equal(x["im"], z["im"]) and torch.equal(x["depth"], z["depth"])
    # guard rows behind both written buffers; then each output skipped in turn, its buffers untouched
    ga, gb = _guarded(*a, cuda), _guarded(*b, cuda)
    _raw(f, (ga, gb), cuda)
    for g, one in ((ga, one_a), (gb, one_b)):
        n = g[0] * g[1]
        assert torch.equal(g[2][:3 * n], one["im"].reshape(-1)) and torch.equal(g[3][:n], one["depth"].reshape(-1))
        assert bool((g[2][3 * n:] == SENTINEL).all()) and bool((g[3][n:] == SENTINEL).all())
    for first in (True, False):
        g, skipped = _guarded(*(a if first else b), cuda), _guarded(*(b if first else a), cuda)
        _raw(f, (g, None) if first else (None, g), cuda)
        one, n = (one_a if first else one_b), g[0] * g[1]
        assert torch.equal(g[2][:3 * n], one["im"].reshape(-1)) and torch.equal(g[3][:n], one["depth"].reshape(-1))
        assert bool((g[2][3 * n:] == SENTINEL).all()) and bool((g[3][n:] == SENTINEL).all())
        assert bool((skipped[2] == SENTINEL).all()) and bool((skipped[3] == SENTINEL).all())


@pytest.mark.parametrize("dst", [(30, 40), (24, 32), (48, 64), (60, 80)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_nan_and_unmeasured_pixels(cuda, dst):
    """One NaN colour and, in the depth, one unmeasured (0) and one NaN pixel: nearest copies the bits, bilinear
    poisons exactly the outputs that the NaN enters with a non-zero weight -- no masking."""
    (H, W), (h, w) = (48, 64), dst
    im, depth = rr.make_frame(H, W, seed=3)
    depth[depth == 0] = 1.0
    im[1, 20, 33] = np.nan
    depth[0, 10, 12], depth[0, 11, 12] = 0.0, np.nan
    out = rz.resize_device(_frame(im, depth, cuda), dst)
    torch.cuda.synchronize()
    got, got_d = _np(out)
    x0, x1, rx, _ = rr.taps(w, W)
    y0, y1, ry, _ = rr.taps(h, H)
    hit_x = (x0 == 33) | ((x1 == 33) & (rx != 0))
    hit_y = (y0 == 20) | ((y1 == 20) & (ry != 0))
    want = np.zeros((3, h, w), dtype=bool)
    want[1] = hit_y[:, None] & hit_x[None, :]
    print(f"{dst}: {int(want.sum())} poisoned outputs")
    assert want.sum() >= 1 and np.array_equal(np.isnan(got), want)
    _, ref_d = rr.restate32(im, depth, dst)
    assert np.array_equal(rr.bits(got_d), rr.bits(ref_d))
    ny, nx = rr.nearest_index(h, H), rr.nearest_index(w, W)
    assert int((got_d == 0).sum()) == int((ny == 10).sum()) * int((nx == 12).sum())
    assert int(np.isnan(got_d).sum()) == int((ny == 11).sum()) * int((nx == 12).sum())
    # the other outputs keep the colour bound (restate64 is a weighted sum: it also poisons the zero-weight
    # neighbours, which are left out of this comparison)
    ref32, ref64 = rr.restate32(im, depth, dst)[0], rr.restate64(im, depth, dst)[0]
    ok = ~want & np.isfinite(ref64)
    assert ok.sum() >= want.size - 4 * want.sum() - 3 * (h + w)
    assert rr.max_distance(got[ok], ref64[ok]) <= 4 * rr.max_distance(ref32[ok], ref64[ok])
