"""CPU checks of splatam_amd.densify: densify_literal (elementwise torch ops on CPU tensors) against the numpy
restatement of the contract (tests/densify_ref.py), the lower-median convention, the ctypes table and the
exported symbols, the argument checks of the two SLAM loops, and downscale_capture."""
import inspect

import numpy as np
import pytest
import torch

import densify_ref as dr
from splatam_amd import densify as dn

CASES = [(H, W, "random") for H, W in dr.SHAPES] + [(61, 67, c) for c in dr.CONTENTS[1:]] + \
    [(97, 131, c) for c in dr.CONTENTS[1:]]


def literal(case: dict, device="cpu"):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    curr = {"im": t(case["im"]), "depth": t(case["gt"])}
    return dn.densify_literal(curr, t(case["w2c"]).reshape(4, 4), case["intrinsics"], case["sil_thres"],
                              t(case["depth_sil"]))


@pytest.mark.parametrize("H,W,content", CASES)
def test_literal_equals_restatement(H, W, content):
    case = dr.make_case(H, W, content, seed=1)
    ref = dr.restate(case)
    rows, mask, count = literal(case)
    assert count == ref["count"]
    assert np.array_equal(mask.numpy(), ref["mask"])
    rank = torch.where(mask, torch.cumsum(mask.to(torch.int64), 0) - 1, torch.full((H * W,), -1, dtype=torch.int64))
    assert np.array_equal(rank.numpy(), ref["rank"])
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities"):
        assert rows[k].shape == (count, dr.COLS[k]) and rows[k].dtype == torch.float32
        assert np.array_equal(dr.bits(rows[k].numpy()), dr.bits(ref["rows"][k])), k
    assert rows["log_scales"].shape == (count, 1)
    d = dr.rel_distance(rows["log_scales"].numpy(), ref["rows"]["log_scales"])
    print(f"{H}x{W} {content}: {count} selected, med {ref['med']!r}, log_scales rel distance {d:.3e}")
    assert d <= 2.0 ** -23  # (a float32 rounding of a float64 logarithm: half an ulp, and torch.log's own)
    if content == "gt_zero":
        assert count == 0
    if content == "all_selected":
        assert count == H * W
    if content == "zeros90":
        assert ref["med"] == 0
    if content == "denormal":
        assert 0 < ref["med"] < np.finfo(np.float32).tiny
    if content == "nan_depth":
        sil = case["depth_sil"][1].reshape(-1)
        assert np.isnan(ref["med"]) and np.array_equal(ref["mask"], (sil < 0.5) & (case["gt"].reshape(-1) > 0))
    if content == "nan_sil":
        assert not ref["mask"][dr.NAN_PIXEL]


@pytest.mark.parametrize("n", [1, 2, 7, 8, 1001, 1002])
def test_lower_median_is_torch_median(n):
    rng = np.random.RandomState(n)
    for v in (rng.standard_normal(n).astype(np.float32), rng.randint(0, 3, n).astype(np.float32)):
        got = float(torch.from_numpy(v).median())
        assert got == float(dr.lower_median(v)) == float(np.sort(v)[(n - 1) // 2])
    v = rng.uniform(size=n).astype(np.float32)
    v[n // 2] = np.nan
    assert np.isnan(float(torch.from_numpy(v).median())) and np.isnan(dr.lower_median(v))


def test_signatures_and_exports():
    from splatam_amd import _lib, build
    for name in ("gsr_densify_frame", "gsr_densify_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["gsr_densify_frame"][1]) == 24
    assert len(_lib.SIGNATURES["gsr_densify_workspace_bytes"][1]) == 2
    assert "gsr_densify.hip" in build.SOURCES
    assert _lib.lib.gsr_abi_version() == 8
    small, big = dn.workspace_bytes(5, 7), dn.workspace_bytes(480, 640)
    assert 0 < small < big and small % 8 == 0 and small >= 4 * 16
    assert dn.workspace_bytes(0, 7) == 0 and dn.workspace_bytes(5, -1) == 0
    assert dn.make_workspace(480, 640, "cpu").numel() * 4 >= big
    for bad in ((0, 7), (5, 0), (-3, 7)):  # refused before anything is enqueued: no device is touched
        assert _lib.lib.gsr_densify_frame(*bad, *([None] * 3), 1.0, 1.0, 0.0, 0.0, None, 0.5, 4, *([None] * 12)) != 0
    assert b"densify_frame" in _lib.lib.gsr_last_error()


def test_loops_take_the_densify_arguments():
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    for cls in (SlamSequence, PerFrameSlam):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["densify_mode"].default == "torch"
        assert all(sig[k].default is None for k in ("densify_frames", "densify_cam", "densify_intrinsics"))


def test_value_errors():
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    frames = [{"im": torch.zeros(3, 4, 6), "depth": torch.ones(1, 4, 6)}] * 2
    params = {"means3D": torch.zeros(5, 3), "rgb_colors": torch.zeros(5, 3), "log_scales": torch.zeros(5, 1)}
    intr = (5.0, 5.0, 3.0, 2.0)
    small, small_intr = dn.downscale_capture(frames, intr, 2)
    bad = [dict(densify_mode="hip"), dict(densify_mode=None), dict(densify_frames=small),
           dict(densify_frames=small, densify_intrinsics=small_intr), dict(densify_cam=object()),
           dict(densify_cam=object(), densify_intrinsics=small_intr),
           dict(densify_frames=small[:1], densify_cam=object(), densify_intrinsics=small_intr)]
    for kw in bad:
        with pytest.raises(ValueError):
            SlamSequence(params, frames, None, None, intr, capacity=16, bin_capacity=16, **kw)
        with pytest.raises(ValueError):
            PerFrameSlam(params, frames, None, None, intr, **kw)
    with pytest.raises(ValueError):
        dn.downscale_capture(frames, intr, 4)  # 6 columns
    with pytest.raises(ValueError):
        dn.downscale_capture(frames, intr, 0)


def test_downscale_capture():
    g = torch.Generator().manual_seed(3)
    frames = [{"im": torch.rand(3, 8, 12, generator=g), "depth": torch.rand(1, 8, 12, generator=g)} for _ in range(2)]
    small, intr = dn.downscale_capture(frames, (100.0, 104.0, 6.0, 4.0), 2)
    assert intr == (50.0, 52.0, 3.0, 2.0) and len(small) == 2
    for s, f in zip(small, frames):
        assert s["im"].shape == (3, 4, 6) and s["depth"].shape == (1, 4, 6)
        assert s["im"].is_contiguous() and s["depth"].is_contiguous()
        assert torch.equal(s["depth"], f["depth"][:, ::2, ::2])  # nearest: a measured depth, never a blend
        box = (f["im"][:, 0::2, 0::2] + f["im"][:, 0::2, 1::2] + f["im"][:, 1::2, 0::2] + f["im"][:, 1::2, 1::2]) / 4
        assert torch.allclose(s["im"], box, atol=1e-6)  # bilinear at factor 2: the 2 x 2 mean
    same, intr1 = dn.downscale_capture(frames, (100.0, 104.0, 6.0, 4.0), 1)
    assert intr1 == (100.0, 104.0, 6.0, 4.0) and torch.equal(same[0]["depth"], frames[0]["depth"])
    cam = dn.downscale_camera(12, 8, (100.0, 104.0, 6.0, 4.0), 2, "cpu")
    assert (cam.image_height, cam.image_width) == (4, 6)
    assert cam.tanfovx == 6 / (2 * 50.0) and cam.tanfovy == 4 / (2 * 52.0)
