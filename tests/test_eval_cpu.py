"""CPU checks of the evaluation path (splatam_amd/evaluate.py): the plain-torch literal form against the float64
numpy restatement of tests/eval_ref.py, the MS-SSIM size condition, the trajectory error, the ABI table, and
PSNR against the reference's own calc_psnr (tests/golden/eval_psnr.npz, tests/golden/make_eval_goldens.py).

Bounds of the float32 literal against the float64 restatement (relative; u = 2^-24 = 6.0e-8 is float32's unit
roundoff): every column but MS-SSIM is a handful of elementwise operations and one sum of at most 2^16 terms that
torch adds pairwise (a rounding chain of ~16 + 8 operations, each <= u): 32 u = 2e-6.  MS-SSIM subtracts
mu^2 from E[x^2] (for these images E[x^2] / sigma^2 <= 8, so each moment's ~12 u becomes ~1e-5 in a pixel of the
maps; the mean over >= 1 pixel and the product of five levels' powers, exponents summing to 1, keep it):
1e-5.  The distances measured here are printed; the largest over these cases and the pixel-only shapes of
tests/test_gpu_eval.py are that module's MEASURED."""
import os

import numpy as np
import pytest
import torch

import eval_ref as er
from splatam_amd import evaluate as ev

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_psnr.npz")
RTOL = {"psnr": 2e-6, "ms_ssim": 1e-5, "depth_rmse": 2e-6, "depth_l1": 2e-6, "n_valid": 0.0, "mse_r": 2e-6,
        "mse_g": 2e-6, "mse_b": 2e-6}


def _torch_case(c, device="cpu"):
    return [torch.from_numpy(np.array(c[k])).to(device) for k in ("im", "depth_sil", "gt_im", "gt_depth")]


@pytest.mark.parametrize("use_sil", [False, True])
@pytest.mark.parametrize("H,W", [(161, 163), (176, 200)])
def test_literal_matches_restatement(H, W, use_sil):
    c = er.make_case(H, W)
    ref = er.reference(H, W, use_sil)
    assert 0 < ref[4] < H * W and 0.5 < ref[1] < 0.999  # a zeroed depth region; a non-trivial MS-SSIM
    if use_sil:
        assert abs(ref[0] - er.reference(H, W, False)[0]) > 0.1  # the low-silhouette region changes the masks
    got = ev.evaluate_literal(*_torch_case(c), c["sil_thres"], use_sil_mask=use_sil).numpy().astype(np.float64)
    for i, name in enumerate(er.COLS):
        rel = abs(got[i] - ref[i]) / abs(ref[i])
        print(f"{H}x{W} sil={use_sil} {name}: literal {got[i]!r} ref {ref[i]!r} rel {rel:.3e}")
        assert rel <= RTOL[name], name


@pytest.mark.parametrize("H,W", [(161, 163), (176, 200)])
def test_ms_ssim_literal_matches_restatement(H, W):
    c = er.make_case(H, W)
    x, y = c["im"], c["gt_im"]
    ref = er.ms_ssim(x.astype(np.float64), y.astype(np.float64))
    got = float(ev.ms_ssim_literal(torch.from_numpy(np.array(x))[None], torch.from_numpy(np.array(y))[None]))
    got64 = float(ev.ms_ssim_literal(torch.from_numpy(np.array(x))[None].double(),
                                     torch.from_numpy(np.array(y))[None].double()))
    print(f"{H}x{W}: literal {got!r} literal(float64) {got64!r} ref {ref!r}")
    assert abs(got - ref) <= 1e-5 * ref
    assert abs(got64 - ref) <= 1e-12 * ref  # the two restatements are the same function


def test_ms_ssim_of_identical_images_is_one():
    x = torch.from_numpy(np.array(er.make_case(161, 163)["gt_im"]))[None]
    v = float(ev.ms_ssim_literal(x, x))
    assert abs(v - 1.0) <= 1e-5
    assert abs(er.ms_ssim(x[0].numpy().astype(np.float64), x[0].numpy().astype(np.float64)) - 1.0) <= 1e-12


def test_small_side_is_refused():
    x = torch.rand(1, 3, 160, 200)
    with pytest.raises(ValueError, match="160"):
        ev.ms_ssim_literal(x, x)
    with pytest.raises(ValueError):
        er.ms_ssim(np.zeros((3, 160, 200)), np.zeros((3, 160, 200)))
    c = er.make_case(160, 200)
    with pytest.raises(ValueError, match="160"):
        ev.evaluate_literal(*_torch_case(c), 0.5, ms_ssim=True)
    row = ev.evaluate_literal(*_torch_case(c), 0.5, ms_ssim=False)
    assert torch.isnan(row[1]) and torch.isfinite(row[0])


def test_literal_invalid_depth_and_equal_images():
    """n_valid == 0: NaN depth columns (0 / 0) and PSNR of two zero images = inf, nothing special-cased."""
    c = er.make_case(5, 7, depth="invalid")
    row = ev.evaluate_literal(*_torch_case(c), 0.5, ms_ssim=False)
    assert torch.isinf(row[0]) and row[0] > 0 and torch.isnan(row[2]) and torch.isnan(row[3]) and row[4] == 0
    assert (row[5:] == 0).all()


# ------------------------------------------------------------------ trajectory

def _traj(n=12, seed=3):
    rng = np.random.RandomState(seed)
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, 3] = np.cumsum(rng.randn(n, 3) * 0.1, axis=0) + rng.randn(3)
    return T


def _rot(axis, ang):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def test_ate_of_a_rigid_copy_is_zero():
    gt = _traj()
    R, t = _rot([1, 2, 3], 0.7), np.array([0.3, -1.0, 2.0])
    est = gt.copy()
    est[:, :3, 3] = gt[:, :3, 3] @ R.T + t
    assert ev.ate_rmse(list(torch.from_numpy(gt)), list(torch.from_numpy(est))) < 1e-12
    assert er.ate(gt, est) < 1e-12


def test_ate_of_a_known_offset():
    """Four points at (+-1, +-1, 0) with offsets +-d along z alternating around the square: centred, and with no
    first-order rotation (the moment sum of p x offset vanishes), so the identity alignment is optimal and
    every point keeps the error d; the result is the mean, d."""
    gt = np.tile(np.eye(4), (4, 1, 1))
    gt[:, :3, 3] = [[1, 1, 0], [-1, 1, 0], [-1, -1, 0], [1, -1, 0]]
    d = 0.05
    est = gt.copy()
    est[:, 2, 3] += d * np.array([1, -1, 1, -1])
    got = ev.ate_rmse(gt, est)
    assert abs(got - d) <= 1e-12 and abs(er.ate(gt, est) - d) <= 1e-12


def test_ate_reflected_configuration():
    """A mirrored copy: the unconstrained optimum is a reflection, so det(U) det(Vh) < 0 and S[2,2] = -1 keeps a
    proper rotation -- the error is then NOT zero (a reflection would make it zero)."""
    gt = _traj(10, seed=5)
    est = gt.copy()
    est[:, 0, 3] = -gt[:, 0, 3]
    model = gt[:, :3, 3].T - gt[:, :3, 3].T.mean(1, keepdims=True)
    data = est[:, :3, 3].T - est[:, :3, 3].T.mean(1, keepdims=True)
    U, _, Vh = np.linalg.svd((model @ data.T).T)
    assert np.linalg.det(U) * np.linalg.det(Vh) < 0  # the branch is taken
    got, ref = ev.ate_rmse(gt, est), er.ate(gt, est)
    assert got > 1e-3 and abs(got - ref) <= 1e-12 * max(1.0, ref)


def test_ate_skips_nan_ground_truth():
    gt, est = _traj(9, seed=8), _traj(9, seed=9)
    keep = [0, 1, 2, 4, 5, 7, 8]
    bad = gt.copy()
    bad[3, 1, 2] = np.nan
    bad[6] = np.nan
    want = er.ate(gt[keep], est[keep])
    assert abs(ev.ate_rmse(bad, est) - want) <= 1e-12
    assert abs(er.ate(bad, est) - want) <= 1e-12
    assert abs(ev.ate_rmse(torch.from_numpy(bad).float(), torch.from_numpy(est).float()) - want) <= 1e-6


# ------------------------------------------------------------------ ABI / golden

def test_eval_symbols_in_abi_table_and_library():
    import ctypes

    from splatam_amd import _lib
    assert len(_lib.SIGNATURES["gsr_eval_workspace_bytes"][1]) == 3
    assert len(_lib.SIGNATURES["gsr_eval_frame"][1]) == 12
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "gsr_eval_frame") and hasattr(lib, "gsr_eval_workspace_bytes")
    big, small, pix = (ev.workspace_bytes(240, 320), ev.workspace_bytes(161, 163), ev.workspace_bytes(240, 320, False))
    assert big > small > pix > 0 and pix == ev.workspace_bytes(5, 7, False)
    assert ev.workspace_bytes(160, 200) == 0  # a size gsr_eval_frame refuses
    assert _lib.lib.gsr_abi_version() == 8


def test_frame_metrics_refuses_cpu_tensors():
    c = er.make_case(5, 7)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        ev.frame_metrics(*_torch_case(c), 0.5, torch.zeros(8), torch.zeros(64, dtype=torch.int32), ms_ssim=False)


def test_psnr_matches_reference_calc_psnr():
    g = np.load(GOLD)
    im, gt_im, mask = (torch.from_numpy(g[k]) for k in ("im", "gt_im", "mask"))
    H, W = im.shape[1:]
    # a depth whose validity IS the mask, a silhouette above the threshold everywhere
    gt_depth = mask.to(torch.float32)
    depth_sil = torch.ones(3, H, W)
    row = ev.evaluate_literal(im, depth_sil, gt_im, gt_depth, 0.5, ms_ssim=False)
    assert abs(float(row[0]) - float(g["psnr"])) <= 2e-6 * float(g["psnr"])
    ref = er.frame_metrics(g["im"], depth_sil.numpy(), g["gt_im"], gt_depth.numpy(), 0.5, False, False)
    assert abs(ref[0] - float(g["psnr"])) <= 2e-6 * float(g["psnr"])
    mse = 10.0 ** (-g["psnr_per_channel"].astype(np.float64)[:, 0] / 10.0)
    assert np.allclose(ref[5:], mse, rtol=4e-6, atol=0)
