"""The silhouette gain next to the EIG (splatam_amd.fisher: silhouette_count, BatchedFisher mode "gains";
gsr_silhouette_count, csrc/gsr_viewgain.hip) on the GPU.

The count is an integer, so against existing code it must be exact: equal to (sil < thres).sum() of the drop-in
GaussianRasterizer render of SplaTAM's [z, 1, z^2] colours (channel 1) on the same camera-frame points.  Against
the float32 CPU oracle it is bracketed by the oracle's counts at thres -+ the forward-image tolerance."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import harness
from splatam_amd.fisher import BatchedFisher, FisherScorer, _count_into, camera_points, silhouette_count
from splatam_amd.rasterizer import GaussianRasterizer
from splatam_amd.scenes import Scene, make_scene
from splatam_amd.slam import camera_settings, init_tracking_params
from test_viewgain_cpu import _restated

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.5, 0.99, 0.0, 1.5)


def _pose(deg, t):
    a = math.radians(deg)
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    w2c[:3, 3] = torch.tensor(t)
    return w2c


@functools.lru_cache(maxsize=None)
def _scorer(P, W, H, seed, bg1=0.0):
    dev = torch.device("cuda:0")
    scene = make_scene(P, W, H, seed=seed)
    params = init_tracking_params(scene, num_frames=1, device=dev)
    cam = camera_settings(scene.cam, dev)
    if bg1 != 0.0:
        cam = cam._replace(bg=torch.tensor([0.1, bg1, 0.2], dtype=torch.float32, device=dev))
    return scene, FisherScorer(params, cam)


def _dropin_silhouette(sc, w2c):
    """Channel 1 of the drop-in render of [z, 1, z^2] on the camera-frame points (one render, shared by the
    thresholds of a case)."""
    with torch.no_grad():
        pts = camera_points(sc.params["means3D"], w2c)
        z = pts[:, 2:3]
        im, _, _ = GaussianRasterizer(sc.cam)(
            means3D=pts, means2D=torch.zeros_like(pts), opacities=sc.opacities,
            colors_precomp=torch.cat([z, torch.ones_like(z), z * z], 1), scales=sc.scales, rotations=sc.rotations)
    return im[1]


def _check_exact(sc, w2c, thresholds=THRESHOLDS):
    sil = _dropin_silhouette(sc, w2c)
    W, H = sc.cam.image_width, sc.cam.image_height
    got = {t: int(silhouette_count(sc, w2c, t)) for t in thresholds}
    want = {t: int((sil < t).sum()) for t in thresholds}
    print(f"{W}x{H}: counts {got}")
    assert got == want
    return got


@pytest.mark.parametrize("P,W,H,seed", [(3000, 128, 96, 32), (2000, 100, 75, 33), (3000, 64, 48, 34)])
def test_count_equals_dropin_render(cuda, P, W, H, seed):
    """128x96; 100x75: partial tiles on both edges (pixels outside the image never count); 64x48 with 3000
    Gaussians: every tile list runs past one 256-entry staging batch, so pixels are decided between batches."""
    _, sc = _scorer(P, W, H, seed)
    got = _check_exact(sc, torch.eye(4, device=cuda))
    assert got[0.0] == 0 and got[1.5] == W * H  # strict comparison; nothing reaches 1.5
    # the scene decides both ways (the dense 64x48 one only at 0.99: every pixel there passes 0.5 early)
    assert got[0.5] < got[0.99] < W * H and (got[0.5] > 0 or (W, H) == (64, 48))


def test_count_with_empty_tiles(cuda):
    """A pose turned away: part of the image sees nothing (empty tile lists, silhouette 0 there)."""
    _, sc = _scorer(3000, 128, 96, 32)
    w2c = _pose(25.0, [0.0, 0.0, 0.0]).to(cuda)
    sil = _dropin_silhouette(sc, w2c)
    empty_cols = int((sil.amax(dim=0) == 0).sum())
    assert empty_cols >= 16, empty_cols  # at least a tile column without a Gaussian
    _check_exact(sc, w2c)


def test_count_of_empty_and_culled_maps(cuda):
    scene = make_scene(0, 64, 48, seed=1)
    params = init_tracking_params(scene, num_frames=1, device=cuda)
    sc0 = FisherScorer(params, camera_settings(scene.cam, cuda))
    eye = torch.eye(4, device=cuda)
    assert int(silhouette_count(sc0, eye, 0.5)) == 64 * 48
    assert int(silhouette_count(sc0, eye, 0.0)) == 0
    # every Gaussian behind the camera: the forward runs with empty lists, the value is the background's
    behind = torch.eye(4, device=cuda)
    behind[2, 3] = -100.0
    for bg1 in (0.0, 0.3):
        _, sc = _scorer(2000, 100, 75, 33, bg1)
        got = _check_exact(sc, behind, (0.5, 0.2, 0.0))
        assert got[0.5] == 100 * 75 and got[0.2] == (100 * 75 if bg1 == 0.0 else 0)


@pytest.mark.parametrize("bg1", [0.3, -0.3])
def test_count_with_background(cuda, bg1):
    """bg[1] = 0.3: the early exit stays exact (the background term only raises the value); -0.3: it could lower
    the value again, so the kernel walks to the forward's own termination."""
    _, sc = _scorer(3000, 128, 96, 32, bg1)
    got = _check_exact(sc, torch.eye(4, device=cuda), (0.5, 0.99, 0.31, 0.0, -0.1, 1.5))
    assert 0 < got[0.5] < 128 * 96


def test_count_against_cpu_oracle(cuda):
    """#(s < thres - d) <= count <= #(s < thres + d), s the oracle's channel-1 image of the same rendervars and
    d = 1e-4 max(1, |s|) the forward-image tolerance of tests/test_gpu_configs.py.  Identity pose: the
    camera-frame points are then the scene's bits.  Not vacuous: the band holds at most 1 % of the pixels and
    the oracle's own count is neither 0 nor W H (seed 32: 2690 / 12266 of 12288 at 0.5 / 0.99, 1 band pixel)."""
    scene, sc = _scorer(3000, 128, 96, 32)
    z = scene.means3D[:, 2:3]
    rv = Scene(means3D=scene.means3D, scales=sc.scales.cpu(), rotations=sc.rotations.cpu(),
               opacities=sc.opacities.cpu(), colors=torch.cat([z, torch.ones_like(z), z * z], 1), shs=None,
               sh_degree=0, cam=scene.cam)
    fr, _ = harness.run_oracle(rv, backward=False)
    s = fr.color[1].astype(np.float64)
    d = 1e-4 * np.maximum(1.0, np.abs(s))
    for thres in (0.5, 0.99):
        lo, hi, mid = int((s < thres - d).sum()), int((s < thres + d).sum()), int((s < thres).sum())
        band = int((np.abs(s - thres) <= d).sum())
        got = int(silhouette_count(sc, torch.eye(4, device=cuda), thres))
        print(f"thres {thres}: oracle {lo} <= {mid} <= {hi} (band {band}), count {got}")
        assert band <= 0.01 * s.size and 0 < mid < s.size
        assert lo <= got <= hi


def test_count_after_dynamic_and_static_forward(cuda):
    """The count does not depend on which forward produced the buffers."""
    from splatam_amd import _C
    _, sc = _scorer(3000, 128, 96, 32)
    cam = sc.cam
    w2c = _pose(3.0, [0.02, -0.01, 0.05]).to(cuda)
    e = torch.Tensor([])
    with torch.no_grad():
        pts = camera_points(sc.params["means3D"], w2c)
        args = (cam.bg, pts, sc.colors, sc.opacities, sc.scales, sc.rotations, cam.scale_modifier, e, cam.viewmatrix,
                cam.projmatrix, cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, e, cam.sh_degree,
                cam.campos, cam.prefiltered)
        dyn = _C.rasterize_gaussians(*args)
        status = torch.zeros(4, dtype=torch.int32, device=cuda)
        sta = _C.rasterize_gaussians(*args, capacity=dyn[0] + 1000, status=status)
        out = torch.zeros(2, 2, dtype=torch.int32, device=cuda)
        for i, thres in enumerate((0.5, 0.99)):
            _count_into(cam, pts.shape[0], dyn[0], dyn[3], dyn[4], dyn[5], thres, out[0, i:i + 1])
            _count_into(cam, pts.shape[0], sta[0], sta[3], sta[4], sta[5], thres, out[1, i:i + 1])
    assert int(status[0]) == dyn[0]
    assert torch.equal(out[0], out[1]) and 0 < int(out[0, 0]) < int(out[0, 1])
    assert int(out[0, 0]) == int(silhouette_count(sc, w2c, 0.5))


def test_batched_gains(cuda):
    """mode "gains": K = 4 over 6 poses (two replays, the second padded and with other poses): the counts are the
    eager silhouette_count's, g_eig is bitwise mode "scores"', the columns are send_gains' formula of the two."""
    _, sc = _scorer(3000, 96, 72, 22)
    poses = [_pose(d, [0.01 * d, -0.005 * d, 0.02]).to(cuda) for d in (-4.0, -2.0, 0.0, 1.5, 3.0, 12.0)]
    K, npix = 4, 96 * 72
    hinv = sc.fit_visited(poses[:3])
    bsc = BatchedFisher(sc, K, mode="scores", probe_w2cs=poses)
    eig = torch.cat([bsc.scores(poses[:4], hinv).clone(), bsc.scores(poses[4:], hinv).clone()])
    bg = BatchedFisher(sc, K, mode="gains", probe_w2cs=poses)
    cnt = [int(silhouette_count(sc, w, 0.5)) for w in poses]
    assert len(set(cnt)) > 1 and all(0 < c < npix for c in cnt), cnt
    raw = torch.cat([bg.gains(poses[:4], hinv).clone(), bg.gains(poses[4:], hinv).clone()])
    assert raw.dtype == torch.float64 and raw.shape == (6, 3)
    assert torch.equal(raw[:, 1], eig)                                   # bitwise "scores"
    assert raw[:, 0].tolist() == [c / npix for c in cnt]
    assert not bg.overflowed()
    for nl in (False, True):
        w = dict(k_sil=250.0, k_eig=0.3, k_sum=2.5, nl_sil=nl, nl_eig=nl)
        got = torch.cat([bg.gains(poses[:4], hinv, **w).clone(), bg.gains(poses[4:], hinv, **w).clone()]).cpu()
        assert bg.counts[:2].tolist() == cnt[4:]                          # the second replay's own poses
        for i in range(6):
            want = _restated(cnt[i], float(eig[i]), npix, 250.0, 0.3, 2.5, nl, nl)
            for c in range(3):  # (the tolerance of tests/test_viewgain_cpu.py: exact without the non-linear map)
                assert abs(float(got[i, c]) - want[c]) <= (5e-12 if nl else 0.0) * max(1.0, abs(want[c])), (i, c)
        # the rank-sharded form (one rank): the same rows with and without the batch
        assert torch.equal(sc.view_gains(poses, batch=bg, **w).cpu(), got)
        assert torch.equal(sc.view_gains(poses, **w).cpu(), got)


def test_batched_gains_capacity_overflow(cuda):
    """A binning capacity too small for a pose: gains() returns None, nothing faults (the count kernel does not
    walk the invalid lists) and the status rows report it."""
    _, sc = _scorer(3000, 96, 72, 22)
    behind = torch.eye(4, device=cuda)
    behind[2, 3] = -100.0  # sees nothing
    bg = BatchedFisher(sc, 2, mode="gains", headroom=0.5, min_extra=0)  # half of what the identity pose needs
    hinv = torch.ones(3000, 4, device=cuda)
    assert bg.gains([torch.eye(4, device=cuda)], hinv) is None
    torch.cuda.synchronize()
    assert bg.overflowed(1) and int(bg.status[0, 0]) > bg.capacity
    g = bg.gains([behind, behind], hinv)  # a pose that fits still scores afterwards
    assert g is not None and torch.equal(g[:, 0], torch.ones(2, dtype=torch.float64, device=cuda))
