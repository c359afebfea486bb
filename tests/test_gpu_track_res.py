"""A tracking resolution of its own (the reference's tracking_image_height / width, "SplaTAM-S") in both
sequence loops: track_frames / track_cam, and track_size / densify_size, under which the sequence makes its small
frames with gsr_resize_frame.

The capture is tests/test_gpu_sequence.py's form (workloads.sequence_workload, copied here) at 64x48 with 6000
Gaussians and four frames.  Two things differ, both so that a half-resolution tracker has a frame it can follow:
the Gaussians lie in a slab (depths 1.9 .. 2.1 m, twice make_scene's radius) rather than at random depths of
0.5 .. 5 m -- a nearest-neighbour depth of a random cloud is not the depth its render has at another resolution --
and the trajectory accelerates (x_t = 0.01 t (t + 1) m, a roll of 0.15 t (t + 1) degrees about z, which a
translation cannot stand in for), so that the constant-velocity initialisation is off by about 2 cm and 0.3
degrees in every frame and tracking has something to correct.  Tracking at 32x24 is 2 x 1.5 tiles: a partial tile
row in the tracker only."""
import math

import numpy as np
import pytest
import torch

from splatam_amd import resize as rz
from splatam_amd.mapper import GAUSS_KEYS
from splatam_amd.scenes import make_scene
from splatam_amd.sequence import PerFrameSlam, SlamSequence, initialize_camera_pose
from splatam_amd.slam import TrackingConfig

pytestmark = pytest.mark.gpu

W, H, N_FRAMES = 64, 48, 4
SMALL = (24, 32)
ITERS = dict(tracking_iters=40, track_replay=20, mapping_iters=10)
WINDOW = dict(keyframe_policy="window", keyframe_every=2, window=3)
OVERLAP = dict(keyframe_policy="overlap", keyframe_every=2, window=3, overlap_pixels=200)
POSE_KEYS = ("cam_unnorm_rots", "cam_trans")


def _workload(scene, num_frames, dev, hole=0.2):
    """workloads.sequence_workload with the accelerating trajectory of this module's docstring."""
    from splatam_amd.rasterizer import GaussianRasterizer
    from splatam_amd.slam import camera_settings, init_tracking_params, transform_to_frame, \
        transformed_params2depthplussilhouette
    from splatam_amd.workloads import render_targets
    truth = init_tracking_params(scene, num_frames=num_frames, device=dev)
    cam = camera_settings(scene.cam, dev)
    w2c = torch.eye(4, device=dev)
    gt = dict(truth)
    q = torch.zeros(1, 4, num_frames, device=dev)
    tr = torch.zeros(1, 3, num_frames, device=dev)
    for t in range(num_frames):
        a = math.radians(0.15 * t * (t + 1))
        q[0, 0, t], q[0, 3, t] = math.cos(a / 2), math.sin(a / 2)
        tr[0, 0, t] = 0.01 * t * (t + 1)
    gt["cam_unnorm_rots"], gt["cam_trans"] = q, tr
    g = torch.Generator().manual_seed(99)
    frames = []
    for t in range(num_frames):
        im, _ = render_targets(truth, cam, w2c, t, perturb=gt)
        with torch.no_grad():
            tg = transform_to_frame(gt, t, False, False)
            ds, _, _ = GaussianRasterizer(cam)(**transformed_params2depthplussilhouette(gt, w2c, tg))
            sil = ds[1:2]
            depth = torch.where(sil > 0.5, ds[0:1] / sil.clamp_min(1e-6), torch.zeros_like(sil))
        depth = depth * (1.0 + 0.01 * torch.randn(depth.shape, generator=g).to(dev))
        frames.append({"im": im.clamp(0, 1).contiguous(), "depth": depth.contiguous()})
    c = scene.cam
    u = truth["means3D"][:, 0] / truth["means3D"][:, 2] * c.fx + c.cx
    keep = u >= hole * c.W
    params = {k: (v[keep].contiguous() if v.shape[0] == keep.shape[0] and k not in POSE_KEYS else v.clone())
              for k, v in truth.items()}
    params["cam_unnorm_rots"][..., 0] = q[..., 0]
    params["cam_trans"][..., 0] = tr[..., 0]
    return params, frames, cam, w2c, (c.fx, c.fy, c.cx, c.cy), (q, tr)


class Capture:
    def __init__(self, dev):
        from splatam_amd.tracker import probe_num_rendered
        self.dev = dev
        scene = make_scene(6000, W, H, seed=7, z_range=(1.9, 2.1))
        scene.scales = scene.scales * 2.0
        self.params, self.frames, self.cam, self.w2c, self.intr, self.gt = _workload(scene, N_FRAMES, dev)
        n, _ = probe_num_rendered(self.params, {"cam": self.cam, "w2c": self.w2c, **self.frames[0]}, 0)
        self.bin_cap = 4 * n + 100_000
        self.P0 = self.params["means3D"].shape[0]
        self.small = [rz.resize_device(f, SMALL) for f in self.frames]
        self.small_cam = rz.resized_camera(W, H, self.intr, *SMALL, dev)

    def sequence(self, frames=None, **kw):
        kw = dict(dict(ITERS, prune=False, seed=0, **WINDOW), **kw)
        capacity = kw.pop("capacity", self.P0 + 2 * W * H)
        return SlamSequence(kw.pop("params", self.params), self.frames if frames is None else frames, self.cam,
                            self.w2c, self.intr, capacity=capacity, bin_capacity=self.bin_cap, **kw)

    def tracked_small(self):
        return dict(track_frames=self.small, track_cam=self.small_cam)


def _run(seq, n=N_FRAMES, before=None):
    """frame(0 .. n - 1); the poses initialize_camera_pose gives each tracked frame, as (q, t) pairs."""
    inits = {}
    for t in range(n):
        if before is not None:
            before(seq, t)
        if t > 0:
            p = {k: seq.params[k].detach().clone() for k in POSE_KEYS}
            initialize_camera_pose(p, t)
            inits[t] = (p["cam_unnorm_rots"][0, :, t].clone(), p["cam_trans"][0, :, t].clone())
        seq.frame(t)
    seq.check()
    torch.cuda.synchronize()
    return inits


def _same_state(a: SlamSequence, b: SlamSequence):
    for k in POSE_KEYS:
        assert torch.equal(a.params[k], b.params[k]), k
    assert torch.equal(a.n_live, b.n_live) and int(a.alive.sum()) == int(b.alive.sum()) == int(a.n_live.item())
    la, lb = a.live_params(), b.live_params()
    for k in GAUSS_KEYS + ("rgb_colors",):
        assert torch.equal(la[k], lb[k]), k
    assert len(a.draws) == len(b.draws)
    for x, y in zip(a.draws, b.draws):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert a.tracking_iters_run == b.tracking_iters_run


def _pose_error(q, tr, gt, t):
    """(rotation angle in degrees, translation distance in metres) of pose (q, tr) from the true pose of frame t."""
    q_gt, t_gt = gt[0][0, :, t], gt[1][0, :, t]
    qn = torch.nn.functional.normalize(q.double(), dim=0)
    dot = float((qn * q_gt.double()).sum().abs().clamp(max=1.0))
    return math.degrees(2.0 * math.acos(dot)), float((tr.double() - t_gt.double()).norm())


@pytest.fixture(scope="module")
def cap(cuda):
    return Capture(torch.device(cuda))


@pytest.fixture(scope="module")
def full_run(cap):
    seq = cap.sequence()
    return seq, _run(seq)


@pytest.fixture(scope="module")
def small_run(cap):
    seq = cap.sequence(**cap.tracked_small())
    return seq, _run(seq)


def test_same_resolution_is_the_plain_sequence(cap, full_run):
    plain, _ = full_run
    seq = cap.sequence(track_frames=cap.frames, track_cam=cap.cam)
    _run(seq)
    _same_state(seq, plain)
    assert int(seq.n_live.item()) - cap.P0 > 100  # the hole was densified


def test_own_resolution_in_both_loops(cap):
    seq = cap.sequence(**cap.tracked_small(), **OVERLAP)
    _run(seq)
    ref = PerFrameSlam(cap.params, cap.frames, cap.cam, cap.w2c, cap.intr, bin_capacity=cap.bin_cap, prune=False,
                       **ITERS, **OVERLAP, **cap.tracked_small())
    for t in range(N_FRAMES):
        ref.frame(t, seq.draws[t])
    torch.cuda.synchronize()
    for k in POSE_KEYS:
        assert torch.equal(seq.params[k], ref.p[k]), k
    live = seq.live_params()
    assert live["means3D"].shape[0] == ref.p["means3D"].shape[0] > cap.P0 + 100
    for k in GAUSS_KEYS + ("rgb_colors",):
        assert torch.equal(live[k], ref.p[k]), k
    assert ref.tracking_iters_run == seq.tracking_iters_run == [0] + [ITERS["tracking_iters"]] * (N_FRAMES - 1)
    # the tracker alone sees the small frame
    sc = seq.slot_curr
    assert sc["im"].shape == (3, *SMALL) and sc["depth"].shape == (1, *SMALL) and sc["cam"] is cap.small_cam
    assert (sc["cam"].image_height, sc["cam"].image_width) == SMALL and sc["w2c"] is cap.w2c
    assert torch.equal(sc["im"], cap.small[N_FRAMES - 1]["im"]) and seq.tracker.curr is sc
    assert all(kf["im"].shape == (3, H, W) and kf["cam"] is cap.cam for kf in seq.keyframes + [seq._kf(2)])
    assert seq.bank.im.shape[1:] == (3, H, W) and seq.bank.depth.shape[1:] == (1, H, W) and seq.bank.n >= 2
    assert seq._densify_kf(1)[0]["im"].shape == (3, H, W)
    out = seq.evaluate(ms_ssim=False)
    assert out["table"].shape == (N_FRAMES, 8)
    n_valid = [int((f["depth"] > 0).sum()) for f in cap.frames]  # the full frames' measured pixels
    assert [int(v) for v in out["table"][:, 4].cpu()] == n_valid and min(n_valid) > 0


def test_tracking_moves_towards_the_true_pose(cap, full_run, small_run):
    """Every tracked frame ends no farther from its true pose than initialize_camera_pose left it, in rotation
    and in translation, and strictly closer in one of them: first at the full resolution (the capture is one
    where that holds at all), then at 32x24."""
    for name, (seq, inits) in (("full", full_run), ("32x24", small_run)):
        for t in range(1, N_FRAMES):
            r0, d0 = _pose_error(*inits[t], cap.gt, t)
            r1, d1 = _pose_error(seq.params["cam_unnorm_rots"][0, :, t], seq.params["cam_trans"][0, :, t], cap.gt, t)
            print(f"{name} frame {t}: rotation {r0:.4f} -> {r1:.4f} deg, translation {d0:.5f} -> {d1:.5f} m")
    for name, (seq, inits) in (("full", full_run), ("32x24", small_run)):
        for t in range(1, N_FRAMES):
            r0, d0 = _pose_error(*inits[t], cap.gt, t)
            r1, d1 = _pose_error(seq.params["cam_unnorm_rots"][0, :, t], seq.params["cam_trans"][0, :, t], cap.gt, t)
            assert r1 <= r0 and d1 <= d0 and (r1 < r0 or d1 < d0), (name, t)


def test_the_tracker_reads_the_small_frame_alone(cap, small_run):
    base, _ = small_run
    t = 2
    # (a) another tracking depth for frame t: its pose changes
    small = [dict(f) for f in cap.small]
    small[t] = {"im": small[t]["im"], "depth": (small[t]["depth"] * 1.25).contiguous()}
    seq = cap.sequence(track_frames=small, track_cam=cap.small_cam)
    _run(seq, t + 1)
    for k in POSE_KEYS:
        assert torch.equal(seq.params[k][..., :t], base.params[k][..., :t]), k
    assert not torch.equal(seq.params["cam_trans"][..., t], base.params["cam_trans"][..., t])
    # (b) another full-resolution image for frame t: neither that pose nor the iterations run change
    frames = [dict(f) for f in cap.frames]
    frames[t] = {"im": (1.0 - frames[t]["im"]).contiguous(), "depth": frames[t]["depth"]}
    seq = cap.sequence(frames=frames, **cap.tracked_small())
    _run(seq, t + 1)
    for k in POSE_KEYS:
        assert torch.equal(seq.params[k][..., :t + 1], base.params[k][..., :t + 1]), k
    assert seq.tracking_iters_run == base.tracking_iters_run[:t + 1]


def test_sizes_make_the_frames(cap):
    """track_size (40x30: no integer ratio) and densify_size (32x24) with full frames pushed, against the frames
    made beforehand by resize_device and handed over."""
    tsize, dsize = (30, 40), SMALL
    made = [rz.resize_device(f, tsize, dsize) for f in cap.frames]
    given = cap.sequence(densify_mode="device", track_frames=[m[0] for m in made],
                         track_cam=rz.resized_camera(W, H, cap.intr, *tsize, cap.dev),
                         densify_frames=[m[1] for m in made],
                         densify_cam=rz.resized_camera(W, H, cap.intr, *dsize, cap.dev),
                         densify_intrinsics=rz.scale_intrinsics(cap.intr, H, W, *dsize))
    _run(given)
    fed = cap.sequence(frames=cap.frames[:1], num_frames=N_FRAMES, densify_mode="device", track_size=tsize,
                       densify_size=dsize)
    fed.frame(0)
    assert [fed.push(f["im"], f["depth"]) for f in cap.frames[1:]] == list(range(1, N_FRAMES))
    fed.check()
    torch.cuda.synchronize()
    _same_state(fed, given)
    assert len(fed.track_frames) == len(fed.densify_frames) == N_FRAMES
    for t in range(N_FRAMES):
        for got, want in ((fed.track_frames[t], made[t][0]), (fed.densify_frames[t], made[t][1])):
            assert torch.equal(got["im"], want["im"]) and torch.equal(got["depth"], want["depth"])
    assert fed.slot_curr["im"].shape == (3, *tsize) and fed.densify_intrinsics == given.densify_intrinsics
    with pytest.raises(ValueError):
        fed.push_frames(cap.frames[0]["im"], cap.frames[0]["depth"], track_frame=made[0][0])  # the sequence makes it
    # either size alone, and the per-frame loop, make the same frames
    only_t = PerFrameSlam(cap.params, cap.frames, cap.cam, cap.w2c, cap.intr, track_size=tsize)
    only_d = PerFrameSlam(cap.params, cap.frames, cap.cam, cap.w2c, cap.intr, densify_size=dsize)
    assert only_t.densify_frames is None and only_d.track_frames is None
    for t in range(N_FRAMES):
        assert torch.equal(only_t.track_frames[t]["im"], made[t][0]["im"])
        assert torch.equal(only_d.densify_frames[t]["depth"], made[t][1]["depth"])
    # a capture with track_frames takes one per pushed frame
    fed2 = cap.sequence(frames=cap.frames[:1], num_frames=N_FRAMES, track_frames=cap.small[:1], track_cam=cap.small_cam)
    fed2.frame(0)
    with pytest.raises(ValueError):
        fed2.push(cap.frames[1]["im"], cap.frames[1]["depth"])
    assert fed2.push_frames(cap.frames[1]["im"], cap.frames[1]["depth"], track_frame=cap.small[1]) == 1


def test_rebuild_carries_the_tracking_slot(cap, small_run):
    base, _ = small_run
    seq = cap.sequence(capacity=cap.P0 + 50, **cap.tracked_small())
    grew = []
    _run(seq, before=lambda s, t: grew.append(s.ensure_headroom(W * H)))
    print(f"ensure_headroom grew {grew}; capacity {seq.capacity}")
    assert sum(grew) >= 1 and seq.capacity > cap.P0 + 50
    assert seq.slot_curr["im"].shape == (3, *SMALL) and seq.slot_curr["cam"] is cap.small_cam
    _same_state(seq, base)


def test_depth_loss_threshold_follows_the_tracking_resolution(cap):
    """use_depth_loss_thres compares the depth loss summed over the tracking frame's pixels: with a threshold
    between frame 1's depth terms at the two resolutions (printed), the sequence whose term is the larger one
    extends the frame and the other does not."""
    S, n = ITERS["track_replay"], ITERS["tracking_iters"]

    def run(thres, **kw):
        seq = cap.sequence(track_cfg=TrackingConfig(use_depth_loss_thres=True, depth_loss_thres=thres), **kw)
        _run(seq, 2)
        return seq, float(seq.tracker.terms[S - 1, 1])
    _, d_full = run(float("inf"))
    _, d_small = run(float("inf"), **cap.tracked_small())
    print(f"frame 1's depth term: {d_full!r} at {W}x{H}, {d_small!r} at {SMALL[1]}x{SMALL[0]}")
    assert d_small > 0 and d_full > 0 and d_small != d_full
    thres = 0.5 * (d_full + d_small)
    full, _ = run(thres)
    small, _ = run(thres, **cap.tracked_small())
    print(f"threshold {thres!r}: iterations {full.tracking_iters_run} at {W}x{H}, {small.tracking_iters_run} at 32x24")
    extended, kept = (full, small) if d_full > d_small else (small, full)
    assert extended.tracking_iters_run == [0, 2 * n] and kept.tracking_iters_run == [0, n]
