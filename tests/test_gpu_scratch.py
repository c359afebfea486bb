"""The glue reductions' scratch contract (include/gsr_glue.h) and their grid edges.

Five kernels finish a fixed-order reduction through a caller-supplied float scratch: the pose sums of
gsr_track_transform_bwd(_adam) (1), the tracking L1 of gsr_track_l1_fwd(_bwd) (2), the render-epilogue L1 of
gsr_track_forward_dual_static (3), the pose-fused per-Gaussian backward of gsr_track_backward_dual (4) and
gsr_map_loss_fwd (5).  The header promises that one zero-filled buffer of at least the queried size serves
any of them, in any order, on one stream.  The tests below call the C ABI with buffers they own:

* every pair of users whose size queries coincide shares one buffer of exactly that size (what
  splatam_amd.glue._scratch hands out), and all five share one buffer of the largest size; each output is
  bitwise what the same call gives with a private, freshly zeroed scratch, and the arrival counters (the
  scratch's first 272 words) are zero afterwards;
* the same through splatam_amd.glue (tracking_l1 + track_transform's backward), eagerly and in a HIP graph;
* users 1, 2 and 5 against float64 restatements at the grid sizes where the reductions change shape
  (1 workgroup, the 16 arrival groups' boundary, the 256 / 1024 workgroup caps, ragged SSIM tiles of both
  heights);
* the tracking L1 mask's NaN / threshold / sign edges.

Every output is filled with NaN before the call that writes it: a result that was never stored fails.
"""
import ctypes
import functools

import pytest
import torch

from splatam_amd import slam
from splatam_amd._lib import lib

pytestmark = pytest.mark.gpu

COUNTER_WORDS = 272  # include/gsr_glue.h: the arrival counters are the scratch's first 272 words
SIL_THRES, W_IM, W_DEPTH = 0.99, 0.5, 1.0
ROUND_SCALE = (1.0, 0.75, 1.25, 0.5, 1.5)  # one input is scaled per round: a stale output differs from the right one
NAN = float("nan")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ok(rc, what):
    assert rc >= 0, (what, lib.gsr_last_error().decode(errors="replace"))


def _nan(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# ------------------------------------------------------------------ inputs --
def _l1_images(H, W, seed=5):
    """im, depth_sil (depth, silhouette, depth^2), gt_im, gt_depth on the CPU; about half the pixels masked in
    by the silhouette, a stripe of invalid gt depth."""
    g = torch.Generator().manual_seed(seed)
    im, gt_im = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    depth = 0.5 + 4 * torch.rand(H, W, generator=g)
    sil = 0.98 + 0.02 * torch.rand(H, W, generator=g)
    ds = torch.stack([depth, sil, depth * depth + 0.01 * torch.rand(H, W, generator=g)])
    gt_d = (depth + 0.3 * torch.randn(H, W, generator=g)).clamp_min(0)[None]
    gt_d[:, :, : max(W // 7, 0)] = 0.0
    return im, ds, gt_im, gt_d


def _l1_reference(im, ds, gt_im, gt_d, thres=SIL_THRES, w_im=W_IM, w_depth=W_DEPTH, seed=1.0):
    """include/gsr_glue.h's formula: the float64 loss and the exact float32 gradient images (sign-based) on
    the CPU.  The mask is decided on the float32 values, as the kernel decides it."""
    thres32 = torch.tensor(thres, dtype=torch.float32)
    mask = (gt_d[0] > 0) & ~torch.isnan(ds[0]) & ~torch.isnan(ds[2] - ds[0] * ds[0]) & (ds[1] > thres32)
    m64 = mask.double()
    r_im = torch.nan_to_num((gt_im.double() - im.double()).abs()) * m64
    r_d = torch.nan_to_num((gt_d[0].double() - ds[0].double()).abs()) * m64
    loss = w_im * r_im.sum() + w_depth * r_d.sum()
    f32 = torch.float32  # the kernel forms seed * weight in float32
    s_im = torch.tensor(seed, dtype=f32) * torch.tensor(w_im, dtype=f32)
    s_d = torch.tensor(seed, dtype=f32) * torch.tensor(w_depth, dtype=f32)
    dim = torch.where(mask[None].expand(3, -1, -1), -s_im * torch.sign(gt_im - im), torch.zeros(()))
    dds = torch.zeros_like(ds)
    dds[0] = torch.where(mask, -s_d * torch.sign(gt_d[0] - ds[0]), torch.zeros(()))
    return float(loss), dim, dds, mask


def _call_l1_fwd_bwd(dev, im, ds, gt_im, gt_d, scratch, seed, thres=SIL_THRES):
    H, W = im.shape[1:]
    loss, dim, dds = _nan(dev), _nan(dev, 3, H, W), _nan(dev, 3, H, W)
    _ok(lib.gsr_track_l1_fwd_bwd(H, W, im.data_ptr(), ds.data_ptr(), gt_im.data_ptr(), gt_d.data_ptr(), thres, W_IM,
                                 W_DEPTH, seed.data_ptr(), loss.data_ptr(), dim.data_ptr(), dds.data_ptr(),
                                 scratch.data_ptr(), _stream(dev)), "track_l1_fwd_bwd")
    return loss, dim, dds


def _call_l1_fwd(dev, im, ds, gt_im, gt_d, scratch, thres=SIL_THRES):
    H, W = im.shape[1:]
    loss = _nan(dev)
    _ok(lib.gsr_track_l1_fwd(H, W, im.data_ptr(), ds.data_ptr(), gt_im.data_ptr(), gt_d.data_ptr(), thres, W_IM,
                             W_DEPTH, loss.data_ptr(), scratch.data_ptr(), _stream(dev)), "track_l1_fwd")
    return loss


def _call_l1_bwd(dev, im, ds, gt_im, gt_d, seed, thres=SIL_THRES):
    H, W = im.shape[1:]
    dim, dds = _nan(dev, 3, H, W), _nan(dev, 3, H, W)
    _ok(lib.gsr_track_l1_bwd(H, W, im.data_ptr(), ds.data_ptr(), gt_im.data_ptr(), gt_d.data_ptr(), thres, W_IM,
                             W_DEPTH, seed.data_ptr(), dim.data_ptr(), dds.data_ptr(), _stream(dev)), "track_l1_bwd")
    return dim, dds


def _pose_inputs(P, scols, seed=11):
    """World-frame map, a strided pose column (t = 1 of T = 2, so q_stride = 2), a non-identity w2c and the
    upstream gradients of (means_cam, rotations, depth colours), on the CPU.  The upstream gradients carry a
    mean, so the 16 sums do not cancel to nothing."""
    g = torch.Generator().manual_seed(seed + 7 * scols)
    p = {"means3D": torch.randn(P, 3, generator=g) + torch.tensor([0.0, 0.0, 3.0]),
         "unnorm_rotations": torch.randn(P, 4, generator=g),
         "logit_opacities": torch.randn(P, 1, generator=g),
         "log_scales": -3.0 + 0.3 * torch.randn(P, scols, generator=g),
         "cam_unnorm_rots": torch.tensor([[[1.0, 0.9], [0.0, 0.12], [0.0, -0.2], [0.0, 0.31]]]),
         "cam_trans": torch.tensor([[[0.0, 0.05], [0.0, -0.1], [0.0, 0.2]]])}
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.05, -0.02, 0.1])
    ups = [0.5 + torch.randn(P, 3, generator=g), 0.3 + torch.randn(P, 4, generator=g),
           0.2 + torch.randn(P, 3, generator=g)]
    return p, w2c, ups


def _pose_reference(p, w2c, ups, t=1):
    """Autograd through slam.transform_to_frame and the rendervar builders in float64."""
    pr = {k: v.double() for k, v in p.items()}
    pr["cam_unnorm_rots"].requires_grad_(True)
    pr["cam_trans"].requires_grad_(True)
    tg = slam.transform_to_frame(pr, t, gaussians_grad=False, camera_grad=True, fast=False)
    rv = slam.transformed_params2rendervar(pr, tg)
    dv = slam.transformed_params2depthplussilhouette(pr, w2c.double(), tg, fast=False)
    total = (rv["means3D"] * ups[0].double()).sum() + (dv["colors_precomp"] * ups[2].double()).sum()
    if p["log_scales"].shape[1] != 1:  # an isotropic map's rotations do not depend on the pose
        total = total + (rv["rotations"] * ups[1].double()).sum()
    total.backward()
    return pr["cam_unnorm_rots"].grad[0, :, t], pr["cam_trans"].grad[0, :, t]


class _Pose:
    """User 1: gsr_track_transform_bwd and _bwd_adam on one map."""

    def __init__(self, dev, P, scols=3):
        self.dev, self.P, self.scols, self.t, self.T = dev, P, scols, 1, 2
        p, w2c, ups = _pose_inputs(P, scols)
        self.cpu = (p, w2c, ups)
        self.p = {k: v.to(dev).contiguous() for k, v in p.items()}
        self.w2c = w2c.to(dev)
        self.ups = [u.to(dev) for u in ups]
        self.n = lib.gsr_track_scratch_floats(P)
        f = functools.partial(_nan, dev)
        self.means_cam, rot, dcol, opac, scl = f(P, 3), f(P, 4), f(P, 3), f(P, 1), f(P, 3)
        q, tr = self.p["cam_unnorm_rots"], self.p["cam_trans"]
        _ok(lib.gsr_track_transform_fwd(P, self.p["means3D"].data_ptr(), self.p["unnorm_rotations"].data_ptr(),
                                        self.p["logit_opacities"].data_ptr(), self.p["log_scales"].data_ptr(), scols,
                                        q.data_ptr() + 4 * self.t, tr.data_ptr() + 4 * self.t, self.T,
                                        self.w2c.data_ptr(), self.means_cam.data_ptr(), rot.data_ptr(),
                                        dcol.data_ptr(), opac.data_ptr(), scl.data_ptr(), _stream(dev)), "transform_fwd")

    def grad(self, scratch, scale=1.0):
        dev, t, T, p = self.dev, self.t, self.T, self.p
        gm, gr, gd = [u * scale for u in self.ups]
        dq, dt = _nan(dev, 1, 4, T), _nan(dev, 1, 3, T)
        _ok(lib.gsr_track_transform_bwd(self.P, p["means3D"].data_ptr(), p["unnorm_rotations"].data_ptr(), self.scols,
                                        p["cam_unnorm_rots"].data_ptr() + 4 * t, self.means_cam.data_ptr(),
                                        self.w2c.data_ptr(), gm.data_ptr(), gr.data_ptr(), gd.data_ptr(),
                                        dq.data_ptr() + 4 * t, dt.data_ptr() + 4 * t, T, scratch.data_ptr(),
                                        _stream(dev)), "transform_bwd")
        torch.cuda.synchronize()
        assert bool(torch.isnan(dq[0, :, 0]).all()) and bool(torch.isnan(dt[0, :, 0]).all())  # column 0 untouched
        return dq[0, :, t].clone(), dt[0, :, t].clone()

    def run(self, scratch, rnd):
        dev, t, T, p = self.dev, self.t, self.T, self.p
        dq, dt = self.grad(scratch, ROUND_SCALE[rnd])
        # the in-place Adam variant: on a snapshot of the pose, from fresh optimizer state
        gm, gr, gd = [u * ROUND_SCALE[rnd] for u in self.ups]
        q, tr = p["cam_unnorm_rots"].clone(), p["cam_trans"].clone()
        state = torch.zeros(15, dtype=torch.float32, device=dev)
        _ok(lib.gsr_track_transform_bwd_adam(self.P, p["means3D"].data_ptr(), p["unnorm_rotations"].data_ptr(),
                                             self.scols, q.data_ptr() + 4 * t, tr.data_ptr() + 4 * t, T,
                                             self.means_cam.data_ptr(), self.w2c.data_ptr(), gm.data_ptr(),
                                             gr.data_ptr(), gd.data_ptr(), 0.0004, 0.002, 0.9, 0.999, 1e-8,
                                             state.data_ptr(), scratch.data_ptr(), None, _stream(dev)),
            "transform_bwd_adam")
        torch.cuda.synchronize()
        # a step that was never applied leaves the snapshot: it must have moved
        assert not torch.equal(q, p["cam_unnorm_rots"]) and not torch.equal(tr, p["cam_trans"])
        assert float(state[14]) == 1.0
        return dq, dt, q, tr, state


class _L1:
    """User 2: gsr_track_l1_fwd_bwd and gsr_track_l1_fwd."""

    def __init__(self, dev, H, W):
        self.dev, self.H, self.W = dev, H, W
        self.im, self.ds, self.gt_im, self.gt_d = [x.to(dev) for x in _l1_images(H, W)]
        self.n = lib.gsr_track_scratch_floats(H * W)
        self.seed = torch.ones((), device=dev)

    def run(self, scratch, rnd):
        im = self.im * ROUND_SCALE[rnd]
        loss, dim, dds = _call_l1_fwd_bwd(self.dev, im, self.ds, self.gt_im, self.gt_d, scratch, self.seed)
        loss2 = _call_l1_fwd(self.dev, im, self.ds, self.gt_im, self.gt_d, scratch)
        return loss, dim, dds, loss2


class _Render:
    """Users 3 and 4 on one small scene: the render-epilogue L1 (gsr_track_forward_dual_static) and the
    pose-fused backward (gsr_track_backward_dual) of that forward."""

    def __init__(self, dev, P, W=160, H=120, aniso=True):
        from splatam_amd.scenes import make_scene
        self.dev, self.P, self.W, self.H = dev, P, W, H
        self.CAP = max(400000, 40 * P)  # binning capacity (tests/test_gpu_slam.py: 400000 for 5000 Gaussians)
        scene = make_scene(P, W, H, seed=3, anisotropic=aniso)
        self.params = slam.init_tracking_params(scene, num_frames=2, device=dev)
        self.cam = slam.camera_settings(scene.cam, dev)
        self.w2c = torch.eye(4, device=dev)
        p = self.params
        self.scols = p["log_scales"].shape[1]
        self.mw, self.ur = p["means3D"].detach().contiguous(), p["unnorm_rotations"].detach().contiguous()
        self.rgb = p["rgb_colors"].detach().contiguous()
        f = functools.partial(_nan, dev)
        self.means, self.rot, self.dcol, self.opac, self.scl = f(P, 3), f(P, 4), f(P, 3), f(P, 1), f(P, 3)
        self.q, self.tr = p["cam_unnorm_rots"].detach().contiguous(), p["cam_trans"].detach().contiguous()
        self.t, self.T = 1, self.q.shape[-1]
        _ok(lib.gsr_track_transform_fwd(P, self.mw.data_ptr(), self.ur.data_ptr(),
                                        p["logit_opacities"].detach().contiguous().data_ptr(),
                                        p["log_scales"].detach().contiguous().data_ptr(), self.scols,
                                        self.q.data_ptr() + 4 * self.t, self.tr.data_ptr() + 4 * self.t, self.T,
                                        self.w2c.data_ptr(), self.means.data_ptr(), self.rot.data_ptr(),
                                        self.dcol.data_ptr(), self.opac.data_ptr(), self.scl.data_ptr(),
                                        _stream(dev)), "transform_fwd")
        g = torch.Generator().manual_seed(2)
        self.gt_im = torch.rand(3, H, W, generator=g).to(dev)
        self.gt_d = (2.0 + torch.rand(1, H, W, generator=g)).to(dev)
        self.seed = torch.ones((), device=dev)
        self.n_fwd = lib.gsr_track_forward_scratch_floats(W, H)
        self.n_bwd = lib.gsr_track_backward_scratch_floats(P)
        self._fwd_state = None

    def forward(self, scratch, gt_im=None, gt_d=None, thres=0.5):
        """gsr_track_forward_dual_static through the C ABI; every output NaN-filled first.  (thres 0.5: the
        small scene covers part of the image only.)"""
        from splatam_amd import _C
        dev, cam, P, H, W = self.dev, self.cam, self.P, self.H, self.W
        gt_im = self.gt_im if gt_im is None else gt_im
        gt_d = self.gt_d if gt_d is None else gt_d
        s, keep_s = _C._settings(cam.bg, cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy, H, W,
                                 cam.scale_modifier, cam.sh_degree, cam.prefiltered, dev)
        g, keep_g, _ = _C._gaussians(self.means, None, self.rgb, self.opac, self.scl, self.rot, None, dev)
        f = functools.partial(_nan, dev)
        out = {"im": f(3, H, W), "ds": f(3, H, W), "depth": f(1, H, W), "loss": f(), "dim": f(3, H, W),
               "dds": f(3, H, W), "radii": torch.empty(P, dtype=torch.int32, device=dev),
               "status": torch.zeros(4, dtype=torch.int32, device=dev)}
        _C._begin(dev)
        n = lib.gsr_track_forward_dual_static(
            ctypes.byref(s), ctypes.byref(g), self.dcol.data_ptr(), self.CAP, out["status"].data_ptr(),
            out["im"].data_ptr(), out["ds"].data_ptr(), out["depth"].data_ptr(), out["radii"].data_ptr(),
            gt_im.data_ptr(), gt_d.data_ptr(), thres, W_IM, W_DEPTH, self.seed.data_ptr(), out["loss"].data_ptr(),
            out["dim"].data_ptr(), out["dds"].data_ptr(), scratch.data_ptr(), _C._ALLOC_CB, None, _stream(dev))
        _ok(n, "track_forward_dual_static")
        out["n"], out["bufs"] = int(n), dict(_C._tls.buffers)
        _C._tls.buffers = {}
        torch.cuda.synchronize()
        assert int(out["status"][1]) == 0 and 0 < int(out["status"][0]) <= self.CAP
        return out

    def run_fwd(self, scratch, rnd):
        o = self.forward(scratch, gt_im=self.gt_im * ROUND_SCALE[rnd])
        return o["loss"], o["dim"], o["dds"]

    def run_bwd(self, scratch, rnd):
        from splatam_amd import _C
        dev, t, T = self.dev, self.t, self.T
        if self._fwd_state is None:  # one forward (private scratch) whose buffers every backward call reads
            self._fwd_state = self.forward(torch.zeros(self.n_fwd, dtype=torch.float32, device=dev))
        o = self._fwd_state
        dim, dds = o["dim"] * ROUND_SCALE[rnd], o["dds"] * ROUND_SCALE[rnd]
        dq, dt = _nan(dev, 1, 4, T), _nan(dev, 1, 3, T)
        _C.track_backward_dual(self.cam, self.means, o["radii"], self.rgb, self.dcol, self.scl, self.rot, dim, dds,
                               o["bufs"][0], o["n"], o["bufs"][1], o["bufs"][2], self.mw, self.ur, self.scols,
                               self.q.data_ptr() + 4 * t, self.tr.data_ptr() + 4 * t, T, self.w2c, scratch,
                               dq_ptr=dq.data_ptr() + 4 * t, dt_ptr=dt.data_ptr() + 4 * t)
        return dq[0, :, t].clone(), dt[0, :, t].clone()


class _View:
    """One user of a shared object (the render scene serves users 3 and 4)."""

    def __init__(self, n, run):
        self.n, self.run = n, run


def _map_images(H, W, seed=0):
    """tests/test_gpu_mapping.py's images, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    im = torch.rand(3, H, W, generator=g)
    gt = (im + 0.2 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    ds = torch.stack([0.5 + 4 * torch.rand(H, W, generator=g), torch.rand(H, W, generator=g), torch.zeros(H, W)])
    ds[2] = ds[0] * ds[0] + 0.01 * torch.rand(H, W, generator=g)
    gd = (ds[0:1] + 0.3 * torch.randn(1, H, W, generator=g)).clamp_min(0)
    gd[:, :, : W // 7] = 0.0
    if H > 3 and W > 5:
        ds[0, 3, 5] = NAN
    return im, ds, gt, gd


def _map_literal(im, ds, gt, gd, w_im=0.5, w_depth=1.0):
    """tests/test_gpu_mapping.py's literal loss (get_loss(mapping=True))."""
    depth, dsq = ds[0:1], ds[2:3]
    unc = (dsq - depth ** 2).detach()
    mask = ((gd > 0) & ~torch.isnan(depth) & ~torch.isnan(unc)).detach()
    l_d = torch.abs(gd - depth)[mask].mean()
    l_im = 0.8 * slam.l1_loss_v1(im, gt) + 0.2 * (1.0 - slam.calc_ssim(im, gt))
    return w_im * l_im + w_depth * l_d


def _map_rows(dev, H, W):
    """The SSIM tile height gsr_map_loss_fwd picks (csrc/gsr_mapping.hip map_loss_rows)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    cols = (W + 63) // 64
    b16, b32 = 3 * cols * ((H + 15) // 16), 3 * cols * ((H + 31) // 32)
    return 32 if (b16 > 3 * cus and b32 <= 2 * cus) else 16


class _MapLoss:
    """User 5: gsr_map_loss_fwd (+ gsr_map_loss_bwd from its state)."""

    def __init__(self, dev, H, W):
        self.dev, self.H, self.W = dev, H, W
        self.im, self.ds, self.gt, self.gd = [x.to(dev) for x in _map_images(H, W)]
        self.n = lib.gsr_map_loss_scratch_floats(H, W)
        self.seed = torch.ones((), device=dev)

    def call(self, scratch, im):
        dev, H, W = self.dev, self.H, self.W
        loss, state = _nan(dev), _nan(dev, lib.gsr_map_loss_state_floats(H, W))
        dim, dds = _nan(dev, 3, H, W), _nan(dev, 3, H, W)
        _ok(lib.gsr_map_loss_fwd(H, W, im.data_ptr(), self.ds.data_ptr(), self.gt.data_ptr(), self.gd.data_ptr(),
                                 0.5, 1.0, loss.data_ptr(), state.data_ptr(), scratch.data_ptr(), _stream(dev)),
            "map_loss_fwd")
        _ok(lib.gsr_map_loss_bwd(H, W, im.data_ptr(), self.ds.data_ptr(), self.gt.data_ptr(), self.gd.data_ptr(),
                                 0.5, 1.0, self.seed.data_ptr(), state.data_ptr(), dim.data_ptr(), dds.data_ptr(),
                                 _stream(dev)), "map_loss_bwd")
        return loss, dim, dds

    def run(self, scratch, rnd):
        return self.call(scratch, (self.im * ROUND_SCALE[rnd]).clamp(0, 1))


# -------------------------------------------------------- shared scratch --
def _find(query, target, preferred, scan):
    """The first size whose scratch query equals `target`: the expected one if the layout is the one this test
    was written against, else whatever the queries say now."""
    for c in list(preferred) + list(scan):
        if query(c) == target:
            return c
    raise AssertionError(f"no size with a scratch of {target} floats")


def _hw_for(target, preferred):
    scan = ((h, w) for w in (16, 50, 80, 96, 240) for h in range(1, 1200))
    return _find(lambda hw: lib.gsr_track_scratch_floats(hw[0] * hw[1]), target, [preferred], scan)


def _p_for(query, target, preferred):
    return _find(query, target, [preferred], range(1, 400000, 64))


@functools.lru_cache(maxsize=None)
def _render(dev, P):
    return _Render(dev, P)


@functools.lru_cache(maxsize=None)
def _map640(dev):
    """User 5 at the mapping config's 640x480, where map_loss_rows picks the 32-row tile on a 256-CU device
    (900 > 768 and 450 <= 512)."""
    return _MapLoss(dev, 480, 640)


def _pair(dev, name):
    """(user A, user B) with equal scratch queries."""
    if name == "pose200_l1":  # one workgroup each
        a = _Pose(dev, 200)
        return a, _L1(dev, *_hw_for(a.n, (12, 16)))
    if name == "pose5000_l1":  # 20 workgroups: uneven arrival groups
        a = _Pose(dev, 5000)
        return a, _L1(dev, *_hw_for(a.n, (64, 80)))
    if name == "epilogue_l1":  # 80 tiles x 2 partials = 10 workgroups x 16
        r = _render(dev, 3000)
        return _View(r.n_fwd, r.run_fwd), _L1(dev, *_hw_for(r.n_fwd, (48, 50)))
    if name == "posefused_l1":  # 16 * 20 + 528 = 16 * 36 + 272
        r = _render(dev, 5000)
        return _View(r.n_bwd, r.run_bwd), _L1(dev, *_hw_for(r.n_bwd, (96, 96)))
    m = _map640(dev)
    if name == "maploss_pose":
        return m, _Pose(dev, _p_for(lib.gsr_track_scratch_floats, m.n, 57600))
    if name == "maploss_l1":
        return m, _L1(dev, *_hw_for(m.n, (240, 240)))
    if name == "maploss_posefused":
        r = _render(dev, _p_for(lib.gsr_track_backward_scratch_floats, m.n, 53400))
        return m, _View(r.n_bwd, r.run_bwd)
    raise KeyError(name)


def _check_shared(dev, users, order, n):
    """Runs users[k] for k in `order` (round = position) on one zero-filled buffer of n floats; every output
    bitwise equal to the same call with a private, freshly zeroed scratch; the counters zero afterwards."""
    shared = torch.zeros(n, dtype=torch.float32, device=dev)
    bad = []
    for rnd, k in enumerate(order):
        u = users[k]
        assert u.n <= n
        got = [x.clone() for x in u.run(shared, rnd)]
        want = u.run(torch.zeros(u.n, dtype=torch.float32, device=dev), rnd)
        torch.cuda.synchronize()
        for j, (g, w) in enumerate(zip(got, want)):
            assert bool(torch.isfinite(w).all()), ("private-scratch reference not finite", rnd, k, j)
            if not _bits_equal(g, w):
                bad.append((rnd, k, j, g.flatten()[:4].tolist(), w.flatten()[:4].tolist()))
    assert not bad, f"(round, user, output, shared-scratch value, private-scratch value): {bad}"
    words = shared[:COUNTER_WORDS].view(torch.int32)
    assert int(words.abs().max()) == 0, words.nonzero().flatten().tolist()


PAIRS = ["pose200_l1", "pose5000_l1", "epilogue_l1", "posefused_l1", "maploss_pose", "maploss_l1",
         "maploss_posefused"]


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("name", PAIRS)
def test_shared_scratch_pair(cuda, name, first):
    """Two users whose size queries coincide (glue._scratch gives them one buffer) alternate A, B, A, B, A on it."""
    a, b = _pair(cuda, name)
    assert a.n == b.n, (name, a.n, b.n)
    if name.startswith("maploss"):
        m = _map640(cuda)
        if _map_rows(cuda, m.H, m.W) != 32:
            pytest.skip(f"{torch.cuda.get_device_properties(cuda).multi_processor_count} CUs: 640x480 keeps the "
                        "16-row SSIM tile")
    _check_shared(cuda, (a, b), [first, 1 - first, first, 1 - first, first], a.n)


def test_shared_scratch_all_five(cuda):
    """What a C caller reading the header does: one zero-filled buffer of the largest query serves all five."""
    r = _render(cuda, 3000)
    users = (_Pose(cuda, 5000), _L1(cuda, 48, 50), _View(r.n_fwd, r.run_fwd), _View(r.n_bwd, r.run_bwd),
             _map640(cuda))
    n = max(u.n for u in users)
    _check_shared(cuda, users, [0, 1, 2, 3, 4], n)
    _check_shared(cuda, users, [4, 3, 2, 1, 0], n)
    _check_shared(cuda, users, [1, 4, 0, 4, 3], n)


# ----------------------------------------------------------- python path --
def _glue_iteration(p, w2c, ups, imgs, scale):
    """tracking_l1 and track_transform's backward (both ask glue._scratch for gsr_track_scratch_floats)."""
    from splatam_amd import glue
    im, ds, gt_im, gt_d = imgs
    loss = glue.tracking_l1(im * scale, ds, gt_im, gt_d, SIL_THRES, W_IM, W_DEPTH)
    means, rot, dcol, _, _ = glue.track_transform(p, 1, w2c)
    total = (means * ups[0]).sum() * scale + (rot * ups[1]).sum() * scale + (dcol * ups[2]).sum() * scale
    total.backward()
    return loss


def test_glue_python_path_shares_scratch(cuda):
    """glue.tracking_l1 + glue.track_transform backward at P = 200 and 12x16 (equal scratch queries, so
    glue._scratch gives both the same buffer): three eager iterations with changing inputs, then a HIP graph
    of one iteration replayed twice; every loss against float64 (1e-5 relative), every pose gradient against
    float64 autograd (rtol 1e-4 / atol 1e-6)."""
    P, H, W = 200, 12, 16
    assert lib.gsr_track_scratch_floats(P) == lib.gsr_track_scratch_floats(H * W)
    p_cpu, w2c_cpu, ups_cpu = _pose_inputs(P, 3)
    imgs_cpu = _l1_images(H, W)
    imgs = [x.to(cuda) for x in imgs_cpu]
    ups, w2c = [u.to(cuda) for u in ups_cpu], w2c_cpu.to(cuda)

    def leaves():
        p = {k: v.to(cuda) for k, v in p_cpu.items()}
        p["cam_unnorm_rots"].requires_grad_(True)
        p["cam_trans"].requires_grad_(True)
        return p

    def check(loss, p, scale):
        ref = _l1_reference(imgs_cpu[0] * scale, *imgs_cpu[1:])[0]
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (scale, float(loss), ref)
        rq, rt = _pose_reference(p_cpu, w2c_cpu, [u * scale for u in ups_cpu])
        torch.testing.assert_close(p["cam_unnorm_rots"].grad[0, :, 1].cpu().double(), rq, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(p["cam_trans"].grad[0, :, 1].cpu().double(), rt, rtol=1e-4, atol=1e-6)

    for scale in ROUND_SCALE[:3]:
        p = leaves()
        check(_glue_iteration(p, w2c, ups, imgs, scale), p, scale)

    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    p = leaves()
    scale_t = torch.ones((), device=cuda)
    with torch.cuda.stream(side):
        _glue_iteration(p, w2c, ups, imgs, scale_t)  # warm-up on the capture stream (allocates its scratch)
        p["cam_unnorm_rots"].grad = None
        p["cam_trans"].grad = None
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss = _glue_iteration(p, w2c, ups, imgs, scale_t)
    for scale in ROUND_SCALE[3:5]:
        scale_t.fill_(scale)
        loss.detach().fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        check(loss.detach(), p, scale)


# ------------------------------------------------------------ grid edges --
L1_SHAPES = [(1, 1), (15, 17), (16, 16), (1, 257), (48, 80), (64, 64), (17, 241), (15, 563), (513, 512)]


@pytest.mark.parametrize("hw", L1_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_track_l1_grid_edges(cuda, hw):
    """H*W = 1, 255, 256, 257 (one / two workgroups), 15*256, 16*256, 16*256+1 (15 / 16 / 17 workgroups: the
    arrival groups' boundary), 33*256-3 (uneven groups, a ragged last workgroup) and 513x512 (past the 1024
    workgroup cap: the grid-stride loop runs twice for some lanes only).  Loss within 1e-5 relative of
    float64; the gradient images are signs times the seed, so they are exact; fwd, fwd_bwd and bwd agree
    bitwise."""
    H, W = hw
    cpu = _l1_images(H, W, seed=H * 1000 + W)
    if H * W == 1:  # the only pixel must be inside the mask
        cpu[1][1], cpu[3][0] = 1.0, cpu[1][0] + 0.25
    im, ds, gt_im, gt_d = [x.to(cuda) for x in cpu]
    scratch = torch.zeros(lib.gsr_track_scratch_floats(H * W), dtype=torch.float32, device=cuda)
    seed = torch.full((), 2.0, device=cuda)
    ref, ref_dim, ref_dds, mask = _l1_reference(*cpu, seed=2.0)
    assert int(mask.sum()) > 0 and ref > 0.0
    for _ in range(2):  # the second call runs on the scratch the first one left
        loss, dim, dds = _call_l1_fwd_bwd(cuda, im, ds, gt_im, gt_d, scratch, seed)
        loss2 = _call_l1_fwd(cuda, im, ds, gt_im, gt_d, scratch)
        dim2, dds2 = _call_l1_bwd(cuda, im, ds, gt_im, gt_d, seed)
        torch.cuda.synchronize()
        print(f"track_l1 {H}x{W}: kernel {float(loss):.9g} float64 {ref:.9g} rel {abs(float(loss) - ref) / ref:.2e}")
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
        assert _bits_equal(loss, loss2)
        assert torch.equal(dim.cpu(), ref_dim) and torch.equal(dds.cpu(), ref_dds)
        assert _bits_equal(dim, dim2) and _bits_equal(dds, dds2)
    assert int(scratch[:COUNTER_WORDS].view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("scols", [1, 3])
@pytest.mark.parametrize("P", [1, 257, 4097, 65536, 65537])
def test_track_transform_bwd_grid_edges(cuda, P, scols):
    """P = 1, 257, 4097 (1, 2, 17 workgroups), 65536 (exactly the 256-workgroup cap) and 65537 (past it: one
    lane runs the grid-stride loop twice), isotropic and anisotropic, on a strided pose column (q_stride = 2,
    t = 1) with a non-identity w2c, against float64 autograd through slam.transform_to_frame and the rendervar
    builders: rtol 1e-4 / atol 1e-6 (tests/test_gpu_slam.py)."""
    u = _Pose(cuda, P, scols)
    scratch = torch.zeros(u.n, dtype=torch.float32, device=cuda)
    rq, rt = _pose_reference(*u.cpu)
    for _ in range(2):
        dq, dt = u.grad(scratch)
        dq, dt = dq.cpu().double(), dt.cpu().double()
        print(f"pose P={P} S={scols}: max rel dq {float(((dq - rq).abs() / rq.abs()).max()):.2e} "
              f"dt {float(((dt - rt).abs() / rt.abs()).max()):.2e}")
        torch.testing.assert_close(dq, rq, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(dt, rt, rtol=1e-4, atol=1e-6)
    assert float(rq.abs().min()) > 0.0 and float(rt.abs().min()) > 0.0
    assert int(scratch[:COUNTER_WORDS].view(torch.int32).abs().max()) == 0


def _map_shape(dev, kind):
    """(H, W, tile rows expected)."""
    if kind == "ragged32":
        # one tile column, 16 * CUs + 5 rows: ceil(H / 16) = CUs + 1 workgroup rows (3 (CUs + 1) > 3 CUs) but
        # 3 * (CUs / 2 + 1) <= 2 CUs with 32 rows; 61 x 4101 on 256 CUs (771 > 768, 387 <= 512); H % 32 = 5
        # and W % 64 = 61 leave ragged bottom and right edges
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        return 16 * cus + 5, 61, 32
    return {"17x65": (17, 65, 16), "33x129": (33, 129, 16), "ragged16": (45, 100, 16)}[kind]


@pytest.mark.parametrize("kind", ["17x65", "33x129", "ragged16", "ragged32"])
def test_map_loss_grid_edges(cuda, kind):
    """gsr_map_loss_fwd / _bwd against the literal loss in float64 at shapes one past a tile in both
    directions, and at ragged tiles of both SSIM tile heights; tolerances of
    test_mapping_loss_kernel_matches_literal (loss 1e-5 relative, dL/dim 1e-5 and dL/ddepth_sil 1e-6
    relative L2)."""
    H, W, rows = _map_shape(cuda, kind)
    if _map_rows(cuda, H, W) != rows:
        pytest.skip(f"{torch.cuda.get_device_properties(cuda).multi_processor_count} CUs: {H}x{W} does not take "
                    f"the {rows}-row SSIM tile")
    assert H % rows != 0 and W % 64 != 0
    u = _MapLoss(cuda, H, W)
    scratch = torch.zeros(u.n, dtype=torch.float32, device=cuda)
    r_im, r_ds = u.im.cpu().double().requires_grad_(True), u.ds.cpu().double().requires_grad_(True)
    ref = _map_literal(r_im, r_ds, u.gt.cpu().double(), u.gd.cpu().double())
    ref.backward()
    ref = ref.detach()
    g_ds = torch.nan_to_num(r_ds.grad, nan=0.0)
    for _ in range(2):
        loss, dim, dds = u.call(scratch, u.im)
        torch.cuda.synchronize()
        print(f"map_loss {H}x{W}: kernel {float(loss):.9g} float64 {float(ref):.9g} "
              f"dim {_rel(dim.cpu(), r_im.grad):.2e} dds {_rel(dds.cpu(), g_ds):.2e}")
        assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
        assert _rel(dim.cpu(), r_im.grad) <= 1e-5
        assert _rel(dds.cpu(), g_ds) <= 1e-6
        assert float(dds[1:].abs().sum()) == 0.0
    assert int(scratch[:COUNTER_WORDS].view(torch.int32).abs().max()) == 0


# ------------------------------------------------------------- mask edges --
def _edge_images():
    """16x16 images with, in row 0: (0) gt_depth == 0, (1) NaN depth, (2) finite depth with NaN depth_sq,
    (3) silhouette exactly sil_thres (strict >: excluded), (4) residual exactly 0 in every channel."""
    im, ds, gt_im, gt_d = _l1_images(16, 16, seed=21)
    ds[1] = 1.0
    gt_d[0] = ds[0] + 0.25
    gt_d[0, 0, 0] = 0.0
    ds[0, 0, 1] = NAN
    ds[2, 0, 2] = NAN
    ds[1, 0, 3] = torch.tensor(SIL_THRES, dtype=torch.float32)
    im[:, 0, 4] = gt_im[:, 0, 4]
    gt_d[0, 0, 4] = ds[0, 0, 4]
    return im, ds, gt_im, gt_d


def test_track_l1_mask_and_sign_edges(cuda):
    cpu = _edge_images()
    im, ds, gt_im, gt_d = [x.to(cuda) for x in cpu]
    scratch = torch.zeros(lib.gsr_track_scratch_floats(256), dtype=torch.float32, device=cuda)
    seed = torch.ones((), device=cuda)
    ref, ref_dim, ref_dds, mask = _l1_reference(*cpu)
    assert not bool(mask[0, :4].any()) and bool(mask[0, 4]) and int(mask.sum()) == 256 - 4
    loss, dim, dds = _call_l1_fwd_bwd(cuda, im, ds, gt_im, gt_d, scratch, seed)
    loss2 = _call_l1_fwd(cuda, im, ds, gt_im, gt_d, scratch)
    dim2, dds2 = _call_l1_bwd(cuda, im, ds, gt_im, gt_d, seed)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
    assert _bits_equal(loss, loss2) and _bits_equal(dim, dim2) and _bits_equal(dds, dds2)
    assert torch.equal(dim.cpu(), ref_dim) and torch.equal(dds.cpu(), ref_dds)
    for x in range(5):  # the four excluded pixels and the zero-residual one: exactly zero
        assert float(dim[:, 0, x].abs().sum()) == 0.0 and float(dds[:, 0, x].abs().sum()) == 0.0, x
    assert float(dim[:, 1:].abs().min()) == W_IM and float(dds[0, 1:].abs().min()) == W_DEPTH
    # one fully masked image
    gt_0 = torch.zeros_like(gt_d)
    loss, dim, dds = _call_l1_fwd_bwd(cuda, im, ds, gt_im, gt_0, scratch, seed)
    loss2 = _call_l1_fwd(cuda, im, ds, gt_im, gt_0, scratch)
    dim2, dds2 = _call_l1_bwd(cuda, im, ds, gt_im, gt_0, seed)
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and float(loss2) == 0.0
    for g in (dim, dds, dim2, dds2):
        assert float(g.abs().sum()) == 0.0  # (a NaN left from the sentinel would fail this too)


def test_render_epilogue_l1_mask_edges(cuda):
    """gsr_track_forward_dual_static with gt_depth == 0 pixels and one pixel whose rendered silhouette equals
    sil_thres exactly, against gsr_track_l1_fwd_bwd on the images that call rendered: gradient images bitwise
    equal, loss equal up to the summation order (1e-6 relative, as
    test_render_epilogue_l1_matches_separate_kernel), excluded pixels exactly zero."""
    r = _render(cuda, 3000)
    H, W = r.H, r.W
    probe = r.forward(torch.zeros(r.n_fwd, dtype=torch.float32, device=cuda))
    sil = probe["ds"][1]
    # a covered pixel whose silhouette is not the image's most common value: the threshold sits on it
    cand = ((sil > 0.3) & (sil < 0.999)).nonzero()
    assert cand.shape[0] > 0
    y, x = [int(v) for v in cand[cand.shape[0] // 2]]
    thres = float(sil[y, x])
    gt_d = r.gt_d.clone()
    gt_d[0, :, : W // 5] = 0.0
    scratch = torch.zeros(r.n_fwd, dtype=torch.float32, device=cuda)
    for _ in range(2):
        o = r.forward(scratch, gt_d=gt_d, thres=thres)
        assert _bits_equal(o["ds"], probe["ds"]) and float(o["ds"][1, y, x]) == thres
        s2 = torch.zeros(lib.gsr_track_scratch_floats(H * W), dtype=torch.float32, device=cuda)
        loss, dim, dds = _call_l1_fwd_bwd(cuda, o["im"], o["ds"], r.gt_im, gt_d, s2, r.seed, thres=thres)
        torch.cuda.synchronize()
        included = (o["ds"][1] > thres) & (gt_d[0] > 0)
        assert int(included.sum()) > 100 and not bool(included[y, x])
        assert float(loss) > 0.0 and abs(float(o["loss"]) - float(loss)) <= 1e-6 * abs(float(loss))
        assert _bits_equal(o["dim"], dim) and _bits_equal(o["dds"], dds)
        assert float(o["dim"][:, ~included].abs().sum()) == 0.0 and float(o["dds"][:, ~included].abs().sum()) == 0.0
        assert float(o["dim"][:, y, x].abs().sum()) == 0.0
    assert int(scratch[:COUNTER_WORDS].view(torch.int32).abs().max()) == 0
