"""Fisher-information view scoring on the backward_power=2 path.

The fork's active-mapping node scores candidate camera poses by the expected
information gain of a view (scripts/ros_handler.py:807-902):

  * compute_Hessian(w2c) (:847-902): the Gaussians moved into the candidate
    camera frame (means only; rotations / opacities / scales / colours as
    rendervars), one RGB render with GaussianRasterizer(backward_power=2), and a
    backward seeded with 1e-3 everywhere; H = [dL/dmeans_cam (P,3), dL/dopacity
    (P,1)] -- per-pair gradients squared before summation, i.e. the diagonal of
    the Gauss-Newton / Fisher matrix;
  * compute_H_visited_inv (:807-829): H_train = sum of H over the visited poses,
    H_train_inv = 1 / (H_train + 0.1);
  * compute_eig_score (:832-836): sum(H(candidate) * H_train_inv).

FisherScorer restates these over a *batch* of poses and shards the batch over
ranks (one process per GPU): H_train is the all-reduce (sum) of the per-rank
partial sums (RCCL over xGMI, 16 B per Gaussian), candidate scores are formed on
the device and exchanged once with an all-gather.  Each pose's render +
power-2 backward runs through the HIP rasterizer (gsr_forward / gsr_backward
with power = 2) and only the two gradients H needs are requested, which selects
the Fisher kernels (gauss_mpack, render_bwd_fisher, gauss_bwd_fisher: 4 powered
values per pixel-Gaussian pair instead of the full path's 22).

BatchedFisher renders a batch of K poses per host launch: the K transforms, static-
capacity forwards (gsr_forward_static), power-2 backwards and the per-pose reductions
(H accumulation for the visited poses, or the EIG score of each candidate) are captured
once into a HIP graph and replayed with the poses written into a device [K,4,4] tensor.
Every pose's Hessian is bitwise the per-pose FisherScorer.hessian's.

The node publishes a mixed gain per candidate (send_gains, :251-359): the EIG next to a silhouette
gain, the share of pixels whose rendered silhouette is below 0.5, which the reference takes from a
second render per pose (get_renders, :955-985) and reads back.  silhouette_count() and
BatchedFisher(mode="gains") take it from the buffers the scoring forward leaves anyway
(gsr_silhouette_count, csrc/gsr_viewgain.hip), so each pose is binned once and nothing is read back.

The node scores after every frame of the realtime loop, on the map as it then stands
(scripts/splatam_realtime.py:1011).  SequenceFisher is BatchedFisher on a running SlamSequence's
capacity-padded map: captured once, it reads the sequence's own tensors under the alive mask on every
replay (gsr_forward_static_alive; gsr_fisher_score for the EIG, a float64 sum over the live rows in one
launch), so a frame's densification, pruning and compaction need no rebuild
(SlamSequence.view_scorer / fit_visited / view_gains).
"""
from __future__ import annotations

import ctypes

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import dist as sd
from ._devcall import check_rc
from .rasterizer import GaussianRasterizer

SEED = 1e-3      # im.backward(gradient=torch.ones_like(im) * 1e-3)  (ros_handler.py:888)
# the gradients H reads (ros_handler.py:884-889): dmeans3D and dopacity -- the Fisher-selective
# backward_power kernel (gsr_backward_power.hip render_bwd_fisher_kernel), 4 values per pair
FISHER_NEEDS = (False, False, True, True, False, False, False, False)
H_EPS = 0.1      # torch.reciprocal(H_train + 0.1)                   (ros_handler.py:829)


def camera_points(means: torch.Tensor, w2c: torch.Tensor) -> torch.Tensor:
    """(rel_w2c @ pts4.T).T[:, :3] (ros_handler.py:863-866) in one launch (gsr_points_to_camera: each
    coordinate summed left to right; a [P,3] x [3,3] addmm took a 22 us hipBLASLt kernel); shared by the
    per-pose and the batched paths, so both see bitwise the same camera-frame points."""
    from ._lib import lib
    if means.device.type != "cuda":
        raise RuntimeError("Fisher scoring runs on ROCm devices only (no CPU fallback)")
    means = means.detach().float().contiguous()
    w2c = w2c.detach().to(means.device).float().contiguous()
    pts = torch.empty_like(means)
    check_rc(lib.gsr_points_to_camera(means.shape[0], means.data_ptr(), w2c.data_ptr(), pts.data_ptr(),
                                      torch.cuda.current_stream(means.device).cuda_stream), "gsr_points_to_camera")
    return pts


def _count_into(cam, P: int, n: int, geom, binning, img, sil_thres: float, out: torch.Tensor):
    """gsr_silhouette_count on a finished forward's buffers into out (device int32 [1]; the C side writes an
    unsigned, W H < 2^31 here)."""
    from . import _C
    from ._lib import lib
    dev = out.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    st, keep = _C._settings(cam.bg, cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy,
                            cam.image_height, cam.image_width, cam.scale_modifier, cam.sh_degree, cam.prefiltered,
                            dev, stream)
    ptr = lambda t: t.data_ptr() if (t is not None and t.numel()) else None  # noqa: E731
    rc = lib.gsr_silhouette_count(ctypes.byref(st), int(P), int(n), ptr(geom), ptr(binning), ptr(img),
                                  float(sil_thres), out.data_ptr(), stream)
    del keep
    check_rc(rc, "gsr_silhouette_count")


def silhouette_count(scorer: "FisherScorer", w2c: torch.Tensor, sil_thres: float = 0.5) -> torch.Tensor:
    """(sil < sil_thres).sum() of send_gains (ros_handler.py:296-299) for one camera (w2c [4,4]): the number of
    pixels whose silhouette -- channel 1 of the [z, 1, z^2] render of the map moved into the candidate frame --
    is below the threshold, as a device int32 scalar (no read-back).  camera_points, the ordinary forward,
    then gsr_silhouette_count on that forward's buffers: no second render.

    The map is moved as compute_Hessian moves it (means only).  The reference's silhouette render
    (transform_gaussians, :905-952) also rotates the quaternions; for SplaTAM's isotropic map the two see the
    same geometry, for an anisotropic one they do not (BatchedFisher mode "gains" refuses such a map)."""
    from . import _C
    if scorer._hessian_fn is not None:
        raise RuntimeError("silhouette_count renders through the rasterizer (no hessian_fn override)")
    cam = scorer.cam
    means = scorer.params["means3D"].detach()
    with torch.no_grad():
        pts = camera_points(means, w2c)
        out = torch.empty(1, dtype=torch.int32, device=means.device)
        e = torch.Tensor([])
        P = pts.shape[0]
        if P == 0:  # the forward of an empty map runs nothing and leaves no buffers
            _count_into(cam, 0, 0, None, None, None, sil_thres, out)
            return out[0]
        n, _, _, geom, binning, img, _ = _C.rasterize_gaussians(
            cam.bg, pts, scorer.colors.detach(), scorer.opacities.detach(), scorer.scales.detach(),
            scorer.rotations.detach(), cam.scale_modifier, e, cam.viewmatrix, cam.projmatrix, cam.tanfovx,
            cam.tanfovy, cam.image_height, cam.image_width, e, cam.sh_degree, cam.campos, cam.prefiltered)
        _count_into(cam, P, n, geom, binning, img, sil_thres, out)
    return out[0]


def _nl(g: torch.Tensor) -> torch.Tensor:
    return 3400.0 / (1.0 + torch.exp(-0.002 * g)) - 1700.0  # ros_handler.py:316,318


def combine_gains(counts: torch.Tensor, eig: torch.Tensor, n_pixels: int, k_sil: float = 1.0, k_eig: float = 1.0,
                  k_sum: float = 1.0, nl_sil: bool = False, nl_eig: bool = False) -> torch.Tensor:
    """send_gains' mixed gain (ros_handler.py:299-322) for n poses, in float64 on the inputs' device:
    counts [n] pixels below the silhouette threshold, eig [n] compute_eig_score.  Returns [n,3]
    (g_sil, g_eig, gain): g_sil = count / (W H) * k_sil, g_eig = eig * k_eig (0 when k_eig == 0, which
    skips the score there), each optionally through 3400 / (1 + exp(-0.002 g)) - 1700,
    gain = k_sum * (g_eig + g_sil)."""
    # (a tensor divisor: torch divides a device tensor by a Python scalar as a product with its reciprocal,
    # one rounding more than the reference's float division)
    g_sil = counts.double() / torch.full_like(counts, float(n_pixels), dtype=torch.float64)
    g_eig = eig.double() if k_eig != 0 else torch.zeros_like(eig, dtype=torch.float64)
    g_sil = g_sil * float(k_sil)
    g_eig = g_eig * float(k_eig)
    if nl_sil:
        g_sil = _nl(g_sil)
    if nl_eig:
        g_eig = _nl(g_eig)
    return torch.stack([g_sil, g_eig, float(k_sum) * (g_eig + g_sil)], dim=1)


class FisherScorer:
    def __init__(self, params: dict, cam, hessian_fn=None):
        """params: SplaTAM parameter dict (means3D, rgb_colors, unnorm_rotations, logit_opacities,
        log_scales); cam: GaussianRasterizationSettings of the scoring camera.  hessian_fn(w2c) -> H
        overrides the per-pose Hessian (tests of the sharding on CPU)."""
        self.params, self.cam = params, cam
        self._hessian_fn = hessian_fn
        self.H_train_inv = None
        if hessian_fn is None:
            with torch.no_grad():  # ros_handler.py:868-874
                self.rotations = F.normalize(params["unnorm_rotations"])
                self.opacities = torch.sigmoid(params["logit_opacities"])
                scales = torch.exp(params["log_scales"])
                self.scales = torch.tile(scales, (1, 3)) if scales.shape[-1] == 1 else scales
                self.colors = params["rgb_colors"]

    def hessian(self, w2c: torch.Tensor) -> torch.Tensor:
        """compute_Hessian(rel_w2c, return_points=True): H [P,4] for one camera (w2c [4,4])."""
        if self._hessian_fn is not None:
            return self._hessian_fn(w2c)
        means = self.params["means3D"].detach()
        w2c = w2c.to(means.device).float()
        with torch.no_grad():
            pts = camera_points(means, w2c)
        pts.requires_grad_(True)
        opac = self.opacities.detach().clone().requires_grad_(True)
        means2D = torch.zeros_like(pts)
        im, _, _ = GaussianRasterizer(self.cam, backward_power=2)(
            means3D=pts, means2D=means2D, opacities=opac, colors_precomp=self.colors.detach(),
            scales=self.scales.detach(), rotations=self.rotations.detach())
        im.backward(gradient=torch.full_like(im, SEED))
        return torch.cat([pts.grad.reshape(pts.shape[0], -1), opac.grad.reshape(pts.shape[0], -1)], dim=1)

    def fit_visited(self, w2cs, batch: "BatchedFisher | None" = None) -> torch.Tensor:
        """compute_H_visited_inv over all visited poses: each rank sums the Hessians of its shard
        (poses r, r+W, ...), one all-reduce merges them.  Returns (and keeps) H_train_inv.
        batch: a BatchedFisher(mode="sum") -- the shard is rendered K poses per graph launch."""
        r, w = sd.world()
        H = None
        mine = [w2cs[j] for j in range(r, len(w2cs), w)]
        if batch is not None:
            for c in range(0, len(mine), batch.K):
                chunk = mine[c:c + batch.K]
                h = batch.hessian_sum(chunk)
                if h is None:  # a pose exceeded the graph's binning capacity: the eager path re-sizes
                    h = sum(self.hessian(w2c) for w2c in chunk)
                H = h.clone() if H is None else H + h
        for w2c in ([] if batch is not None else mine):
            h = self.hessian(w2c)
            H = h if H is None else H + h
        if H is None:  # this rank has no pose: contribute zeros of the right shape
            P = self.params["means3D"].shape[0]
            H = torch.zeros(P, 4, device=self.params["means3D"].device)
        sd.all_reduce_sum_(H)
        self.H_train_inv = torch.reciprocal(H + H_EPS)
        return self.H_train_inv

    def eig_scores(self, w2cs, batch: "BatchedFisher | None" = None) -> torch.Tensor:
        """compute_eig_score for every candidate pose: sum(H(pose) * H_train_inv).  The batch is
        sharded over ranks; returns all scores (float64, in pose order) on every rank.
        batch: a BatchedFisher(mode="scores") -- K candidate poses per graph launch."""
        if self.H_train_inv is None:
            raise RuntimeError("fit_visited() first (H_train_inv)")
        r, w = sd.world()
        n = len(w2cs)
        per = -(-n // w) if n else 0
        dev = self.H_train_inv.device
        local = torch.zeros(max(per, 1), dtype=torch.float64, device=dev)
        mine = list(range(r, n, w))
        if batch is not None:
            for c in range(0, len(mine), batch.K):
                idx = mine[c:c + batch.K]
                sc = batch.scores([w2cs[j] for j in idx], self.H_train_inv)
                if sc is None:  # capacity overflow in the graph: score this chunk on the eager path
                    sc = torch.stack([(self.hessian(w2cs[j]) * self.H_train_inv).sum().double() for j in idx])
                local[c:c + len(idx)] = sc
        for k, j in enumerate([] if batch is not None else mine):
            local[k] = (self.hessian(w2cs[j]) * self.H_train_inv).sum().double()
        if w == 1:
            return local[:n]
        gathered = [torch.zeros_like(local) for _ in range(w)]
        dist.all_gather(gathered, local)
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        for rr in range(w):
            idx = list(range(rr, n, w))
            out[idx] = gathered[rr][:len(idx)]
        return out

    def view_gains(self, w2cs, batch: "BatchedFisher | None" = None, sil_thres: float = 0.5, **weights) -> torch.Tensor:
        """send_gains' (g_sil, g_eig, gain) for every candidate pose: float64 [n,3] in pose order on every rank,
        sharded and gathered like eig_scores.  weights: k_sil, k_eig, k_sum, nl_sil, nl_eig (combine_gains).
        batch: a BatchedFisher(mode="gains") -- K candidate poses per graph launch (its sil_thres holds);
        without one each pose is hessian() + silhouette_count()."""
        if self.H_train_inv is None:
            raise RuntimeError("fit_visited() first (H_train_inv)")
        r, w = sd.world()
        n = len(w2cs)
        per = -(-n // w) if n else 0
        dev = self.H_train_inv.device
        npix = self.cam.image_width * self.cam.image_height
        local = torch.zeros(max(per, 1), 3, dtype=torch.float64, device=dev)
        mine = list(range(r, n, w))

        def eager(idx):
            eig = torch.stack([(self.hessian(w2cs[j]) * self.H_train_inv).sum().double() for j in idx])
            cnt = torch.stack([silhouette_count(self, w2cs[j], sil_thres) for j in idx])
            return combine_gains(cnt, eig, npix, **weights)

        step = batch.K if batch is not None else 1
        for c in range(0, len(mine), step):
            idx = mine[c:c + step]
            g = batch.gains([w2cs[j] for j in idx], self.H_train_inv, **weights) if batch is not None else None
            if g is None:  # no batch, or a capacity overflow in the graph: this chunk on the eager path
                g = eager(idx)
            local[c:c + len(idx)] = g
        if w == 1:
            return local[:n]
        gathered = [torch.zeros_like(local) for _ in range(w)]
        dist.all_gather(gathered, local)
        out = torch.zeros(n, 3, dtype=torch.float64, device=dev)
        for rr in range(w):
            idx = list(range(rr, n, w))
            out[idx] = gathered[rr][:len(idx)]
        return out


class _PoseBatchGraph:
    """What BatchedFisher and SequenceFisher share: K pose slots rendered per HIP-graph launch.  The slots (`w2c`
    [K,4,4], `weight` [K], `H_inv` [P,4], `status` [K,4], `counts` [K] in mode "gains", the backward's `seed`),
    the warm-up and the capture, and the calls that load the slots, replay and read the status.  A subclass sets
    `cam`, `alive` (the forward's mask, or None) and `capacity` (the forward's binning capacity) and gives
    _rendervars, _scores_out, _score and _scores_result."""

    @staticmethod
    def _check_mode(mode: str, log_scales: torch.Tensor):
        if mode not in ("sum", "scores", "gains"):
            raise ValueError("mode is 'sum', 'scores' or 'gains'")
        if mode == "gains" and log_scales.shape[-1] != 1:
            raise ValueError("mode 'gains' takes an isotropic map only (log_scales [P,1]): the reference's "
                             "silhouette render rotates the Gaussians, its Hessian render does not")

    def _make_slots(self, cam, P: int, dev, K: int, mode: str, sil_thres: float):
        self.cam, self.K, self.mode, self.sil_thres = cam, int(K), mode, float(sil_thres)
        self.w2c = torch.eye(4, device=dev).repeat(self.K, 1, 1).contiguous()
        self.weight = torch.zeros(self.K, device=dev)
        self.H_inv = torch.zeros(P, 4, device=dev)
        self.status = torch.zeros(self.K, 4, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(self.K, dtype=torch.int32, device=dev) if mode == "gains" else None
        self.seed = torch.full((3, cam.image_height, cam.image_width), SEED, device=dev)  # ros_handler.py:888
        self.e = torch.Tensor([])

    def _capture(self):
        from . import _C
        dev = self.H_inv.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._body(_C)  # warm-up (allocator pools, kernels) outside the capture
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.status.zero_()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._body(_C)

    def _forward(self, _C, pts, rv, capacity, k):
        """The forward of camera-frame points `pts`; static (capacity > 0) into status row k."""
        cam = self.cam
        _, colors, opac, scales, rot = rv
        return _C.rasterize_gaussians(cam.bg, pts, colors, opac, scales, rot, cam.scale_modifier, self.e,
                                      cam.viewmatrix, cam.projmatrix, cam.tanfovx, cam.tanfovy, cam.image_height,
                                      cam.image_width, self.e, cam.sh_degree, cam.campos, cam.prefiltered,
                                      capacity=capacity, status=self.status[k] if capacity else None,
                                      alive=self.alive)

    def _grads(self, _C, k, rv):
        """(dL/dmeans_cam [P,3], dL/dopacity [P,1]) of pose slot k (power-2 backward, Fisher kernels)."""
        cam = self.cam
        _, colors, _, scales, rot = rv
        pts = camera_points(rv[0], self.w2c[k])
        n, _, radii, geom, binning, img, _ = self._forward(_C, pts, rv, self.capacity, k)
        if self.mode == "gains":  # the silhouette count on this forward's lists, ahead of the backward
            _count_into(cam, pts.shape[0], n, geom, binning, img, self.sil_thres, self.counts[k:k + 1])
        g = _C.rasterize_gaussians_backward(cam.bg, pts, radii, colors, scales, rot, cam.scale_modifier, self.e,
                                            cam.viewmatrix, cam.projmatrix, cam.tanfovx, cam.tanfovy, self.seed,
                                            self.e, cam.sh_degree, cam.campos, geom, n, binning, img, 2,
                                            needs=FISHER_NEEDS)
        return g[3], g[2]

    def _body(self, _C):
        from ._lib import lib
        with torch.no_grad():
            rv = self._rendervars()
            if self.mode == "sum":
                self.out = torch.zeros_like(self.H_inv)
                P = self.out.shape[0]
                stream = torch.cuda.current_stream(self.out.device).cuda_stream
                for k in range(self.K):
                    dm, dop = self._grads(_C, k, rv)
                    # out += [dm, dop] * weight[k] in one launch (bitwise torch's add_(cat(...) * w))
                    check_rc(lib.gsr_fisher_accumulate(P, dm.data_ptr(), dop.data_ptr(),
                                                       self.weight.data_ptr() + 4 * k, self.out.data_ptr(), stream),
                             "gsr_fisher_accumulate")
            else:
                self.out = self._scores_out()
                for k in range(self.K):
                    self._score(k, *self._grads(_C, k, rv))

    def _load(self, w2cs):
        if len(w2cs) > self.K:
            raise ValueError(f"at most {self.K} poses per launch")
        with torch.no_grad():
            self.weight.zero_()
            for k, w in enumerate(w2cs):
                self.w2c[k].copy_(w)
                self.weight[k] = 1.0

    def _replay(self, n: int, check: bool) -> bool:
        """One graph launch on the loaded slots; with `check` (one host sync) False when one of the first n
        slots exceeded the binning capacity."""
        if check:
            self.status.zero_()
        self.graph.replay()
        return not (check and self.overflowed(n))

    def hessian_sum(self, w2cs, check: bool = True) -> torch.Tensor | None:
        """sum over the (<= K) poses of H(w2c) [P,4] (one graph launch; on a padded map over the padded rows,
        the dead ones +0).  With `check` (one host sync) returns None when a pose of this launch exceeded the
        binning capacity (its Hessian would be missing from the sum): the caller re-renders the chunk eagerly
        or rebuilds with more headroom."""
        if self.mode != "sum":
            raise RuntimeError(f"built for mode='{self.mode}'")
        self._load(w2cs)
        return self.out if self._replay(len(w2cs), check) else None

    def scores(self, w2cs, H_inv, check: bool = True) -> torch.Tensor | None:
        """sum(H(w2c_k) * H_inv) for each of the (<= K) poses against H_inv [P,4] (on a padded map the padded
        rows; the dead ones are not read): float64 [n] (one graph launch); None on a capacity overflow of any
        of them (see hessian_sum)."""
        if self.mode != "scores":
            raise RuntimeError(f"built for mode='{self.mode}'")
        return self._replay_scores(w2cs, H_inv, check)

    def _replay_scores(self, w2cs, H_inv, check):
        self._load(w2cs)
        if H_inv is not self.H_inv:  # (a caller may fill self.H_inv in place and pass it)
            with torch.no_grad():
                self.H_inv.copy_(H_inv)
        return self._scores_result(len(w2cs)) if self._replay(len(w2cs), check) else None

    def gains(self, w2cs, H_inv, k_sil: float = 1.0, k_eig: float = 1.0, k_sum: float = 1.0, nl_sil: bool = False,
              nl_eig: bool = False, check: bool = True) -> torch.Tensor | None:
        """send_gains' (g_sil, g_eig, gain) for each of the (<= K) poses: float64 [n,3] on the device (one graph
        launch, then combine_gains); None on a capacity overflow of any of them (see hessian_sum).  The raw
        counts of the launch stay in `counts[:n]`."""
        if self.mode != "gains":
            raise RuntimeError(f"built for mode='{self.mode}'")
        eig = self._replay_scores(w2cs, H_inv, check)
        if eig is None:
            return None
        cam = self.cam
        return combine_gains(self.counts[:len(w2cs)], eig, cam.image_width * cam.image_height, k_sil, k_eig, k_sum,
                             nl_sil, nl_eig)

    def overflowed(self, n: int | None = None) -> bool:
        """True if a replay since the last status reset exceeded the capacity in one of the first `n`
        slots (default: all K; padded slots render the previous poses and are not results)."""
        st = self.status[: self.K if n is None else n].cpu()
        return bool((st[:, 0] > self.capacity).any() or (st[:, 2] > st[:, 3]).any() or (st[:, 1] != 0).any())


class BatchedFisher(_PoseBatchGraph):
    """K poses of FisherScorer's Hessian per HIP-graph launch.

    mode "sum": `hessian_sum(w2cs)` returns sum_k H(w2c_k) (compute_H_visited_inv's H_train before the
    all-reduce); mode "scores": `scores(w2cs, H_inv)` returns [sum(H(w2c_k) * H_inv) for k] (float64 like
    FisherScorer.eig_scores); mode "gains": `gains(w2cs, H_inv, ...)` returns send_gains' (g_sil, g_eig, gain)
    per pose -- per slot the transform, the static forward, gsr_silhouette_count on that forward's buffers, the
    power-2 backward and "scores"' reduction, so each pose is binned once; g_eig / k_eig is bitwise "scores"'
    result.  Gains mode takes SplaTAM's isotropic map only (log_scales [P,1]): the reference renders the
    silhouette with the quaternions rotated into the candidate frame (transform_gaussians, ros_handler.py:905-952)
    and the Hessian without (compute_Hessian), which is the same geometry only for isotropic Gaussians -- one
    forward then serves both; an anisotropic map raises ValueError.
    Fewer than K poses pad the batch with weight-0 slots.  The binning capacity
    comes from eager probes of `probe_w2cs` times `headroom`; `overflowed()` reports (sticky) whether a
    replay exceeded it (results then invalid: rebuild with more headroom)."""

    alive = None  # (the compact map of a FisherScorer: every row is live)

    def __init__(self, scorer: FisherScorer, K: int, mode: str = "sum", probe_w2cs=None, headroom: float = 1.5,
                 min_extra: int = 65536, sil_thres: float = 0.5):
        if scorer._hessian_fn is not None:
            raise RuntimeError("BatchedFisher renders through the rasterizer (no hessian_fn override)")
        self._check_mode(mode, scorer.params["log_scales"])
        from . import _C
        self.sc = scorer
        self.means = means = scorer.params["means3D"].detach().contiguous()
        dev = means.device
        self._make_slots(scorer.cam, means.shape[0], dev, K, mode, sil_thres)
        rv = self._rendervars()
        probes = list(probe_w2cs) if probe_w2cs is not None else [torch.eye(4, device=dev)]
        n = 0
        with torch.no_grad():
            for w in probes:
                pts = camera_points(means, w.to(dev).float())
                n = max(n, self._forward(_C, pts, rv, 0, 0)[0])
        self.capacity = max(1, int(headroom * n) + int(min_extra))
        self._capture()

    def _rendervars(self):
        """The scorer's precomputed rendervars (FisherScorer.__init__)."""
        sc = self.sc
        return self.means, sc.colors.detach(), sc.opacities.detach(), sc.scales.detach(), sc.rotations.detach()

    def _scores_out(self):
        return torch.zeros(self.K, dtype=torch.float32, device=self.H_inv.device)

    def _score(self, k, dm, dop):  # compute_eig_score in float32 torch ops
        self.out[k] = (torch.cat([dm, dop.reshape(-1, 1)], dim=1) * self.H_inv).sum()

    def _scores_result(self, n):
        return self.out[:n].double()


def fisher_score(dmeans: torch.Tensor, dopac: torch.Tensor, H_inv: torch.Tensor, alive, workspace: torch.Tensor,
                 out: torch.Tensor):
    """gsr_fisher_score: out (device float64, one element) = the float64 sum over the live rows of the float32
    products [dmeans, dopac] * H_inv -- compute_eig_score in one launch, nothing read back.  alive: uint8 [P] or
    None (every row); workspace: score_workspace()'s."""
    from ._lib import lib
    P = dmeans.shape[0]
    dev = out.device
    # (hand checks: _devcall.require words its message otherwise)
    for name, t, n in (("dmeans", dmeans, 3 * P), ("dopac", dopac, P), ("H_inv", H_inv, 4 * P)):
        if t.device != dev or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"fisher_score: {name} must be a contiguous float32 tensor of {n} values on {dev}")
    if alive is not None and (alive.device != dev or alive.dtype != torch.uint8 or alive.numel() != P or
                              not alive.is_contiguous()):
        raise RuntimeError("fisher_score: alive must be a contiguous uint8 tensor of P entries")
    if out.dtype != torch.float64 or out.numel() != 1:
        raise RuntimeError("fisher_score: out is one float64")
    if workspace.device != dev or workspace.numel() * workspace.element_size() < lib.gsr_fisher_score_workspace_bytes():
        raise RuntimeError("fisher_score: workspace too small (score_workspace)")
    ptr = lambda t: t.data_ptr() if (t is not None and t.numel()) else None  # noqa: E731
    check_rc(lib.gsr_fisher_score(int(P), ptr(dmeans), ptr(dopac), ptr(H_inv), ptr(alive), workspace.data_ptr(),
                                  out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gsr_fisher_score")


def score_workspace(device) -> torch.Tensor:
    """gsr_fisher_score's workspace: zero-filled once; serves any number of calls on one stream."""
    from ._lib import lib
    return torch.zeros(int(lib.gsr_fisher_score_workspace_bytes()), dtype=torch.uint8, device=device)


class SequenceFisher(_PoseBatchGraph):
    """BatchedFisher on a running sequence's capacity-padded map (splatam_amd.sequence), captured once for the
    life of the buffers: K poses per HIP-graph launch, read from the map in place.

    params: the sequence's own tensors (`capacity + 1` rows each; means3D, rgb_colors, unnorm_rotations,
    logit_opacities, log_scales), alive: its uint8 mask, cam: the scoring camera, bin_capacity: the binning
    capacity of every pose's forward (given, not probed: the sequence sizes it once for all its renders).
    Every replay forms the rendervars from the tensors as they then stand (the torch ops of
    FisherScorer.__init__: elementwise per row, so a live row gets the bits it has on the compact map), then
    per pose slot camera_points, the static forward under the alive mask (gsr_forward_static_alive), in mode
    "gains" gsr_silhouette_count, the power-2 backward (FISHER_NEEDS) and gsr_fisher_accumulate (mode "sum")
    or gsr_fisher_score (modes "scores" / "gains"; float64 straight from the kernel, dead rows selected out).
    So densification, pruning and compact_static between replays need no rebuild; only a map moved to other
    buffers (SlamSequence.ensure_headroom) does.  The live rows' Hessians are bitwise BatchedFisher's on the
    compacted map and the dead rows' are +0 (tests/test_gpu_seqscore.py).  Mode "gains" takes the isotropic
    map only, as BatchedFisher does; overflowed() and the None of a checked call are BatchedFisher's too."""

    def __init__(self, params: dict, alive: torch.Tensor, cam, K: int, mode: str = "sum", bin_capacity: int = 0,
                 sil_thres: float = 0.5):
        self._check_mode(mode, params["log_scales"])
        if int(K) < 1 or int(bin_capacity) <= 0:
            raise ValueError("SequenceFisher: K >= 1 and bin_capacity > 0 (the static forward's binning capacity)")
        means = params["means3D"]
        dev, P = means.device, means.shape[0]
        if dev.type != "cuda":
            raise RuntimeError("Fisher scoring runs on ROCm devices only (no CPU fallback)")
        if alive.dtype != torch.uint8 or alive.numel() != P or alive.device != dev or not alive.is_contiguous():
            raise RuntimeError("alive: contiguous uint8 [P] on the parameters' device")
        self.params, self.alive, self.capacity = params, alive, int(bin_capacity)
        self._make_slots(cam, P, dev, K, mode, sil_thres)
        if mode != "sum":
            self.out = torch.zeros(self.K, dtype=torch.float64, device=dev)
            self.workspace = score_workspace(dev)
        self._capture()

    def _rendervars(self):
        """The map's rendervars as FisherScorer.__init__ forms them (ros_handler.py:868-874), once per replay."""
        p = self.params
        rot = F.normalize(p["unnorm_rotations"].detach())
        opac = torch.sigmoid(p["logit_opacities"].detach())
        scales = torch.exp(p["log_scales"].detach())
        scales = torch.tile(scales, (1, 3)) if scales.shape[-1] == 1 else scales
        return p["means3D"].detach(), p["rgb_colors"].detach(), opac, scales, rot

    def _scores_out(self):
        return self.out  # (preallocated: gsr_fisher_score writes its elements)

    def _score(self, k, dm, dop):
        fisher_score(dm, dop, self.H_inv, self.alive, self.workspace, self.out[k:k + 1])

    def _scores_result(self, n):
        return self.out[:n].clone()
