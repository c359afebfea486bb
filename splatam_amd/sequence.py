"""SplaTAM's per-frame loop on one capture: a SLAM sequence whose frames reuse one HIP-graph tracker and one
HIP-graph mapper.

scripts/splatam.py:697-929 runs, per frame t: the constant-velocity pose initialisation (initialize_camera_pose,
:429-448), `num_iters` tracking iterations with the best candidate written back (:700-763), add_new_gaussians
(:384-426: Gaussians from the pixels the map does not explain, appended to every parameter tensor), the mapping
iterations over a keyframe window (:796-905, prune_gaussians inside), and the keyframe bookkeeping.  P changes
every frame, and a captured graph needs fixed shapes, so the per-frame GraphTracker / GraphMapper of
splatam_amd.tracker / splatam_amd.mapper would be rebuilt every frame (probe, warm-up, capture: tens of ms).

Here the map lives in a capacity-padded buffer (splatam_amd.padded_map: pad_map, densify_static,
compact_static), so the padded map's live rows are always the reference map's rows in its order; the sequence
raises (check()) when the capacity is exhausted.  The tracker renders from a one-column pose slot and slot
targets that each frame fills; the mapper draws from a keyframe window set per frame (GraphMapper.set_keyframes).

The parts, one module each:
* splatam_amd.padded_map: the capacity-padded map and its row operations;
* splatam_amd.frame_ops: the frame steps restated on a parameter dict (pose initialisation, add_new_gaussians);
* splatam_amd.capture: the options, the frame store (tracking / densification resolutions, track_size /
  densify_size), the intake of a frame that arrives (float or raw) and the keyframe rule -- _SequenceBase;
* splatam_amd.seqscore: view scoring on the padded map (view_scorer, fit_visited, view_gains);
* splatam_amd.perframe: PerFrameSlam, the comparison loop that rebuilds its graphs every frame;
* this module: SlamSequence.  Their names stay importable from here (__all__).

Two keyframe policies (`keyframe_policy`):
* "window" (the default): the last `window - 1` keyframes plus the current frame; frame 0 and every
  keyframe_every-th frame are keyframes.  The draws are window indices from the sequence's numpy stream.
* "overlap": SplaTAM's own selection (keyframe_selection_overlap, :820-837; splatam_amd.keyframes states it and
  its two deliberate differences from the reference).  It runs on the device (select_device, three launches,
  after densification and before mapping) from a KeyframeBank that is appended at frame 0, at every
  keyframe_every-th frame and at frame num_frames - 2 (:932) with the pose as estimated then; the mapper
  gathers its per-iteration keyframes from the device-resident draws (GraphMapper.run(device_sequence=...)),
  so frame() still reads nothing back (but see track_cfg.use_depth_loss_thres below).  Randomness comes as
  32-bit words from the sequence's numpy stream (`draws` records them); PerFrameSlam runs
  keyframes.select_literal on the same words.

track_cfg.use_depth_loss_thres (the reference's iPhone and ScanNet++ configurations; scripts/splatam.py:745-758):
a frame whose last tracking iteration's depth loss is not below track_cfg.depth_loss_thres tracks for
tracking_iters more iterations, once.  The depth loss is a sum over the TRACKING frame's pixels (as in the reference,
whose loss is formed on tracking_curr_data), so with a tracking resolution the threshold is resolution-dependent:
a quarter of the pixels give about a quarter of the sum.  Both loops then build their trackers with loss_terms=True and pass the
threshold to GraphTracker.track_frame, which reads that one float per tracked frame -- the only host read of
frame(), and only with the option on (the reference reads the loss in every iteration).  tracking_iters_run
lists, per frame() call, the tracking iterations run (0 for frame 0, which is not tracked): an entry of
2 * tracking_iters is one of the reference's "Extra Tracking Iters Frames".

The realtime loop (scripts/splatam_realtime.py) is the same sequence fed frame by frame: `num_frames` fixes the
pose columns while the frame list grows, SlamSequence.push(im, depth, w2c=None) appends a frame and runs it,
a frame with `w2c` (its pose relative to frame 0, tracking.use_gt_poses, :812-821) is not tracked
(write_given_pose), `map_every` (:844) maps every that-many-th frame, `median_thr` / `median_scale` are
add_new_gaussians' threshold there (:444-453; densify.depth_threshold, gsr_densify_frame_capped) and
SlamSequence(params=None) builds the map from the first frame on the device (init_map_device: gsr_init_frame).
SlamSequence.push_raw takes the frame as the sensor delivers it (splatam_amd.capture).  arrival_report=True
keeps the reference's on-arrival PSNR record (scripts/ros_handler.py:431-446, 473-481) in `arrival`
(report_arrival).
"""
from __future__ import annotations

import numpy as np
import torch

from .capture import _SequenceBase, _check_policy
from .densify import densify_device
from .densify import make_workspace as make_densify_workspace
from .frame_ops import add_new_gaussians_device, add_new_gaussians_literal, frame_pointcloud, \
    initialize_camera_pose, non_presence_mask, render_depth_sil, write_given_pose
from .keyframes import KeyframeBank, WordFeed, draw_words, make_workspace, pose_w2c, select_device
from .mapper import GraphMapper
from .padded_map import MAP_KEYS, compact_static, densify_static, init_map_device, init_map_literal, is_row_tensor, \
    pad_map
from .perframe import PerFrameSlam
from .seqscore import ViewScorer, ViewScoring
from .slam import MappingConfig, TrackingConfig, color_key
from .tracker import GraphTracker

__all__ = ["SlamSequence", "PerFrameSlam", "ViewScorer", "pad_map", "compact_static", "initialize_camera_pose",
           "non_presence_mask", "init_map_literal", "densify_static", "add_new_gaussians_literal",
           "add_new_gaussians_device", "render_depth_sil", "frame_pointcloud", "_SequenceBase", "_check_policy"]


class SlamSequence(ViewScoring, _SequenceBase):
    """Frames of SplaTAM's loop on a capacity-padded map with one GraphTracker and one GraphMapper.

    params: the initial map (SplaTAM's init from frame 0; isotropic, rgb colours) with one pose column per frame;
    frames: per frame {"im", "depth"} targets (all sharing `cam` / `w2c`, the first frame's, like the reference);
    intrinsics (fx, fy, cx, cy).  frame(t) runs one frame; run(frames) a range of them; push(im, depth) one that
    arrives (num_frames given).  params None: the map is init_map_device's, from frames[0].
    track_frames / track_cam: the tracker's frames and camera at a resolution of their own (everything else
    keeps `frames`); track_size / densify_size (h, w): the sequence makes the tracking / densification frames
    and cameras itself (splatam_amd.resize)."""

    def __init__(self, params: dict, frames: list, cam, w2c, intrinsics, capacity: int, bin_capacity: int,
                 tracking_iters: int = 40, mapping_iters: int = 60, track_replay: int = 20, window: int = 8,
                 keyframe_every: int = 5, sil_thres: float = 0.5, track_cfg: TrackingConfig = TrackingConfig(),
                 map_cfg: MappingConfig = MappingConfig(), prune: bool | None = None, seed: int = 0,
                 scene_radius=None, keyframe_policy: str = "window", overlap_pixels: int = 1600,
                 densify_mode: str = "torch", densify_frames=None, densify_cam=None, densify_intrinsics=None,
                 median_thr=None, median_scale: float = 50.0, num_frames: int | None = None, map_every: int = 1,
                 track_frames=None, track_cam=None, track_size=None, densify_size=None, png_depth_scale=None,
                 max_depth=None, arrival_report: bool = False):
        if params is not None and (color_key(params) != "rgb_colors" or params["log_scales"].shape[1] != 1):
            raise ValueError("SlamSequence: SplaTAM's isotropic rgb map (the tracking fast path's form)")
        if tracking_iters % track_replay:
            raise ValueError("tracking_iters must be a multiple of track_replay")
        self._set_options(locals())
        frames = self.frames  # (raw frames given: their float frames, _ingest_given)
        self.bin_capacity, self.seed = int(bin_capacity), seed
        self.rng = np.random.RandomState(seed)
        self.draws = []  # per frame: the mapper's keyframe draws (window indices; None: the frame did not map); "overlap": the random words
        dev = frames[0]["depth"].device if params is None else params["means3D"].device
        if keyframe_policy == "overlap":
            f0 = frames[0]
            self.bank = KeyframeBank(f0["im"].shape, f0["depth"].shape, dev)
            self.feed = WordFeed(dev)
            self.kf_workspace = make_workspace(f0["depth"].shape[-2], self.overlap_pixels, dev)
            self.selections = []  # per frame: select_device's outputs (device tensors; nothing is read here)
        self.overflow = torch.zeros(1, dtype=torch.bool, device=dev)
        self.dstatus = torch.zeros(4, dtype=torch.int32, device=dev)
        if densify_mode == "device":
            d0 = (self.densify_frames if self.densify_frames is not None else frames)[0]["depth"]
            self.densify_workspace = make_densify_workspace(d0.shape[-2], d0.shape[-1], dev)
        if arrival_report:
            from . import evaluate as ev
            d0 = frames[0]["depth"]
            self.arrival = torch.full((self._n_frames(), 8), float("nan"), dtype=torch.float32, device=dev)
            self.arrival_workspace = ev.make_workspace(d0.shape[-2], d0.shape[-1], dev, ms_ssim=False)
            self.arrival_status = torch.zeros(4, dtype=torch.int32, device=dev)
        padded = None
        if params is None:  # the map is born from frame 0 (initialize_first_timestep), on the device
            kf, intr = self._densify_kf(0)
            padded = init_map_device(kf, w2c, intr, self._n_frames(), int(capacity), overflow=self.overflow,
                                     workspace=getattr(self, "densify_workspace", None))
            params = padded[0]
        self._build(params, int(capacity), padded)

    def _build(self, params: dict, capacity: int, padded=None):
        """The padded map of `params` (its per-Gaussian rows live; `padded`: pad_map's triple, when the caller
        built it) and the tracker / mapper graphs over it."""
        self._retire_scorer()
        self.capacity = capacity
        self.params, self.alive, self.n_live = pad_map(params, self.capacity) if padded is None else padded
        for k in MAP_KEYS:
            self.params[k].requires_grad_(True)
        q, tr = params["cam_unnorm_rots"], params["cam_trans"]
        self.params["cam_unnorm_rots"] = q.detach().clone()
        self.params["cam_trans"] = tr.detach().clone()
        # the tracker's pose slot (one column) and targets: filled per frame; the map tensors as detached views
        # (the same storage: every replay reads the current map; tracking differentiates the pose only)
        self.slot = {k: (v.detach() if k in MAP_KEYS else v) for k, v in self.params.items()}
        self.slot["cam_unnorm_rots"] = q[..., :1].detach().clone().requires_grad_(True)
        self.slot["cam_trans"] = tr[..., :1].detach().clone().requires_grad_(True)
        c0 = self._track_curr(0)  # (the tracking resolution's frame and camera, when the capture has those)
        self.slot_curr = dict(c0, im=c0["im"].clone(), depth=c0["depth"].clone())
        self.tracker = GraphTracker(self.slot, self.slot_curr, 0, iters_per_graph=self.track_replay,
                                    cfg=self.track_cfg, warmup_iters=1, fuse_pose=True, alive=self.alive,
                                    capacity=self.bin_capacity, loss_terms=self.track_cfg.use_depth_loss_thres)
        self.mapper = GraphMapper(self.params, self.keyframes, iters_per_graph=self.mapping_iters, cfg=self.map_cfg,
                                  seed=self.seed, prune=self.prune, scene_radius=self.scene_radius,
                                  alive=self.alive, capacity=self.bin_capacity)
        if self.keyframe_policy == "overlap":
            self.mapper.set_keyframe_bank(self.bank.im, self.bank.depth)

    def ensure_headroom(self, free: int) -> bool:
        """One host read of n_live: when fewer than `free` rows are left, move the map into a larger buffer
        (max(2 x capacity, n_live + free) rows) and rebuild the two graphs -- the live rows and their order
        unchanged, so the results are the same bits.  Every per-Gaussian launch covers the whole capacity
        (bench.py's sequence leg: 45.6 frames/s at 342 k rows, 27.1 at 1.84 M for the same 293 k live
        Gaussians), so size it to the map and grow on demand.  Returns True when it grew (a cached view scorer
        is then stale: the next scoring call rebuilds it, counted in scorer_captures)."""
        n = int(self.n_live.item())
        if self.capacity - n >= free:
            return False
        self._build(self.live_params(), max(2 * self.capacity, n + int(free)))
        return True

    def track(self, t: int):
        """initialize_camera_pose, then tracking_iters iterations from the pose slot (best candidate written
        back into column t); with track_cfg.use_depth_loss_thres, once more unless the depth loss fell below the
        threshold (one host read).  Returns the iterations run."""
        p = self.params
        initialize_camera_pose(p, t)
        with torch.no_grad():
            self.slot["cam_unnorm_rots"][..., 0] = p["cam_unnorm_rots"][..., t]
            self.slot["cam_trans"][..., 0] = p["cam_trans"][..., t]
            curr = self._track_curr(t)
            self.slot_curr["im"].copy_(curr["im"])
            self.slot_curr["depth"].copy_(curr["depth"])
        ran = self.tracker.track_frame(self.tracking_iters, check=False, depth_loss_thres=self._depth_loss_thres())
        with torch.no_grad():
            p["cam_unnorm_rots"][..., t] = self.slot["cam_unnorm_rots"][..., 0]
            p["cam_trans"][..., t] = self.slot["cam_trans"][..., 0]
        return ran

    def densify(self, t: int):
        """add_new_gaussians without a host read.  densify_mode "torch": densify_static; "device": the
        silhouette render, then splatam_amd.densify.densify_device (one call, only the new rows written)."""
        kf, intr = self._densify_kf(t)
        if self.densify_mode == "torch":
            densify_static(self.params, self.alive, self.n_live, self.overflow, kf, t, intr,
                           self.sil_thres, self.capacity, self.bin_capacity, self.dstatus, self.median_thr,
                           self.median_scale)
            return
        ds = render_depth_sil(self.params, kf, t, self.alive, self.bin_capacity, self.dstatus)
        densify_device(self.params, self.alive, self.n_live, self.overflow, kf, pose_w2c(self.params, t), intr,
                       self.sil_thres, self.capacity, ds, self.densify_workspace, median_thr=self.median_thr,
                       median_scale=self.median_scale)

    def map(self, t: int, sequence=None):
        """The mapping frame over the window (the last window - 1 keyframes + frame t), keyframe draws from the
        sequence's numpy stream (np.random.randint, scripts/splatam.py:851) unless `sequence` is given.
        keyframe_policy "overlap": _map_overlap (`sequence`: the frame's random words)."""
        if self.keyframe_policy == "overlap":
            return self._map_overlap(t, sequence)
        win = self._window(t)
        self.mapper.set_keyframes(win)
        seq = [int(self.rng.randint(0, len(win))) for _ in range(self.mapping_iters)] if sequence is None else sequence
        self.draws.append(seq)
        self.mapper.run(check=False, sequence=seq)
        self._compact_pruned()
        self._add_keyframe(t)

    def _add_keyframe(self, t: int):
        """The keyframe bookkeeping after a frame (scripts/splatam.py:907-913, 932-945), mapped or not."""
        if not self._is_keyframe(t):
            return
        if self.keyframe_policy == "overlap":
            f = self.frames[t]
            if self.bank.append(f["im"], f["depth"], self.params, t):  # (the bank doubled: new tensors)
                self.mapper.set_keyframe_bank(self.bank.im, self.bank.depth)
        else:
            self.keyframes.append(self._kf(t))

    def _compact_pruned(self):
        if self.mapper.prune_at:  # the frame's pruned Gaussians removed for good (in place, no sync)
            compact_static(self.params, self.alive, self.n_live, self.capacity)

    def _map_overlap(self, t: int, words=None):
        """The mapping frame under the overlap policy, without a host read: the frame into the bank's last
        row, the frame's random words (overlap_pixels for the sample, one key per candidate keyframe,
        one per mapping iteration) to the device, select_device, the mapper's replay from its draws, and the
        keyframe bookkeeping of scripts/splatam.py:932-945."""
        bank, f = self.bank, self.frames[t]
        bank.set_current(f["im"], f["depth"])
        S, n_cand, total = self._word_counts(bank.n)
        words = draw_words(self.rng, total) if words is None else \
            np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
        if words.shape != (total,):
            raise ValueError(f"frame {t}: {total} random words")
        self.draws.append(words)
        w = self.feed.push(words)
        sel = select_device(f["depth"], self.intrinsics, pose_w2c(self.params, t), bank.est_w2c, bank.n,
                            self.window - 2, w[:S], w[S:S + n_cand], w[S + n_cand:], bank.time, t, bank.cur_row,
                            workspace=self.kf_workspace)
        self.selections.append(sel)
        self.mapper.run(check=False, device_sequence=(sel["draw_rows"], sel["draw_times"]))
        self._compact_pruned()
        self._add_keyframe(t)

    def frame(self, t: int, sequence=None, w2c=None):
        """One frame of scripts/splatam.py:697-929: tracking (t > 0), densification (t > 0), mapping.
        w2c (device [4,4], the frame's pose relative to frame 0; tracking.use_gt_poses): the frame is not tracked,
        write_given_pose fills column t (ignored for frame 0, whose column is the identity).  A frame that does
        not map (map_every) does not densify either; its keyframe bookkeeping still runs."""
        ran = 0
        if t > 0:
            if w2c is None:
                ran = self.track(t)
            else:
                write_given_pose(self.params, t, w2c)
            if self.arrival_report:
                self.report_arrival(t)
            if self._maps(t):
                self.densify(t)
        self.tracking_iters_run.append(ran)
        if self._maps(t):
            self.map(t, sequence)
        else:
            self.draws.append(None)
            self._add_keyframe(t)

    def report_arrival(self, t: int):
        """The reference's on-arrival record (scripts/ros_handler.py:431-446, 473-481: gain_psnr_arr's "psnr"):
        frame t rendered at its pose column from the map as it stands BEFORE the frame's densification and
        mapping (one evaluate.render_frame: the static forward under the alive mask), and the metrics of render
        against frame under the valid-depth mask (one evaluate.frame_metrics, no MS-SSIM) into row t of
        `arrival` [num_frames, 8] (evaluate.COLUMNS; NaN where nothing was reported: frame 0, the MS-SSIM
        column).  Nothing is read back.  The gains of the same record are view_gains'."""
        from . import evaluate as ev
        f = self.frames[t]
        im, ds = ev.render_frame(self.params, t, self.cam, self.w2c, self.alive, self.bin_capacity,
                                 self.arrival_status)
        ev.frame_metrics(im, ds, f["im"], f["depth"], self.sil_thres, self.arrival[t], self.arrival_workspace,
                         use_sil_mask=False, ms_ssim=False)

    def run(self, frames=None):
        """frame(t) for every t of `frames` (an iterable; default: the frames in the list that have not run)."""
        for t in (range(len(self.tracking_iters_run), len(self.frames)) if frames is None else frames):
            self.frame(t)

    def push(self, im: torch.Tensor, depth: torch.Tensor, w2c=None, densify_frame=None) -> int:
        """A frame that arrives (the realtime loop, scripts/splatam_realtime.py): appended to the frame list and
        run as frame t = len(frames) - 1, with its pose when `w2c` is given (frame()).  Needs num_frames: the
        pose tensors have that many columns, and a frame beyond them raises ValueError.  densify_frame
        {"im", "depth"}: the frame at the densification resolution, for a capture with densify_frames.
        Under densify_size / track_size the sequence makes the small frames itself (one gsr_resize_frame
        launch) and the caller pushes the full frame alone.  A capture with track_frames goes through
        push_frames.  Returns t.  Nothing is read back (but see track_cfg.use_depth_loss_thres)."""
        return self.push_frames(im, depth, w2c=w2c, densify_frame=densify_frame)

    def push_frames(self, im: torch.Tensor, depth: torch.Tensor, w2c=None, densify_frame=None, track_frame=None) -> int:
        """push() with the frame at the tracking resolution: track_frame {"im", "depth"}, for a capture with
        track_frames (one per frame, by the rule of densify_frame)."""
        t = self._append_frame(im, depth, densify_frame, track_frame)
        self.frame(t, w2c=w2c)
        return t

    def push_raw(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor, pose=None, w2c=None) -> int:
        """push() for the frame as the sensor delivers it (scripts/ros_handler.py:402-411): rgb_u8 [H,W,3] uint8,
        depth_u16 [H,W] uint16 in sensor units (png_depth_scale per metre; max_depth marks far readings -1) --
        splatam_amd.ingest.  One gsr_ingest_frame launch makes the float frame and, under track_size /
        densify_size, the small frames (no gsr_resize_frame launch for this frame); then push_frames'
        bookkeeping and frame(t, w2c=...).  pose: the odometry pose (x, y, z, qx, qy, qz, qw), made relative to
        the first pose pushed (ingest.odometry_w2c; host float64, a non-blocking copy to the device); w2c: as
        in push().  ValueError: both given, no png_depth_scale, or a capture with explicit track_frames /
        densify_frames (those callers own their small frames: push_frames).  Returns t.  Nothing is read back."""
        t, w2c = self._push_raw_frame(rgb_u8, depth_u16, pose, w2c)
        self.frame(t, w2c=w2c)
        return t

    def _bin_overflowed(self, status: torch.Tensor) -> bool:
        """Whether a render's status (device int32 [4]) shows more instances than bin_capacity or a prefiltered
        violation.  One host read."""
        st = status.cpu()
        return int(st[0]) > self.bin_capacity or int(st[1]) != 0

    def check(self):
        """One host synchronisation: raises if a binning capacity or the map capacity overflowed."""
        if self.tracker.overflowed() or self.mapper.overflowed() or bool(self.overflow.item()):
            raise RuntimeError("SlamSequence: a binning capacity or the map capacity was exceeded")
        st = [self.dstatus] + ([self.arrival_status] if self.arrival_report else [])
        if any(self._bin_overflowed(s) for s in st):
            raise RuntimeError("SlamSequence: the densification (or arrival) render overflowed its binning capacity")

    def evaluate(self, gt_w2c=None, eval_every: int = 1, ms_ssim: bool = True) -> dict:
        """The reference's end-of-run eval() (utils/eval_helpers.py:408-640) of the padded map as it stands
        against the capture: splatam_amd.evaluate.evaluate_sequence with the alive mask (one dual render and
        one row of device metrics per evaluated frame, nothing read back), then the one host read of
        evaluate.summarize.  gt_w2c ([num_frames, 4, 4] or a list): adds "ate_rmse", the estimated
        trajectory being the first frame's w2c and the pose columns of frames 1 .. (:556-575)."""
        from . import evaluate as ev
        status = torch.zeros(4, dtype=torch.int32, device=self.alive.device)
        table, times = ev.evaluate_sequence(self.params, self.frames, self.cam, self.w2c, sil_thres=self.sil_thres,
                                            eval_every=eval_every, use_sil_mask=False, ms_ssim=ms_ssim,
                                            alive=self.alive, bin_capacity=self.bin_capacity, status=status)
        ate = None
        if gt_w2c is not None:
            est = [self.w2c] + [pose_w2c(self.params, t) for t in range(1, len(self.frames))]
            ate = ev.ate_rmse(gt_w2c, est)
        out = ev.summarize(table, times, ate)
        if self._bin_overflowed(status):
            raise RuntimeError("SlamSequence.evaluate: a render overflowed its binning capacity")
        out["table"] = table
        return out

    def live_params(self) -> dict:
        """The live rows (slot order) of every per-Gaussian tensor, and the camera tensors."""
        keep = self.alive.bool()
        return {k: (v.detach()[keep] if is_row_tensor(k, v, keep.shape[0]) else v) for k, v in self.params.items()}
