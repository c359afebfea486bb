"""SplaTAM's per-frame loop in the form a shape-changing map forces on captured graphs: the comparison loop for
SlamSequence (splatam_amd.sequence), on the same capture (splatam_amd.capture) and the same frame steps
(splatam_amd.frame_ops)."""
from __future__ import annotations

import torch

from .capture import _SequenceBase
from .frame_ops import add_new_gaussians_device, add_new_gaussians_literal, initialize_camera_pose, write_given_pose
from .keyframes import pose_w2c, select_literal, words_tensor
from .mapper import GraphMapper
from .padded_map import MAP_KEYS
from .slam import MappingConfig, TrackingConfig
from .tracker import GraphTracker


class PerFrameSlam(_SequenceBase):
    """The same frames in the form a shape-changing map forces on captured graphs: per frame a fresh
    GraphTracker on the frame's pose (probe, warm-up, capture), add_new_gaussians by torch.cat, a fresh
    GraphMapper on the grown map (probe, warm-up, capture) and, after its pruning, compact().  The comparison
    form for SlamSequence (tests/test_gpu_sequence.py; bench.py's sequence leg times both).  bin_capacity None:
    each tracker / mapper probes its own (what a per-frame loop must do); given: every one uses it."""

    def __init__(self, params: dict, frames: list, cam, w2c, intrinsics, tracking_iters: int = 40,
                 mapping_iters: int = 60, track_replay: int = 20, window: int = 8, keyframe_every: int = 5,
                 sil_thres: float = 0.5, track_cfg: TrackingConfig = TrackingConfig(),
                 map_cfg: MappingConfig = MappingConfig(), prune: bool | None = None, scene_radius=None,
                 bin_capacity: int | None = None, keyframe_policy: str = "window", overlap_pixels: int = 1600,
                 densify_mode: str = "torch", densify_frames=None, densify_cam=None, densify_intrinsics=None,
                 median_thr=None, median_scale: float = 50.0, num_frames: int | None = None, map_every: int = 1,
                 track_frames=None, track_cam=None, track_size=None, densify_size=None, png_depth_scale=None,
                 max_depth=None, arrival_report: bool = False):
        self._set_options(locals())
        self.arrival = {}  # arrival_report: per reported frame, evaluate_literal's row of the on-arrival render
        self.kf_list = []  # "overlap": the keyframes in the order appended, each with its est_w2c snapshot
        self.windows = []  # "overlap": per frame, the selected window's time indices
        self.p = {k: v.detach().clone() for k, v in params.items()}

    def frame(self, t: int, sequence, w2c=None):
        p = self.p
        ran = 0
        if t > 0 and w2c is not None:
            write_given_pose(p, t, w2c)
        elif t > 0:
            initialize_camera_pose(p, t)
            tp = dict(p)
            tp["cam_unnorm_rots"] = p["cam_unnorm_rots"][..., t:t + 1].clone().requires_grad_(True)
            tp["cam_trans"] = p["cam_trans"][..., t:t + 1].clone().requires_grad_(True)
            tracker = GraphTracker(tp, self._track_curr(t), 0, iters_per_graph=self.track_replay, cfg=self.track_cfg, warmup_iters=1,
                                   fuse_pose=True, capacity=self.bin_capacity,
                                   loss_terms=self.track_cfg.use_depth_loss_thres)
            ran = tracker.track_frame(self.tracking_iters, depth_loss_thres=self._depth_loss_thres())
            with torch.no_grad():
                p["cam_unnorm_rots"][..., t] = tp["cam_unnorm_rots"][..., 0]
                p["cam_trans"][..., t] = tp["cam_trans"][..., 0]
        if t > 0 and self.arrival_report:  # (SlamSequence.report_arrival's point, in plain renders and torch ops)
            from . import evaluate as ev
            f = self.frames[t]
            self.arrival[t] = ev.evaluate_literal(*ev.render_frame(p, t, self.cam, self.w2c), f["im"], f["depth"],
                                                  self.sil_thres, ms_ssim=False)
        if t > 0 and self._maps(t):
            kf, intr = self._densify_kf(t)
            add = add_new_gaussians_device if self.densify_mode == "device" else add_new_gaussians_literal
            p = add(p, kf, t, intr, self.sil_thres, self.median_thr, self.median_scale)
        self.tracking_iters_run.append(ran)
        if not self._maps(t):
            self._add_keyframe(t)
            return
        mp = {k: (v.detach().requires_grad_(True) if k in MAP_KEYS else v) for k, v in p.items()}
        if self.keyframe_policy == "overlap":
            win, sequence = self._select_overlap(p, t, sequence)
        else:
            win = self._window(t)
        m = GraphMapper(mp, win, iters_per_graph=self.mapping_iters, cfg=self.map_cfg, seed=0, prune=self.prune,
                        scene_radius=self.scene_radius, capacity=self.bin_capacity)
        m.run(sequence=sequence)
        if m.prune_at:
            mp, _, _ = m.compact()
        self.p = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in mp.items()}
        self._add_keyframe(t)

    def push_raw(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor, sequence=None, pose=None, w2c=None) -> int:
        """SlamSequence.push_raw for this loop: the same intake (one gsr_ingest_frame launch, the bookkeeping,
        the pose), then frame(t, sequence, w2c=...) with the mapper's draws `sequence`.  Needs num_frames."""
        t, w2c = self._push_raw_frame(rgb_u8, depth_u16, pose, w2c)
        self.frame(t, sequence, w2c=w2c)
        return t

    def _add_keyframe(self, t: int):
        if not self._is_keyframe(t):
            return
        if self.keyframe_policy == "overlap":
            self.kf_list.append(dict(self._kf(t), est_w2c=pose_w2c(self.p, t)))
        else:
            self.keyframes.append(self._kf(t))

    def _select_overlap(self, p: dict, t: int, words):
        """keyframes.select_literal on the frame's random words (SlamSequence.draws[t]): the window's keyframe
        dicts and the per-iteration window indices, for the per-frame GraphMapper's host path."""
        dev = p["means3D"].device
        n_kf = len(self.kf_list)
        w = words_tensor(words, dev)
        S, n_cand, total = self._word_counts(n_kf)
        if w.numel() != total:
            raise ValueError(f"frame {t}: {total} random words")
        kf_w2c = torch.stack([kf["est_w2c"].reshape(16) for kf in self.kf_list]) if n_kf else \
            torch.zeros(0, 16, device=dev)
        kf_time = torch.tensor([kf["id"] for kf in self.kf_list], dtype=torch.int64, device=dev)
        sel = select_literal(self.frames[t]["depth"], self.intrinsics, pose_w2c(p, t), kf_w2c, n_kf, self.window - 2,
                             w[:S], w[S:S + n_cand], w[S + n_cand:], kf_time, t, n_kf)
        rows = sel["window"][:int(sel["n_window"])].tolist()
        self.windows.append([t if r == n_kf else self.kf_list[r]["id"] for r in rows])
        return [self._kf(t) if r == n_kf else self.kf_list[r] for r in rows], sel["draw_index"].tolist()
