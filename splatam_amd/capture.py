"""A capture as SlamSequence and PerFrameSlam (splatam_amd.sequence, splatam_amd.perframe) hold it: the loop's
options, the frame store with its small frames, the intake of a frame that arrives, and the keyframe rule.

With densify_frames / densify_cam / densify_intrinsics densification renders and reads a densification frame of
its own resolution (the reference's densification_image_height / width, scripts/splatam.py:801-812).  With
track_frames / track_cam the tracker renders and compares against a tracking frame of its own resolution (the
reference's tracking_image_height / width, scripts/splatam.py:517-523, 588-607, 680-687 -- what makes
configs/replica/splatam_s.py "SplaTAM-S"): only the tracker's slot holds it; densification, the keyframe dicts
and bank, mapping, evaluate() and the view scorer keep the full-resolution frames, as in the reference, where
only tracking_curr_data differs.  track_size / densify_size (h, w) have the capture make those frames itself:
the cameras and intrinsics through splatam_amd.resize (resized_camera, scale_intrinsics), each frame's small
copies by one gsr_resize_frame launch (resize.resize_device) -- at construction for the frames given, in
_append_frame for a frame that arrives, so the realtime loop's caller pushes the full frame and nothing else.

The realtime loop's frames arrive as the sensor delivers them (scripts/ros_handler.py:402-411): an interleaved
uint8 image, a uint16 depth image and an odometry pose.  _push_raw_frame takes exactly that (png_depth_scale,
max_depth): one gsr_ingest_frame launch (splatam_amd.ingest) writes the float frame and, under track_size /
densify_size, the small frames -- no gsr_resize_frame launch for such a frame -- and ingest.odometry_w2c makes
the pose relative to the first one on the host.  Raw frames given at construction ({"rgb_u8", "depth_u16"[,
"pose"]}) are ingested before anything reads them.
"""
from __future__ import annotations

import numpy as np
import torch

from .densify import check_densify_args
from .ingest import ingest_device, odometry_w2c
from .resize import check_track_args, resize_device, resized_camera, scale_intrinsics


def _check_policy(keyframe_policy: str, window: int):
    if keyframe_policy not in ("window", "overlap"):
        raise ValueError(f"keyframe_policy {keyframe_policy!r}: 'window' or 'overlap'")
    if keyframe_policy == "overlap" and window < 2:
        raise ValueError("keyframe_policy 'overlap' needs window >= 2 (the last keyframe and the current frame)")


class _SequenceBase:
    """What SlamSequence and PerFrameSlam share: the loop's options, the keyframe dicts, the densification frame,
    the "window" policy's window, both policies' keyframe rule and an "overlap" frame's random-word counts."""

    OPTIONS = ("frames", "cam", "w2c", "intrinsics", "bin_capacity", "tracking_iters", "mapping_iters", "track_replay",
               "window", "keyframe_every", "sil_thres", "track_cfg", "map_cfg", "prune", "scene_radius",
               "keyframe_policy", "overlap_pixels", "densify_mode", "densify_frames", "densify_cam",
               "densify_intrinsics", "median_thr", "median_scale", "num_frames", "map_every", "track_frames",
               "track_cam", "track_size", "densify_size", "png_depth_scale", "max_depth", "arrival_report")

    def _set_options(self, args: dict):
        """Stores the constructor arguments both classes take (OPTIONS, out of the constructor's locals()) as
        attributes of their names, validated, and starts the keyframe list with frame 0."""
        for k in self.OPTIONS:
            setattr(self, k, args[k])
        _check_policy(self.keyframe_policy, self.window)
        if self.num_frames is not None and not 1 <= len(self.frames) <= int(self.num_frames):
            raise ValueError(f"num_frames {self.num_frames}: between 1 and num_frames frames to start with")
        if int(self.map_every) < 1:
            raise ValueError("map_every >= 1")
        premade = self._ingest_given()
        check_densify_args(self.densify_mode, self.densify_frames, self.densify_cam, self.densify_intrinsics,
                           self.frames)
        check_track_args(self.track_frames, self.track_cam, self.frames)
        self._set_sizes(premade)
        self.overlap_pixels = int(self.overlap_pixels)
        if self.scene_radius is None:  # initialize_first_timestep: max depth / scene_radius_depth_ratio (3, the config's)
            self.scene_radius = self.frames[0]["depth"].max() / 3.0
        self.keyframes = [self._kf(0)]
        self.tracking_iters_run = []  # per frame() call: the tracking iterations run (0: frame 0, not tracked)

    def _owns_small_frames(self) -> bool:
        """Whether the caller gives the small frames (track_frames / densify_frames without track_size /
        densify_size): such a capture is not fed raw frames."""
        return (self.track_frames is not None and self.track_size is None) or \
            (self.densify_frames is not None and self.densify_size is None)

    def _sizes(self) -> list:
        """The sizes set, in the order one launch makes their frames: track_size, then densify_size."""
        return [s for s in (self.track_size, self.densify_size) if s is not None]

    def _small_pair(self, made) -> tuple:
        """(tracking frame, densification frame), None where track_size / densify_size is unset, out of the
        frames a launch made for _sizes(): the small pair."""
        made = iter(made)
        return tuple(next(made) if s is not None else None for s in (self.track_size, self.densify_size))

    def _make_small(self, frame: dict) -> tuple:
        """The small pair of a full frame: one gsr_resize_frame launch for both, nothing read back."""
        sizes = self._sizes()
        if not sizes:
            return None, None
        made = resize_device(frame, *sizes)
        return self._small_pair(made if len(sizes) == 2 else (made,))

    def _ingest_raw(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor) -> tuple:
        """(frame, tracking frame, densification frame) of a raw sensor frame (splatam_amd.ingest: uint8 [H,W,3],
        uint16 [H,W]) under png_depth_scale / max_depth: one gsr_ingest_frame launch for the frame and its small
        pair, nothing read back."""
        sizes = self._sizes()
        out = ingest_device(rgb_u8, depth_u16, self.png_depth_scale, self.max_depth, *sizes)
        return (out[0], *self._small_pair(out[1:])) if sizes else (out, None, None)

    def _need_scale(self, who: str):
        if self.png_depth_scale is None:
            raise ValueError(f"{who} needs png_depth_scale (the sensor units per metre)")

    def _ingest_given(self):
        """Raw frames given at construction ({"rgb_u8", "depth_u16"[, "pose"]} each, with png_depth_scale): the
        frame list becomes their float frames (a new list), before anything reads a frame.  Returns per frame
        the small pair the same launch made, for _set_sizes; None for float frames.
        The first frame's "pose" (x, y, z, qx, qy, qz, qw), when given, is what push_raw's poses are relative to."""
        self.initial_pose = None
        raw = ["rgb_u8" in f for f in self.frames]
        if not any(raw):
            return None
        if not all(raw):
            raise ValueError("frames: raw ({'rgb_u8', 'depth_u16'}) or float ({'im', 'depth'}), not both")
        if self._owns_small_frames():
            raise ValueError("raw frames: a capture with track_frames / densify_frames owns its small frames")
        self._need_scale("a raw frame")
        given = self.frames
        made = [self._ingest_raw(f["rgb_u8"], f["depth_u16"]) for f in given]
        self.frames = [m[0] for m in made]
        if given[0].get("pose") is not None:
            self.initial_pose = np.array(given[0]["pose"], dtype=np.float64)
        return [m[1:] for m in made]

    def _set_sizes(self, premade=None):
        """track_size / densify_size (h, w): the sequence makes the small frames itself -- the camera (and the
        densification intrinsics) through splatam_amd.resize, the frames given so far by one gsr_resize_frame
        launch each (_make_small; `premade`: _ingest_given's, for raw frames, whose ingest launch made them).
        Exclusive with track_frames / densify_frames."""
        if self.track_size is not None and self.track_frames is not None:
            raise ValueError("track_size: exclusive with track_frames / track_cam")
        if self.densify_size is not None and self.densify_frames is not None:
            raise ValueError("densify_size: exclusive with densify_frames / densify_cam / densify_intrinsics")
        if self.track_size is None and self.densify_size is None:
            return
        d0 = self.frames[0]["depth"]
        H, W, dev = int(d0.shape[-2]), int(d0.shape[-1]), d0.device
        w2c = None if self.w2c is None else self.w2c.detach().cpu()
        if self.track_size is not None:
            self.track_size = tuple(int(v) for v in self.track_size)
            self.track_cam = resized_camera(W, H, self.intrinsics, *self.track_size, dev, w2c=w2c)
            self.track_frames = []
        if self.densify_size is not None:
            self.densify_size = tuple(int(v) for v in self.densify_size)
            self.densify_cam = resized_camera(W, H, self.intrinsics, *self.densify_size, dev, w2c=w2c)
            self.densify_intrinsics = scale_intrinsics(self.intrinsics, H, W, *self.densify_size)
            self.densify_frames = []
        for i, f in enumerate(self.frames):
            tf, df = self._make_small(f) if premade is None else premade[i]
            if tf is not None:
                self.track_frames.append(tf)
            if df is not None:
                self.densify_frames.append(df)

    def _next_index(self) -> int:
        """The index a frame that arrives gets; ValueError beyond num_frames (the pose columns)."""
        t = len(self.frames)
        if self.num_frames is None or t >= int(self.num_frames):
            raise ValueError(f"frame {t}: the sequence holds num_frames = {self.num_frames} frames")
        return t

    def _append_frame(self, im: torch.Tensor, depth: torch.Tensor, densify_frame=None, track_frame=None,
                      made=None) -> int:
        """A frame that arrived: appended to the frame list (and its densification frame to densify_frames, its
        tracking frame to track_frames, when the capture has those; under densify_size / track_size the sequence
        makes them here, _make_small, and takes none -- unless `made`, the small pair _ingest_raw's launch made
        already).  Returns its index; ValueError beyond num_frames (the pose columns)."""
        t = self._next_index()
        if (densify_frame is not None and self.densify_size is not None) or \
                (track_frame is not None and self.track_size is not None):
            raise ValueError("densify_size / track_size: the sequence makes that frame itself")
        if self.densify_size is None and (densify_frame is None) != (self.densify_frames is None):
            raise ValueError("densify_frame: one per frame when the capture has densify_frames, else none")
        if self.track_size is None and (track_frame is None) != (self.track_frames is None):
            raise ValueError("track_frame: one per frame when the capture has track_frames, else none")
        made_t, made_d = self._make_small({"im": im, "depth": depth}) if made is None else made
        track_frame = made_t if track_frame is None else track_frame
        densify_frame = made_d if densify_frame is None else densify_frame
        self.frames.append({"im": im, "depth": depth})
        if densify_frame is not None:
            self.densify_frames.append(densify_frame)
        if track_frame is not None:
            self.track_frames.append(track_frame)
        return t

    def _push_raw_frame(self, rgb_u8: torch.Tensor, depth_u16: torch.Tensor, pose=None, w2c=None) -> tuple:
        """push_raw's intake (SlamSequence.push_raw states it): every check before the one gsr_ingest_frame launch,
        so a refused call appends nothing; _append_frame's bookkeeping without _make_small; the pose against the
        first one pushed (or the first raw frame's "pose").  Returns (t, w2c)."""
        self._need_scale("push_raw")
        if pose is not None and w2c is not None:
            raise ValueError("push_raw: pose or w2c, not both")
        if self._owns_small_frames():
            raise ValueError("push_raw: a capture with track_frames / densify_frames owns its small frames "
                             "(push_frames)")
        self._next_index()
        frame, *made = self._ingest_raw(rgb_u8, depth_u16)
        t = self._append_frame(frame["im"], frame["depth"], made=made)
        if pose is not None:
            if self.initial_pose is None:
                self.initial_pose = np.array(pose, dtype=np.float64)
            w2c = odometry_w2c(self.initial_pose, pose, device=frame["depth"].device)
        return t, w2c

    def _depth_loss_thres(self):
        """GraphTracker.track_frame's depth_loss_thres: the configured threshold, or None (option off)."""
        cfg = self.track_cfg
        return float(cfg.depth_loss_thres) if cfg.use_depth_loss_thres else None

    def _n_frames(self) -> int:
        """The capture's length: num_frames when given (the frame list may still be growing), else the list's."""
        return len(self.frames) if self.num_frames is None else int(self.num_frames)

    def _maps(self, t: int) -> bool:
        """Whether frame t densifies and maps (map_every, scripts/splatam_realtime.py:844): frame 0 always."""
        return t == 0 or (t + 1) % int(self.map_every) == 0

    def _kf(self, t: int) -> dict:
        return {"cam": self.cam, "w2c": self.w2c, "im": self.frames[t]["im"], "depth": self.frames[t]["depth"], "id": t}

    def _track_curr(self, t: int) -> dict:
        """What the tracker renders and compares against for frame t: the frame itself, or the tracking
        resolution's (track_frames / track_cam, scripts/splatam.py:588-607, 680-687); w2c stays the first frame's."""
        f, cam = (self.frames[t], self.cam) if self.track_frames is None else (self.track_frames[t], self.track_cam)
        return {"cam": cam, "w2c": self.w2c, "im": f["im"], "depth": f["depth"]}

    def _densify_kf(self, t: int) -> tuple[dict, tuple]:
        """The frame densification reads and its intrinsics: the tracking frame, or the densification
        resolution's (densify_frames / densify_cam / densify_intrinsics, scripts/splatam.py:801-812)."""
        if self.densify_frames is None:
            return self._kf(t), self.intrinsics
        f = self.densify_frames[t]
        return dict(self._kf(t), cam=self.densify_cam, im=f["im"], depth=f["depth"]), self.densify_intrinsics

    def _window(self, t: int) -> list:  # "window": the last window - 1 keyframes plus frame t
        return self.keyframes[-(self.window - 1):] + ([self._kf(t)] if self.keyframes[-1]["id"] != t else [])

    def _is_keyframe(self, t: int) -> bool:
        """Whether frame t joins the keyframes after its mapping: every keyframe_every-th frame
        (scripts/splatam.py:907-913; frame 0 is one from the start) and, "overlap" (:932), frames 0 and num_frames - 2."""
        every = (t + 1) % self.keyframe_every == 0
        if self.keyframe_policy == "overlap":
            return every or t in (0, self._n_frames() - 2)
        return every and t > 0

    def _word_counts(self, n_kf: int) -> tuple[int, int, int]:
        """An "overlap" frame's random words with n_kf keyframes: the sample's, the candidate keyframes' keys, and
        all of them (with one per mapping iteration)."""
        S, n_cand = self.overlap_pixels, max(n_kf - 1, 0)
        return S, n_cand, S + n_cand + self.mapping_iters
