"""SHA-256 digests of what the sequence loops compute on a tiny capture: the check that a change to the Python
side of splatam_amd.sequence / splatam_amd.fisher (a move, a merge) left every result bit for bit.

Capture: make_scene(3000, 64, 48, seed=7) through sequence_workload, 4 frames; tracking_iters=10, track_replay=10,
mapping_iters=10, keyframe_every=2, window=3, prune=True, seed=0.  Three SlamSequence runs --

  window    keyframe_policy "window", densify_mode "torch"
  overlap   keyframe_policy "overlap", densify_mode "device", track_size=(24, 32)
  raw       fed raw frames (the first at construction, the others by push_raw with odometry poses),
            densify_mode "device", track_size / densify_size (24, 32), arrival_report=True

-- each followed by view_scorer(K=4, seed=3), fit_visited(check=True), view_gains of five candidates,
ensure_headroom(capacity) (which grows the map and retires the scorer) and view_gains again; and PerFrameSlam on
the frames and draws of "window" and "overlap".  One line per item: its name and the SHA-256 of its bytes.

Run it on two commits, each in a process of its own, and compare the outputs: every line must be identical.
Needs a GPU (no fallback).
Usage: python tools/sequence_digest.py [--out FILE]"""
import argparse
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

N, SMALL, PNG_SCALE, MAX_DEPTH = 4, (24, 32), 1000.0, 20.0
KW = dict(tracking_iters=10, track_replay=10, mapping_iters=10, keyframe_every=2, window=3, prune=True)
LINES = []


def emit(name: str, value):
    if torch.is_tensor(value):
        value = value.detach().cpu().contiguous().numpy()
    data = value.tobytes() if isinstance(value, np.ndarray) else repr(value).encode()
    LINES.append(f"{name} {hashlib.sha256(data).hexdigest()}")
    print(LINES[-1], flush=True)


def pose(deg: float, t, dev) -> torch.Tensor:
    a = math.radians(deg)
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    w2c[:3, 3] = torch.tensor(t)
    return w2c.to(dev)


def quantise(frame: dict):
    """A float frame as a sensor delivers it: uint8 [H,W,3], uint16 [H,W] in 1 / PNG_SCALE m."""
    rgb = (frame["im"].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    d = (frame["depth"][0].clamp(0, 30) * PNG_SCALE).round().to(torch.int32)
    return rgb, (d & 0xFFFF).to(torch.int16).contiguous().view(torch.uint16)


def odometry(t: int) -> np.ndarray:
    """Frame t's camera-to-world pose (x, y, z, qx, qy, qz, qw) on sequence_workload's trajectory (2 cm along x
    and 0.3 degrees about y per frame, as w2c)."""
    a = math.radians(0.3 * t)
    c, s = math.cos(a), math.sin(a)
    rt = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])  # Ry(a)^T
    return np.array([*(-rt @ np.array([0.02 * t, 0.0, 0.0])), 0.0, math.sin(-a / 2), 0.0, math.cos(-a / 2)])


def digest_sequence(tag: str, seq, cands):
    seq.check()
    emit(f"{tag}.cam_unnorm_rots", seq.params["cam_unnorm_rots"])
    emit(f"{tag}.cam_trans", seq.params["cam_trans"])
    for k, v in sorted(seq.live_params().items()):
        if torch.is_tensor(v) and k not in ("cam_unnorm_rots", "cam_trans"):
            emit(f"{tag}.live.{k}", v)
    emit(f"{tag}.n_live", int(seq.n_live.item()))
    emit(f"{tag}.draws", [None if d is None else np.asarray(d).tolist() for d in seq.draws])
    emit(f"{tag}.tracking_iters_run", list(seq.tracking_iters_run))
    if seq.arrival_report:
        emit(f"{tag}.arrival", seq.arrival)
    seq.view_scorer(K=4, seed=3)
    h = seq.fit_visited(check=True)
    emit(f"{tag}.H_train_inv", h[seq.alive.bool()])
    emit(f"{tag}.gains", seq.view_gains(cands, check=True))
    emit(f"{tag}.grew", seq.ensure_headroom(seq.capacity))
    emit(f"{tag}.gains_after_growth", seq.view_gains(cands, check=True))
    emit(f"{tag}.scorer_captures", seq.scorer_captures)
    seq.check()


def digest_per_frame(tag: str, per, draws):
    for t in range(N):
        per.frame(t, draws[t])
    for k, v in sorted(per.p.items()):
        if torch.is_tensor(v):
            emit(f"{tag}.{k}", v)
    emit(f"{tag}.tracking_iters_run", list(per.tracking_iters_run))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sequence_digest needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    from splatam_amd.scenes import make_scene
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload

    scene = make_scene(3000, 64, 48, seed=7)
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, N, dev, prunable=0.02)
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = params["means3D"].shape[0] + 2 * 64 * 48, 4 * n + 100_000
    cands = [pose(-3.0 + 1.5 * j, [0.05, 0.01 * (j % 4), -0.02 * (j % 3)], dev) for j in range(5)]
    configs = {"window": dict(keyframe_policy="window", densify_mode="torch"),
               "overlap": dict(keyframe_policy="overlap", densify_mode="device", track_size=SMALL)}
    for tag, kw in configs.items():
        seq = SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                           **dict(KW, **kw))
        seq.run()
        digest_sequence(tag, seq, cands)
        per = PerFrameSlam(params, frames, cam, w2c, intr, bin_capacity=bin_cap, **dict(KW, **kw))
        digest_per_frame(f"{tag}.per_frame", per, seq.draws)

    raw = [quantise(f) for f in frames]
    first = [{"rgb_u8": raw[0][0], "depth_u16": raw[0][1], "pose": odometry(0)}]
    seq = SlamSequence(params, first, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0, num_frames=N,
                       densify_mode="device", track_size=SMALL, densify_size=SMALL, png_depth_scale=PNG_SCALE,
                       max_depth=MAX_DEPTH, arrival_report=True, **KW)
    seq.frame(0)
    for t in range(1, N):
        seq.push_raw(*raw[t], pose=odometry(t))
    digest_sequence("raw", seq, cands)
    torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
