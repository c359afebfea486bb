"""What use_depth_loss_thres (scripts/splatam.py:745-758) costs a SLAM sequence: bench.py's sequence leg at config 3
(sequence_workload, 40 tracking + densification + 60 mapping iterations per frame, frames 0 and 1 untimed) as

  off      the default: no terms published, frame() reads nothing back
  read     the option on with the threshold at +inf: every tracked frame publishes its terms and reads the one
           float, no frame extends -- the cost of the read (and of the _terms entry points) alone
  extend   the threshold at 0: every tracked frame runs its tracking iterations twice

The three forms are built once each and timed alternately, `--rounds` rounds of `--frames` frames (host clock around
work that ends in a device synchronise); the median round and the spread are reported.  The map is restored
before every round (the same frames on the same map each time).  Needs a GPU (no fallback).
Usage: python tools/track_extend_timing.py [--frames 4] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="timed frames per round (after frames 0 and 1)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_extend_timing needs a ROCm GPU")
    from splatam_amd.scenes import config_scene
    from splatam_amd.sequence import SlamSequence
    from splatam_amd.slam import TrackingConfig
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    dev = torch.device("cuda", 0)
    K, W0 = max(1, a.frames), 2
    scene = config_scene(a.config)
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, K + W0, dev, prunable=0.02)
    P0 = params["means3D"].shape[0]
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = P0 + scene.cam.W * scene.cam.H // 3, 2 * n + 2_000_000
    forms = {"off": TrackingConfig(),
             "read": TrackingConfig(use_depth_loss_thres=True, depth_loss_thres=float("inf")),
             "extend": TrackingConfig(use_depth_loss_thres=True, depth_loss_thres=0.0)}
    times = {k: [] for k in forms}
    iters = {}
    for r in range(a.rounds + 1):  # round 0: warm-up (allocator, first launches), not reported
        for name, cfg in forms.items():
            # a fresh sequence per round and form: the same frames on the same map, the same keyframe draws (seed)
            seq = SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                               track_cfg=cfg)
            for t in range(W0):
                seq.frame(t)
            seq.check()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(W0, W0 + K):
                seq.frame(t)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            seq.check()
            if r > 0:
                times[name].append(dt / K)
            iters[name] = seq.tracking_iters_run[W0:]
            del seq
    out = {"workload": f"config {a.config} sequence leg ({scene.P} Gaussians, {scene.cam.W}x{scene.cam.H}): 40 tracking "
                       "+ densification + 60 mapping iterations per frame",
           "frames_per_round": K, "rounds": a.rounds, "forms": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        out["forms"][name] = {"frames_per_s": round(1.0 / med, 3), "ms_per_frame": round(1e3 * med, 3),
                              "ms_per_frame_min": round(1e3 * min(ts), 3), "ms_per_frame_max": round(1e3 * max(ts), 3),
                              "tracking_iters_run": iters[name]}
    off = out["forms"]["off"]["ms_per_frame"]
    out["read_cost_ms_per_frame"] = round(out["forms"]["read"]["ms_per_frame"] - off, 3)
    out["extend_cost_ms_per_frame"] = round(out["forms"]["extend"]["ms_per_frame"] - off, 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
