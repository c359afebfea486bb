#!/usr/bin/env python3
"""bench.py's sequence configuration (config 3's scene, 40 tracking + densification + 60 mapping iterations
per frame) under both keyframe policies of splatam_amd.sequence: sequence frames/s for "window" and "overlap",
and the per-frame time of the overlap selection alone -- keyframes.select_device (three launches, no host read;
GPU time between two events) and keyframes.select_literal (torch ops with host synchronisations; wall time)
on the same frames, keyframes and random words.  Prints one JSON line.

    python tools/sequence_policy.py [--frames 4] [--keyframe-every 5] [--window 8]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from splatam_amd import keyframes as kfm
    from splatam_amd.scenes import config_scene
    from splatam_amd.sequence import SlamSequence
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="timed frames (after frames 0 and 1)")
    ap.add_argument("--keyframe-every", type=int, default=5)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--map-prunable", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=20, help="repetitions of the selection-only timings")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K, W0 = max(1, args.frames), 2
    scene = config_scene(3)
    W, H = scene.cam.W, scene.cam.H
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, K + W0, dev, prunable=args.map_prunable)
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = params["means3D"].shape[0] + W * H // 3, 2 * n + 2_000_000
    out = {"frames": K, "width": W, "height": H, "window": args.window, "keyframe_every": args.keyframe_every}
    seqs = {}
    for policy in ("window", "overlap"):
        seq = SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                           window=args.window, keyframe_every=args.keyframe_every, keyframe_policy=policy)
        for t in range(W0):
            seq.frame(t)
        seq.check()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(W0, W0 + K):
            seq.frame(t)
        torch.cuda.synchronize()
        out[f"{policy}_frames_per_s"] = round(K / (time.perf_counter() - t0), 3)
        seq.check()
        seqs[policy] = seq
    # the selection alone, on the overlap sequence's last frame: its bank, pose and words
    seq = seqs["overlap"]
    t, bank, S = W0 + K - 1, seq.bank, seq.overlap_pixels
    n_kf = bank.n - (1 if bank.times and bank.times[-1] == t else 0)  # (the keyframes frame t selected from)
    n_cand = max(n_kf - 1, 0)
    w = kfm.words_tensor(seq.draws[t], dev)
    a = (frames[t]["depth"], intr, kfm.pose_w2c(seq.params, t), bank.est_w2c, n_kf, args.window - 2, w[:S],
         w[S:S + n_cand], w[S + n_cand:], bank.time, t, bank.cur_row)
    ws = kfm.make_workspace(H, S, dev)
    res = kfm.select_device(*a, workspace=ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        kfm.select_device(*a, workspace=ws, out=res)
    e1.record()
    torch.cuda.synchronize()
    out["select_device_ms"] = round(e0.elapsed_time(e1) / args.reps, 4)
    kfm.select_literal(*a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        kfm.select_literal(*a)
    torch.cuda.synchronize()
    out["select_literal_ms"] = round(1000.0 * (time.perf_counter() - t0) / args.reps, 4)
    out["keyframes"], out["n_window"] = n_kf, int(res["n_window"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
