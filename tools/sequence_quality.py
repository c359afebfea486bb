#!/usr/bin/env python3
"""bench.py's sequence configuration (config 3's scene, 40 tracking + densification + 60 mapping iterations per
frame) under both keyframe policies of splatam_amd.sequence, evaluated the way SplaTAM's eval() ends a run
(splatam_amd.evaluate): per policy one JSON line with the means of PSNR, MS-SSIM, depth RMSE and depth L1 over the
capture's frames, the trajectory's ATE, and the evaluation time per frame of
* the device form -- evaluate_sequence: one dual render and gsr_eval_frame's six launches per frame, one
  synchronisation at the end (wall time, and the GPU time between two events), and
* the literal form -- per frame the reference's two renders, evaluate_literal's torch ops and one read of the
  row (wall time; "literal_on": where its torch ops ran),
each as [min, median, max] over --reps repetitions.

    python tools/sequence_quality.py [--frames 4] [--keyframe-every 5] [--window 8] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spread(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def main():
    import torch

    from splatam_amd import evaluate as ev
    from splatam_amd.rasterizer import GaussianRasterizer
    from splatam_amd.scenes import config_scene
    from splatam_amd.sequence import SlamSequence
    from splatam_amd.slam import transform_to_frame, transformed_params2depthplussilhouette, \
        transformed_params2rendervar
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="frames after frames 0 and 1")
    ap.add_argument("--keyframe-every", type=int, default=5)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--map-prunable", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5, help="repetitions of the evaluation timings")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = max(1, args.frames) + 2
    scene = config_scene(3)
    W, H = scene.cam.W, scene.cam.H
    params, frames, cam, w2c, intr, (q_gt, t_gt) = sequence_workload(scene, N, dev, prunable=args.map_prunable)
    gt_w2c = ev.poses_w2c(q_gt, t_gt)
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = params["means3D"].shape[0] + W * H // 3, 2 * n + 2_000_000
    for policy in ("window", "overlap"):
        seq = SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                           window=args.window, keyframe_every=args.keyframe_every, keyframe_policy=policy)
        for t in range(N):
            seq.frame(t)
        seq.check()
        res = seq.evaluate(gt_w2c=gt_w2c)
        out = {"policy": policy, "frames": N, "width": W, "height": H, "window": args.window,
               "keyframe_every": args.keyframe_every, "live_gaussians": int(seq.n_live.item())}
        for k in ("psnr", "ssim", "rmse", "l1"):
            out["avg_" + k] = round(res["avg_" + k], 6)
        out["ate_rmse"] = round(res["ate_rmse"], 6)
        # ---- the device form's time per frame
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        table = torch.empty(N, 8, device=dev)
        wall, gpu = [], []
        for _ in range(args.reps + 1):  # (the first repetition warms up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            ev.evaluate_sequence(seq.params, frames, cam, w2c, sil_thres=seq.sil_thres, alive=seq.alive,
                                 bin_capacity=bin_cap, status=status, table=table)
            e1.record()
            torch.cuda.synchronize()
            wall.append(1000.0 * (time.perf_counter() - t0) / N)
            gpu.append(e0.elapsed_time(e1) / N)
        out["device_ms_per_frame_wall"], out["device_ms_per_frame_gpu"] = _spread(wall[1:]), _spread(gpu[1:])
        # ---- the literal form on the same frames: the live map, two renders, torch ops, one read per frame
        live = seq.live_params()

        def literal(on):
            rows = []
            for t in range(N):
                with torch.no_grad():
                    tg = transform_to_frame(live, t, False, False)
                    im, _, _ = GaussianRasterizer(cam)(**transformed_params2rendervar(live, tg))
                    ds, _, _ = GaussianRasterizer(cam)(**transformed_params2depthplussilhouette(live, w2c, tg))
                a = [x.to(on) for x in (im, ds, frames[t]["im"], frames[t]["depth"])]
                rows.append(ev.evaluate_literal(*a, seq.sil_thres).cpu())
            return torch.stack(rows)

        on = dev
        try:
            lit = literal(on)
        except RuntimeError:  # (no convolution kernels for the device's torch build: the literal's CPU form)
            on = torch.device("cpu")
            lit = literal(on)
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            literal(on)
            torch.cuda.synchronize()
            wall.append(1000.0 * (time.perf_counter() - t0) / N)
        out["literal_ms_per_frame_wall"], out["literal_on"] = _spread(wall), on.type
        d = (table.cpu() - lit).abs() / lit.abs()
        out["max_rel_diff_device_vs_literal"] = float(torch.nan_to_num(d[:, :4]).max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
