#!/usr/bin/env python3
"""A tracking resolution of its own, timed: bench.py's sequence configuration (config 3's scene: 300 k Gaussians,
640x480, 40 tracking + densification + 60 mapping iterations per frame) tracked at 640x480 and at 320x240
(SlamSequence(track_size=(240, 320)): the reference's SplaTAM-S setting) -- sequence frames/s and the share of
the frame spent in track() (between two events around every track() call), with an A/A repeat of the
full-resolution leg as the noise figure; and gsr_resize_frame making 320x240 and 160x120 from 640x480 in one
launch against the four F.interpolate calls it replaces (densify.downscale_capture's two, twice), per call over
--calls back-to-back calls between two events.  [min, median, max] over --reps repetitions.  Every measurement
is a child process under its own time limit (a hung step ends the run).  Prints one JSON line and writes it to
profiles/track_res_timing.json.

    python tools/track_res_timing.py [--frames 4] [--reps 5] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("full", "full_again", "track_half", "resize")
OUT = os.path.join(ROOT, "profiles", "track_res_timing.json")


def _stats(v, nd=4):
    v = sorted(v)
    return [round(v[0], nd), round(v[len(v) // 2], nd), round(v[-1], nd)]


def sequence_step(args):
    import torch

    from splatam_amd import sequence as sq
    from splatam_amd.scenes import config_scene
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    dev = torch.device("cuda:0")
    scene = config_scene(3)
    W, H = scene.cam.W, scene.cam.H
    K, W0 = max(1, args.frames), 2
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, K + W0, dev, prunable=args.map_prunable)
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = params["means3D"].shape[0] + W * H // 3, 2 * n + 2_000_000
    kw = dict(track_size=(H // 2, W // 2)) if args.step == "track_half" else {}
    fps, share, track_ms = [], [], []
    for _ in range(args.reps):
        seq = sq.SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                              densify_mode="device", **kw)
        events, track = [], seq.track

        def timed_track(t):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ran = track(t)
            e1.record()
            events.append((e0, e1))
            return ran
        seq.track = timed_track
        for t in range(W0):
            seq.frame(t)
        seq.check()
        events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(W0, W0 + K):
            seq.frame(t)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        seq.check()
        ms = sum(a.elapsed_time(b) for a, b in events)
        fps.append(K / wall)
        track_ms.append(ms / K)
        share.append(ms / (1000.0 * wall))
    s = args.step
    print(json.dumps({f"{s}_frames_per_s": _stats(fps), f"{s}_track_ms_per_frame": _stats(track_ms),
                      f"{s}_track_share": _stats(share), f"{s}_tracking_size": list(seq.slot_curr["im"].shape[-2:]),
                      f"{s}_live": int(seq.n_live.item())}))


def resize_step(args):
    import torch
    import torch.nn.functional as F

    from splatam_amd import resize as rz
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    frame = {"im": torch.rand(3, 480, 640, generator=g).to(dev), "depth": torch.rand(1, 480, 640, generator=g).to(dev)}
    a, b = (240, 320), (120, 160)
    out = (rz.empty_frame(a, dev), rz.empty_frame(b, dev))

    def device_form():
        rz.resize_device(frame, a, b, out=out)

    def torch_form():
        with torch.no_grad():
            for size in (a, b):
                F.interpolate(frame["im"][None], size=size, mode="bilinear", align_corners=False)
                F.interpolate(frame["depth"][None], size=size, mode="nearest")
    res = {}
    for name, fn in (("resize_device_us", device_form), ("resize_torch_us", torch_form)):
        us = []
        for i in range(args.reps + 2):  # (two warm-up repetitions)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                us.append(1000.0 * e0.elapsed_time(e1) / args.calls)
        res[name] = _stats(us, 2)
    res["resize_calls"] = args.calls
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="timed frames (after frames 0 and 1)")
    ap.add_argument("--map-prunable", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back resize calls per timed repetition")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one measurement in this process")
    args = ap.parse_args()
    if args.step:
        return resize_step(args) if args.step == "resize" else sequence_step(args)
    out = {"frames": args.frames, "reps": args.reps}
    for s in STEPS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", s,
               "--frames", str(args.frames), "--reps", str(args.reps), "--map-prunable", str(args.map_prunable),
               "--calls", str(args.calls)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {s} ended with status {r.returncode}")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    full, half = out["full_frames_per_s"][1], out["track_half_frames_per_s"][1]
    out["speedup_track_half"] = round(half / full, 4)
    out["speedup_full_again"] = round(out["full_again_frames_per_s"][1] / full, 4)  # the A/A noise figure
    out["resize_speedup"] = round(out["resize_torch_us"][1] / out["resize_device_us"][1], 3)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
