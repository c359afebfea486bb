#!/usr/bin/env python3
"""The raw-frame intake, timed: bench.py's sequence configuration (config 3's scene: 300 k Gaussians, 640x480, 40
tracking + densification + 60 mapping iterations per frame) with track_size and densify_size (320x240), fed frame
by frame as a sensor delivers them (uint8 colour, uint16 depth in mm) -- through SlamSequence.push_raw (one
gsr_ingest_frame launch per frame) and through the literal torch chain of the reference's intake
(scripts/ros_handler.py:402-411, 434-435, on the device) followed by push(), which adds one gsr_resize_frame
launch -- as sequence ms per frame, with an A/A repeat of the push_raw leg as the noise figure; and the intake
alone, per call over --calls back-to-back calls between two events, with the kernel launches of one call of
either form counted by torch.profiler (null when the profiler gives no device events).  [min, median, max] over
--reps repetitions.  Every measurement is a child process under its own time limit (a hung step ends the run).
Prints one JSON line and writes it to profiles/ingest_timing.json.

    python tools/ingest_timing.py [--frames 4] [--reps 3] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("raw", "raw_again", "chain", "intake")
OUT = os.path.join(ROOT, "profiles", "ingest_timing.json")
PNG_SCALE, MAX_DEPTH, SMALL = 1000.0, 9.5, (240, 320)


def _stats(v, nd=4):
    v = sorted(v)
    return [round(v[0], nd), round(v[len(v) // 2], nd), round(v[-1], nd)]


def quantise(frame):
    """A float frame as the sensor's uint8 [H,W,3] and uint16 [H,W] (1 / PNG_SCALE m)."""
    import torch
    rgb = (frame["im"].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    d = (frame["depth"][0].clamp(0, 30) * PNG_SCALE).round().to(torch.int32)
    return rgb, (d & 0xFFFF).to(torch.int16).contiguous().view(torch.uint16)


def torch_chain(rgb, d16):
    """The reference's intake op by op, on the device: the float frame push() takes."""
    import torch
    color = rgb.float()
    try:
        wide = d16.to(torch.float64)
    except (RuntimeError, NotImplementedError):  # (a torch without uint16 device conversions: two more launches)
        wide = (d16.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float64)
    depth = (wide / PNG_SCALE).float()
    depth[depth >= MAX_DEPTH] = -1
    return (color.permute(2, 0, 1) / 255).contiguous(), depth[None]


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
    raw = [quantise(f) for f in frames]
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = params["means3D"].shape[0] + W * H // 3, 2 * n + 2_000_000
    chain = args.step == "chain"
    ms = []
    for _ in range(args.reps):
        first = dict(zip(("im", "depth"), torch_chain(*raw[0]))) if chain else {"rgb_u8": raw[0][0], "depth_u16": raw[0][1]}
        seq = sq.SlamSequence(params, [first], cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                              densify_mode="device", num_frames=K + W0, track_size=SMALL, densify_size=SMALL,
                              png_depth_scale=PNG_SCALE, max_depth=MAX_DEPTH)

        def feed(t):
            if chain:
                seq.push(*torch_chain(*raw[t]))
            else:
                seq.push_raw(*raw[t])
        seq.frame(0)
        for t in range(1, W0):
            feed(t)
        seq.check()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(W0, W0 + K):
            feed(t)
        torch.cuda.synchronize()
        ms.append(1000.0 * (time.perf_counter() - t0) / K)
        seq.check()
    print(json.dumps({f"{args.step}_ms_per_frame": _stats(ms), f"{args.step}_live": int(seq.n_live.item())}))


def _launches(fn):
    """Device kernels of one call of fn, by torch.profiler; None when it records no device events."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception:  # (a profiler without device tracing: the count is left out, the timings stand)
        return None


def intake_step(args):
    import torch

    from splatam_amd import ingest as ig
    from splatam_amd import resize as rz
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).to(dev)
    d16 = torch.randint(0, 12000, (480, 640), generator=g, dtype=torch.int32).to(torch.int16).to(dev).view(torch.uint16)
    a, b = SMALL, (120, 160)
    out = [rz.empty_frame(s, dev) for s in ((480, 640), a, b)]

    def device_form():
        ig.ingest_device(rgb, d16, PNG_SCALE, MAX_DEPTH, a, b, out=out)

    def torch_form():
        im, depth = torch_chain(rgb, d16)
        rz.resize_device({"im": im, "depth": depth}, a, b, out=out[1:])
    res = {}
    for name, fn in (("ingest_device", device_form), ("torch_chain", torch_form)):
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
        res[f"{name}_us"] = _stats(us, 2)
        res[f"{name}_launches"] = _launches(fn)
    res["intake_calls"] = args.calls
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="timed frames (after frames 0 and 1)")
    ap.add_argument("--map-prunable", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back intake calls per timed repetition")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one measurement in this process")
    args = ap.parse_args()
    if args.step:
        return intake_step(args) if args.step == "intake" else sequence_step(args)
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
    raw, chain = out["raw_ms_per_frame"][1], out["chain_ms_per_frame"][1]
    out["chain_over_raw"] = round(chain / raw, 4)
    out["raw_again_over_raw"] = round(out["raw_again_ms_per_frame"][1] / raw, 4)  # the A/A noise figure
    out["intake_speedup"] = round(out["torch_chain_us"][1] / out["ingest_device_us"][1], 3)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
