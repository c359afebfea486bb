#!/usr/bin/env python3
"""bench.py's sequence configuration (config 3's scene, 40 tracking + densification + 60 mapping iterations
per frame) under the densification forms of splatam_amd.sequence: sequence frames/s for densify_mode "torch"
and "device", and for "device" at a factor-2 densification resolution; and the per-frame GPU time of the
densification step alone, silhouette render excluded, between two events -- the torch form
(sequence.densify_static's ops after its render) and densify.densify_device on the same render, frame, pose
and map.  [min, median, max] over --reps repetitions.  Every measurement is a child process under its own time
limit (a hung step ends the run).  Prints one JSON line.

    python tools/sequence_densify.py [--frames 4] [--reps 5] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ("torch", "device", "device_half", "step")


def _setup(frames_n, prunable):
    import torch

    from splatam_amd.scenes import config_scene
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    dev = torch.device("cuda:0")
    scene = config_scene(3)
    W, H = scene.cam.W, scene.cam.H
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, frames_n, dev, prunable=prunable)
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    return dev, (W, H), (params, frames, cam, w2c, intr), params["means3D"].shape[0] + W * H // 3, 2 * n + 2_000_000


def _stats(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def step(args):
    """One measurement in this process; prints its JSON."""
    import torch

    from splatam_amd import densify as dn
    from splatam_amd import sequence as sq
    from splatam_amd.keyframes import pose_w2c
    K, W0 = max(1, args.frames), 2
    dev, (W, H), (params, frames, cam, w2c, intr), capacity, bin_cap = _setup(K + W0, args.map_prunable)
    kw = {}
    if args.step == "device_half":
        small, small_intr = dn.downscale_capture(frames, intr, 2)
        kw = dict(densify_frames=small, densify_cam=dn.downscale_camera(W, H, intr, 2, dev),
                  densify_intrinsics=small_intr)
    mode = "torch" if args.step == "torch" else "device"

    def sequence():
        return sq.SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0,
                               densify_mode=mode, **kw)
    if args.step != "step":
        fps = []
        for _ in range(args.reps):
            seq = sequence()
            for t in range(W0):
                seq.frame(t)
            seq.check()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(W0, W0 + K):
                seq.frame(t)
            torch.cuda.synchronize()
            fps.append(K / (time.perf_counter() - t0))
            seq.check()
        print(json.dumps({f"{args.step}_frames_per_s": _stats(fps), "appended": int(seq.n_live.item()) -
                          params["means3D"].shape[0]}))
        return
    # the densification step alone on frame W0 of a sequence that ran frames 0 .. W0 - 1 and tracked frame W0:
    # both forms from the same render, on copies of the same map
    seq = sequence()
    for t in range(W0):
        seq.frame(t)
    t = W0
    seq.track(t)
    kf = seq._kf(t)
    ds = sq.render_depth_sil(seq.params, kf, t, seq.alive, seq.bin_capacity, seq.dstatus).contiguous()
    pose = pose_w2c(seq.params, t)
    state = {k: seq.params[k].detach().clone() for k in dn.ROW_KEYS}
    alive0, n0 = seq.alive.clone(), seq.n_live.clone()
    ws = dn.make_workspace(H, W, dev)

    def reset():
        with torch.no_grad():
            for k, v in state.items():
                seq.params[k].detach().copy_(v)
            seq.alive.copy_(alive0)
            seq.n_live.copy_(n0)

    def torch_form():  # densify_static after its render
        with torch.no_grad():
            mask = sq.non_presence_mask(ds, kf["depth"], seq.sil_thres)
            new = sq.frame_pointcloud(seq.params, kf, t, intr)
            incl = torch.cumsum(mask.to(torch.int64), 0)
            dest = seq.n_live + incl - 1
            ok = mask & (dest < capacity)
            dest = torch.where(ok, dest, torch.full_like(dest, capacity))
            for k, v in new.items():
                seq.params[k].data.index_put_((dest,), v)
            seq.alive.index_put_((dest,), ok.to(torch.uint8))
            total = seq.n_live + incl[-1:]
            seq.overflow.logical_or_(total > capacity)
            seq.n_live.copy_(torch.clamp(total, max=capacity))

    def device_form():
        dn.densify_device(seq.params, seq.alive, seq.n_live, seq.overflow, kf, pose, intr, seq.sil_thres, capacity,
                          ds, ws)
    out = {}
    for name, fn in (("torch_step_ms", torch_form), ("device_step_ms", device_form)):
        ms = []
        for i in range(args.reps + 2):  # (two warm-up repetitions)
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        out[name] = _stats(ms)
        out[name.replace("_step_ms", "_step_added")] = int(seq.n_live.item()) - int(n0.item())
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="timed frames (after frames 0 and 1)")
    ap.add_argument("--map-prunable", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one measurement in this process")
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"frames": args.frames, "reps": args.reps}
    for s in STEPS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", s,
               "--frames", str(args.frames), "--reps", str(args.reps), "--map-prunable", str(args.map_prunable)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {s} ended with status {r.returncode}")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
