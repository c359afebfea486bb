"""What the realtime loop's entries cost (include/gsr_glue.h: gsr_densify_frame_capped, gsr_init_frame) and what
feeding a sequence frame by frame costs against handing it over whole.

Kernels, at 640x480 on a seeded synthetic depth / silhouette image (about one pixel in eight selected): the device
time per call (device events around `--calls` back-to-back calls, each preceded by the n_live reset that keeps
every call on the same work; `reset` is that reset alone) of

  parent     gsr_densify_frame of the parent revision's library (--parent-lib; built with
             `python -m splatam_amd.build --from-rev REV parent` where git is at hand)
  this       gsr_densify_frame of this tree's library
  this_again the same call again, as a second series: the A/A distance is the spread a difference must exceed
  capped     gsr_densify_frame_capped with median_thr / median_scale set
  init       gsr_init_frame

The series alternate within each of `--rounds` rounds (round 0 is the warm-up); the median round and the range
are reported.  Sequence: bench.py's sequence workload at config 3, frames 0 and 1 untimed, the next `--frames`
frames through frame() on a SlamSequence given every frame (`run`) and through push() on one given two frames
and num_frames (`push`), alternately, a fresh sequence per round (host clock around work that ends in a device
synchronise).  Needs a GPU (no fallback).
Usage: python tools/online_timing.py [--parent-lib FILE] [--calls 200] [--rounds 7] [--frames 4] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 480, 640


def synthetic(dev):
    """A depth / silhouette render and a frame: 5 % of the depths missing, rendered depth within a few cm of the
    measured one but for 2 % far behind it, 10 % of the silhouette below the threshold."""
    rng = np.random.RandomState(5)
    N = H * W
    gt = rng.uniform(0.5, 6.0, N).astype(np.float32)
    gt[rng.uniform(size=N) < 0.05] = 0.0
    rd = (gt + rng.standard_normal(N).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    rd[rng.uniform(size=N) < 0.02] += np.float32(3.0)
    sil = np.where(rng.uniform(size=N) < 0.1, rng.uniform(0.0, 0.5, N), rng.uniform(0.6, 1.0, N)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {"depth_sil": t(np.stack((rd, sil, rd * rd)).reshape(3, H, W)), "gt": t(gt.reshape(1, H, W)),
            "im": t(rng.uniform(size=(3, H, W)).astype(np.float32)), "w2c": torch.eye(4, device=dev)}


def kernel_times(a, dev) -> dict:
    from splatam_amd import _lib
    from splatam_amd import densify as dn
    from splatam_amd.sequence import pad_map
    s = synthetic(dev)
    cap = H * W
    empty = {k: torch.zeros(0, c, device=dev) for k, c in zip(dn.ROW_KEYS, (3, 3, 4, 1, 1))}
    p, alive, n_live = pad_map(empty, cap)
    overflow = torch.zeros(1, dtype=torch.bool, device=dev)
    n_added = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = dn.make_workspace(H, W, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cam = (600.0, 600.0, 319.5, 239.5)
    tail = (cap, *(p[k].data_ptr() for k in dn.ROW_KEYS), alive.data_ptr(), n_live.data_ptr(), overflow.data_ptr(),
            n_added.data_ptr(), None, ws.data_ptr(), stream)
    head = (H, W, s["depth_sil"].data_ptr(), s["im"].data_ptr(), s["gt"].data_ptr(), *cam, s["w2c"].data_ptr(), 0.5)
    lib = _lib.lib
    series = {"reset": lambda: None,
              "this": lambda: lib.gsr_densify_frame(*head, *tail),
              "this_again": lambda: lib.gsr_densify_frame(*head, *tail),
              "capped": lambda: lib.gsr_densify_frame_capped(*head, *tail, 1, 0.01, 20.0),
              "init": lambda: lib.gsr_init_frame(H, W, s["im"].data_ptr(), s["gt"].data_ptr(), *cam,
                                                 s["w2c"].data_ptr(), *tail)}
    if a.parent_lib and os.path.exists(a.parent_lib):
        parent = ctypes.CDLL(a.parent_lib)
        parent.gsr_densify_frame.restype, parent.gsr_densify_frame.argtypes = _lib.SIGNATURES["gsr_densify_frame"]
        series = {"parent": lambda: parent.gsr_densify_frame(*head, *tail), **series}
    added, times = {}, {k: [] for k in series}
    for r in range(a.rounds + 1):  # round 0: warm-up (code objects, first launches), not reported
        for name, call in series.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                n_live.zero_()
                rc = call()
                assert not rc, lib.gsr_last_error()
            e1.record()
            e1.synchronize()
            if r > 0:
                times[name].append(1e3 * e0.elapsed_time(e1) / a.calls)
            added[name] = int(n_added.item())
    assert not bool(overflow.item())
    out = {name: {"us_per_call": round(statistics.median(ts), 3), "us_min": round(min(ts), 3),
                  "us_max": round(max(ts), 3), "n_added": added[name]} for name, ts in times.items()}
    reset = out["reset"]["us_per_call"]
    for name, o in out.items():
        if name != "reset":
            o["us_per_call_less_reset"] = round(o["us_per_call"] - reset, 3)
    out["a_a_distance_us"] = round(abs(out["this"]["us_per_call"] - out["this_again"]["us_per_call"]), 3)
    return out


def sequence_times(a, dev) -> dict:
    from splatam_amd.scenes import config_scene
    from splatam_amd.sequence import SlamSequence
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    K, W0 = max(1, a.frames), 2
    scene = config_scene(a.config)
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, K + W0, dev, prunable=0.02)
    P0 = params["means3D"].shape[0]
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    kw = dict(capacity=P0 + scene.cam.W * scene.cam.H // 3, bin_capacity=2 * n + 2_000_000, seed=0)
    times, live = {"run": [], "push": []}, {}
    for r in range(a.seq_rounds + 1):  # round 0: warm-up, not reported
        for form in times:
            given = frames if form == "run" else list(frames[:W0])
            seq = SlamSequence(params, given, cam, w2c, intr, num_frames=K + W0, **kw)
            for t in range(W0):
                seq.frame(t)
            seq.check()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(W0, W0 + K):
                if form == "run":
                    seq.frame(t)
                else:
                    seq.push(frames[t]["im"], frames[t]["depth"])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            seq.check()
            if r > 0:
                times[form].append(dt / K)
            live[form] = int(seq.n_live.item())
            del seq
    assert live["run"] == live["push"]
    out = {"workload": f"config {a.config} sequence leg ({scene.P} Gaussians, {scene.cam.W}x{scene.cam.H}): 40 tracking "
                       "+ densification + 60 mapping iterations per frame", "frames_per_round": K, "rounds": a.seq_rounds}
    for form, ts in times.items():
        med = statistics.median(ts)
        out[form] = {"frames_per_s": round(1.0 / med, 3), "ms_per_frame": round(1e3 * med, 3),
                     "ms_per_frame_min": round(1e3 * min(ts), 3), "ms_per_frame_max": round(1e3 * max(ts), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "splatam_amd", "_diag", "libgsr_parent.so"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=4, help="timed frames per round (after frames 0 and 1)")
    ap.add_argument("--seq-rounds", type=int, default=3)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_timing needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    out = {"image": f"{W}x{H}", "calls_per_round": a.calls, "rounds": a.rounds, "kernels": kernel_times(a, dev),
           "sequence": sequence_times(a, dev)}
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
