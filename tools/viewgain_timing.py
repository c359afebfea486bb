"""View gains (scripts/ros_handler.py:251-359, send_gains) on the bench map at config 3, K poses per launch:

  literal   the caller that needs no new code: per pose a dual render (rasterize_gaussians_dual, colours and
            [z, 1, z^2]), (sil < 0.5).sum().item(), FisherScorer.hessian and the EIG sum, the gain in Python floats
  gains     BatchedFisher(mode="gains").gains: K poses per HIP-graph launch, the silhouette count taken from the
            scoring forward's own lists (gsr_silhouette_count), one checked call per launch
  scores    BatchedFisher(mode="scores").scores in the same run: gains minus the count kernel

The three are timed alternately, `--rounds` rounds of `--launches` launches each (host clock around work that ends
in a device synchronise); the median round and the spread are reported.  Then, on one pose, the count kernel
(gsr_silhouette_count's zeroing launch and count kernel: `--reps` calls captured into one graph, the replay
between two device events) beside render_fwd's stage clock on the same lists.  The counts of the two callers are compared at the timed size.  Needs a GPU (no fallback).
Usage: python tools/viewgain_timing.py [--k 16] [--rounds 5] [--launches 8] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="kernel-time repetitions on one pose")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("viewgain_timing needs a ROCm GPU")
    from splatam_amd import _C, profiling
    from splatam_amd.fisher import BatchedFisher, FisherScorer, _count_into, camera_points, combine_gains
    from splatam_amd.scenes import config_scene
    from splatam_amd.slam import camera_settings, init_tracking_params
    dev = torch.device("cuda", 0)
    scene = config_scene(a.config)
    params = init_tracking_params(scene, num_frames=1, device=dev)
    cam = camera_settings(scene.cam, dev)
    sc = FisherScorer(params, cam)
    K, npix = a.k, scene.cam.W * scene.cam.H
    e = torch.Tensor([])

    def pose(k):  # bench.py's ring of views: 0.5 deg yaw steps, 1 cm translations
        ang = math.radians(0.5 * (k - K / 2))
        w = torch.eye(4, device=dev)
        w[0, 0], w[0, 2], w[2, 0], w[2, 2] = math.cos(ang), math.sin(ang), -math.sin(ang), math.cos(ang)
        w[:3, 3] = torch.tensor([0.01 * math.sin(k), 0.01 * math.cos(k), 0.0], device=dev)
        return w

    poses = [pose(k) for k in range(K)]
    hinv = sc.fit_visited(poses[:4])

    def literal():
        out = []
        for w2c in poses:
            with torch.no_grad():
                pts = camera_points(sc.params["means3D"], w2c)
                z = pts[:, 2:3]
                r = _C.rasterize_gaussians_dual(
                    cam.bg, pts, sc.colors, torch.cat([z, torch.ones_like(z), z * z], 1), sc.opacities, sc.scales,
                    sc.rotations, cam.scale_modifier, e, cam.viewmatrix, cam.projmatrix, cam.tanfovx, cam.tanfovy,
                    cam.image_height, cam.image_width, e, cam.sh_degree, cam.campos, cam.prefiltered)
                g_sil = float((r[2][1] < 0.5).sum().item()) / npix
            g_eig = float((sc.hessian(w2c) * hinv).sum().double().item())
            out.append((g_sil, g_eig, g_eig + g_sil))
        return out

    bg = BatchedFisher(sc, K, mode="gains", probe_w2cs=poses)
    bs = BatchedFisher(sc, K, mode="scores", probe_w2cs=poses)
    legs = {"literal": literal, "gains": lambda: bg.gains(poses, hinv), "scores": lambda: bs.scores(poses, hinv)}
    ref = literal()  # warm-up of every leg, and the results to compare
    got = bg.gains(poses, hinv).cpu()
    assert got is not None and bs.scores(poses, hinv) is not None, "binning capacity overflow"
    same_counts = [round(g[0] * npix) for g in ref] == bg.counts[:K].tolist()
    eig_rel = max(abs(float(got[i, 1]) - ref[i][1]) / max(abs(ref[i][1]), 1e-30) for i in range(K))
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / (a.launches * K))
    res = {"config": a.config, "K": K, "rounds": a.rounds, "launches": a.launches, "counts_equal": same_counts,
           "counts": bg.counts[:K].tolist(), "eig_max_rel_diff": eig_rel}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"poses_per_s": round(1.0 / med, 1), "ms_per_pose": round(1e3 * med, 4),
                     "min_ms": round(1e3 * min(t), 4), "max_ms": round(1e3 * max(t), 4)}
    res["count_cost_ms_per_pose"] = round(res["gains"]["ms_per_pose"] - res["scores"]["ms_per_pose"], 4)

    # one pose: render_fwd's stage clock and the count kernel on the same lists
    with torch.no_grad():
        pts = camera_points(sc.params["means3D"], poses[0])
        args = (cam.bg, pts, sc.colors, sc.opacities, sc.scales, sc.rotations, cam.scale_modifier, e, cam.viewmatrix,
                cam.projmatrix, cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, e, cam.sh_degree,
                cam.campos, cam.prefiltered)
        _C.set_geom_cache(False)  # every call a full forward
        fw = _C.rasterize_gaussians(*args)
        torch.cuda.synchronize()
        profiling.enable_timing(True)
        for _ in range(a.reps):
            fw = _C.rasterize_gaussians(*args)
        torch.cuda.synchronize()
        stages = profiling.read_timing()
        profiling.enable_timing(False)
        out = torch.zeros(1, dtype=torch.int32, device=dev)
        for thres in (0.5, 0.99):
            # `reps` calls captured into one graph: the replay runs them back to back, without the host's call cost
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                _count_into(cam, pts.shape[0], fw[0], fw[3], fw[4], fw[5], thres, out)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(a.reps):
                    _count_into(cam, pts.shape[0], fw[0], fw[3], fw[4], fw[5], thres, out)
            graph.replay()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            res[f"count_us_thres_{thres}"] = round(1e3 * ev[0].elapsed_time(ev[1]) / a.reps, 2)
            res[f"count_thres_{thres}"] = int(out[0])
    res["render_fwd_us"] = round(stages["render_fwd"]["avg_us"], 2)
    res["num_rendered"] = int(fw[0])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same_counts:
        raise SystemExit("the two callers' counts differ")


if __name__ == "__main__":
    main()
