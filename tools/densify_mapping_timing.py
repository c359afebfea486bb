"""Mapping with Gaussian-splatting densification: slam.map_frame_fused against slam.map_frame_literal, and the
render backward's M2D1 variant beside the mapping variant.  python tools/densify_mapping_timing.py [--reps 5]

One child process per measurement, each under its own time limit (a child that fails or runs out of time ends
the run).  Scenes: bench.py's mapping scene (config 4, workloads.mapping_workload) and a 3000-Gaussian scene
(320 x 240, isotropic).  The configuration's own densify_dict (start_after = 500, densify_every = 100): the timed
iterations carry the per-iteration cost -- the RGB render's own means2D gradient and the statistics -- and the
surgery itself, plain torch every 100th iteration on either path, does not fire in them.  Iterations / s over
`--iters` iterations after `--warmup`, [min, median, max] over the repetitions; render_bwd from the library's
stage events, averaged over the same iterations.  Writes profiles/densify_mapping_timing.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _workload(scene_name, dev):
    import torch
    from splatam_amd import slam
    from splatam_amd.scenes import config_scene, make_scene
    from splatam_amd.workloads import mapping_workload
    scene = config_scene(4) if scene_name == "bench" else make_scene(3000, 320, 240, seed=5)
    params, cam, kfs = mapping_workload(scene, 4, dev)
    p = slam.as_parameters(params)
    for k in ("cam_unnorm_rots", "cam_trans"):
        p[k].requires_grad_(False)
    variables = slam.tracking_variables(scene.P, dev)
    variables["scene_radius"] = torch.max(kfs[0]["depth"]) / 3.0
    del variables["timestep"]
    cfg = slam.MappingConfig(prune_gaussians=False, use_gaussian_splatting_densification=True)
    return p, variables, kfs, cfg


def child_frame(path, scene_name, warmup, iters):
    import numpy as np
    import torch
    from splatam_amd import slam
    dev = torch.device("cuda:0")
    p, variables, kfs, cfg = _workload(scene_name, dev)
    frame = slam.map_frame_fused if path == "fused" else slam.map_frame_literal
    rng = np.random.RandomState(2)
    opt = frame(p, variables, kfs, warmup, cfg, rng=rng)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frame(p, variables, kfs, iters, cfg, optimizer=opt, rng=rng)
    torch.cuda.synchronize()
    return {"iters_per_s": iters / (time.perf_counter() - t0)}


def child_bwd(variant, scene_name, warmup, iters):
    """render_bwd of the fused iteration's one dual rasterization: 'm2d' with means2D_grad_color1, 'map' without."""
    import torch
    from splatam_amd import profiling, slam
    from splatam_amd.glue import map_transform, mapping_loss
    from splatam_amd.rasterizer import rasterize_gaussians_dual
    dev = torch.device("cuda:0")
    p, _, kfs, cfg = _workload(scene_name, dev)
    key = slam.color_key(p)
    for it in range(warmup + iters):
        if it == warmup:
            torch.cuda.synchronize()
            profiling.enable_timing(True)
        kf = kfs[it % len(kfs)]
        means, rots, dcol, opac, scales, col = map_transform(p, kf["id"], kf["w2c"], key)
        m2 = torch.zeros(means.shape[0], 3, device=dev, requires_grad=True)
        sh, colors = (col, None) if key == "shs" else (None, col)
        im, ds, _, _ = rasterize_gaussians_dual(means, m2, sh, colors, dcol, opac, scales, rots, None, kf["cam"],
                                                grad2_channels=1, means2D_grad_color1=variant == "m2d")
        mapping_loss(im, ds, kf["im"], kf["depth"], cfg.w_im, cfg.w_depth).backward()
        for v in p.values():
            v.grad = None
    torch.cuda.synchronize()
    t = profiling.read_timing()["render_bwd"]
    profiling.enable_timing(False)
    return {"render_bwd_us": t["avg_us"], "launches": t["launches"]}


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *map(str, args)], cwd=ROOT,
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f"child {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(xs):
    return [min(xs), statistics.median(xs), max(xs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_mapping_timing.json"))
    ap.add_argument("--child", nargs=5, metavar=("KIND", "WHAT", "SCENE", "WARMUP", "ITERS"))
    a = ap.parse_args()
    if a.child:
        kind, what, scene, warmup, iters = a.child
        fn = child_frame if kind == "frame" else child_bwd
        print(json.dumps(fn(what, scene, int(warmup), int(iters))))
        return
    out = {"reps": a.reps, "warmup": a.warmup, "iters": a.iters, "scenes": {}}
    for scene in ("3k", "bench"):
        res = {}
        for path in ("fused", "literal"):
            xs = [run_child(("frame", path, scene, a.warmup, a.iters), a.limit)["iters_per_s"] for _ in range(a.reps)]
            res[f"map_frame_{path}_iters_per_s"] = spread(xs)
            print(scene, path, spread(xs), flush=True)
        for variant in ("m2d", "map"):
            xs = [run_child(("bwd", variant, scene, a.warmup, a.iters), a.limit)["render_bwd_us"]
                  for _ in range(a.reps)]
            res[f"render_bwd_{variant}_us"] = spread(xs)
            print(scene, "render_bwd", variant, spread(xs), flush=True)
        out["scenes"][scene] = res
        with open(a.out, "w") as f:  # (after every scene: a later child's failure keeps what was measured)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
