"""What scoring candidate views costs after every frame of a running sequence, two ways.

Workload: bench.py's sequence leg at config 3 (300 k Gaussians, 640x480, the capacity and binning capacity as that
leg sizes them).  After frames 0 and 1 (untimed), every further frame is followed by scoring `--visited` (40)
visited poses and `--candidates` (16) candidate poses, K = 16 poses per graph launch, by

  rebuild   what a caller had to do before the padded scorer: seq.live_params() (a boolean index: a host
            synchronisation and a copy of every row), a FisherScorer, BatchedFisher(mode="sum") and
            BatchedFisher(mode="gains") (each: eager probes, warm-up, graph capture), then fit_visited and
            view_gains through them
  padded    seq.fit_visited(w2cs) and seq.view_gains(w2cs) on the scorer the sequence built once
  padded_again  the same two calls again, as a second series: the A/A distance is the spread a difference must
            exceed

in that order within each of `--rounds` rounds (one frame per round; round 0 is the warm-up and builds the padded
scorer, untimed).  Each series is timed by device events around it and by the host clock around it and a device
synchronise (the rebuild path's cost is largely host work).  The median round and the fastest-slowest range are
reported.

Steady state: `--replays` back-to-back replays of the "gains" graph, K poses each, of the padded scorer and of the
last round's BatchedFisher on the compact map of the same live count, alternately (device events; poses/s), with
an A/A pair of the padded one.  Kernel: gsr_fisher_score on the live count's rows against the three torch launches
it replaces (cat, mul, sum over two [P,4] temporaries), `--calls` calls each, alternately.

Needs a GPU (no fallback).
Usage: python tools/seqscore_timing.py [--rounds 5] [--visited 40] [--candidates 16] [--replays 20] [--out FILE]"""
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

K = 16


def pose(deg: float, t, dev) -> torch.Tensor:
    a = math.radians(deg)
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    w2c[:3, 3] = torch.tensor(t)
    return w2c.to(dev)


def timed(fn):
    """(device ms, wall ms, result) of fn(): device events around it, the host clock around it and a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), out


def summary(ts) -> dict:
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--visited", type=int, default=40)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqscore_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seqscore_timing needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    from splatam_amd.fisher import BatchedFisher, FisherScorer, fisher_score, score_workspace
    from splatam_amd.scenes import config_scene
    from splatam_amd.sequence import SlamSequence
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload

    W0 = 2
    scene = config_scene(a.config)
    n_frames = W0 + a.rounds + 1
    params, frames, cam, w2c, intr, _ = sequence_workload(scene, n_frames, dev, prunable=0.02)
    P0 = params["means3D"].shape[0]
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, **frames[0]}, 0)
    capacity, bin_cap = P0 + scene.cam.W * scene.cam.H // 3, 2 * n + 2_000_000  # (bench.py's sequence leg)
    seq = SlamSequence(params, frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, seed=0)
    # poses around the trajectory (2 cm / 0.3 degrees per frame): the visited ones along it, the candidates off it
    visited = [pose(0.3 * j / 4, [0.02 * j / 4, 0.0, 0.0], dev) for j in range(a.visited)]
    cands = [pose(-3.0 + 0.6 * j, [0.05, 0.01 * (j % 4), -0.02 * (j % 3)], dev) for j in range(a.candidates)]
    for t in range(W0):
        seq.frame(t)
    seq.check()

    state = {}

    def rebuild():
        live = seq.live_params()
        fs = FisherScorer(live, cam)
        probes = [visited[0], visited[-1], cands[0], cands[-1]]
        bsum = BatchedFisher(fs, K, mode="sum", probe_w2cs=probes)
        bg = BatchedFisher(fs, K, mode="gains", probe_w2cs=probes)
        fs.fit_visited(visited, batch=bsum)
        g = fs.view_gains(cands, batch=bg)
        state.update(fs=fs, bg=bg, fell_back=bsum.overflowed() or bg.overflowed())
        return g

    def padded():
        seq.fit_visited(visited)
        return seq.view_gains(cands)

    series = {"rebuild": rebuild, "padded": padded, "padded_again": padded}
    dev_ms, wall_ms = {k: [] for k in series}, {k: [] for k in series}
    frame_ms, agree, live_rows = [], [], []
    for r in range(a.rounds + 1):  # round 0: warm-up (kernels, allocator pools, the padded scorer's one build)
        _, fw, _ = timed(lambda: seq.frame(W0 + r))
        got = {}
        for name, fn in series.items():
            d, w, got[name] = timed(fn)
            if r > 0:
                dev_ms[name].append(d)
                wall_ms[name].append(w)
        if r > 0:
            frame_ms.append(fw)
        live_rows.append(int(seq.n_live.item()))
        ref, mine = got["rebuild"], got["padded"]
        agree.append({"counts_equal": bool(torch.equal(ref[:, 0], mine[:, 0])),
                      "eig_max_relative": float(((ref[:, 1] - mine[:, 1]).abs() / ref[:, 1].abs()).max())})
        assert not state["fell_back"], "the rebuild path's graphs overflowed their probed capacity"
    seq.check()
    assert seq.scorer_captures == 1, seq.scorer_captures
    sc = seq.scorer
    assert not sc.sum.overflowed() and not sc.gains.overflowed()

    # steady state: the gains graphs alone, K poses per replay
    bg, hinv_c, hinv_p = state["bg"], state["fs"].H_train_inv, sc.gains.H_inv
    chunk = cands[:K]

    def replays(graph, hinv):
        def run():
            for _ in range(a.replays):
                graph.gains(chunk, hinv, check=False)
        return run
    steady = {"padded": replays(sc.gains, hinv_p), "compact": replays(bg, hinv_c), "padded_again": replays(sc.gains, hinv_p)}
    rate = {k: [] for k in steady}
    for r in range(a.rounds + 1):
        for name, fn in steady.items():
            d, _, _ = timed(fn)
            if r > 0:
                rate[name].append(len(chunk) * a.replays / (1e-3 * d))

    # the kernel against the three torch launches it replaces
    P = seq.params["means3D"].shape[0]
    dm, dop = torch.rand(P, 3, device=dev), torch.rand(P, 1, device=dev)
    ws, out64 = score_workspace(dev), torch.zeros(1, dtype=torch.float64, device=dev)
    out32 = torch.zeros(1, device=dev)

    def kernel():
        for _ in range(a.calls):
            fisher_score(dm, dop, hinv_p, seq.alive, ws, out64)

    def torch3():
        for _ in range(a.calls):
            out32[0] = (torch.cat([dm, dop.reshape(-1, 1)], dim=1) * hinv_p).sum()
    micro = {"gsr_fisher_score": kernel, "torch_cat_mul_sum": torch3, "gsr_fisher_score_again": kernel}
    us = {k: [] for k in micro}
    for r in range(a.rounds + 1):
        for name, fn in micro.items():
            d, _, _ = timed(fn)
            if r > 0:
                us[name].append(1e3 * d / a.calls)

    med = lambda ts: statistics.median(ts)  # noqa: E731
    out = {
        "workload": f"config {a.config} sequence leg ({scene.P} Gaussians, {scene.cam.W}x{scene.cam.H}), capacity "
                    f"{capacity} rows, binning capacity {bin_cap}; per frame {a.visited} visited + {a.candidates} "
                    f"candidate poses, K = {K} per launch",
        "rounds": a.rounds, "live_rows": live_rows, "rows": P,
        "frame_wall_ms": summary(frame_ms),
        "per_frame_scoring_device_ms": {k: summary(v) for k, v in dev_ms.items()},
        "per_frame_scoring_wall_ms": {k: summary(v) for k, v in wall_ms.items()},
        "a_a_distance_device_ms": round(abs(med(dev_ms["padded"]) - med(dev_ms["padded_again"])), 3),
        "a_a_distance_wall_ms": round(abs(med(wall_ms["padded"]) - med(wall_ms["padded_again"])), 3),
        "rebuild_over_padded_wall": round(med(wall_ms["rebuild"]) / med(wall_ms["padded"]), 2),
        "agreement": agree,
        "scorer_captures": seq.scorer_captures,
        "steady_state_poses_per_s": {k: summary(v) for k, v in rate.items()},
        "steady_state_a_a_distance": round(abs(med(rate["padded"]) - med(rate["padded_again"])), 1),
        "capacity_over_live": round(P / live_rows[-1], 3),
        "score_us_per_call": {k: summary(v) for k, v in us.items()},
    }
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
