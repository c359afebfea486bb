"""The realtime loop's pieces on the GPU: gsr_densify_frame_capped and gsr_init_frame against the numpy
restatements (tests/online_ref.py) and the torch forms, one workspace under interleaved calls of the three
entries, and SlamSequence fed frame by frame -- push() against run(), given poses against PerFrameSlam, a map born
from the first frame (params=None) and map_every.

log_scales is compared with the tolerance tests/test_gpu_densify.py uses (its docstring: four times
densify_literal's measured distance from the float64 logarithm, 4 x 6.11e-08); everything else is bitwise."""
import numpy as np
import pytest
import torch

import densify_ref as dr
import online_ref as orf
from splatam_amd import densify as dn

pytestmark = pytest.mark.gpu

LOG_SCALES_BOUND = 4 * 6.11e-08
SENTINEL = {"means3D": 7.25, "rgb_colors": -3.5, "unnorm_rotations": 9.0, "logit_opacities": -20.0,
            "log_scales": -10.0}
SIZES = ((5, 7), (64, 32), (37, 61))  # one partial tile; exactly one 2048-pixel tile; two tiles, the last ballot word partial
THRESHOLD_CASES = orf.threshold_cases()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Call:
    """One call's device buffers (tests/test_gpu_densify.py's form): a padded map whose rows hold sentinels, so a
    row the call must not touch is recognised byte for byte.  entry: "densify" (densify_device, which takes the
    capped entry for a threshold other than the default), "raw_capped" (gsr_densify_frame_capped itself) or
    "init"."""

    def __init__(self, case: dict, n_live: int, capacity: int, dev, entry: str = "densify", median_thr=None,
                 median_scale=50.0):
        self.case, self.capacity, self.dev, self.entry = case, capacity, dev, entry
        self.median_thr, self.median_scale = median_thr, median_scale
        self.H, self.W = case["H"], case["W"]
        self.curr = {"im": _t(case["im"], dev), "depth": _t(case["gt"], dev)}
        self.depth_sil, self.w2c = _t(case["depth_sil"], dev), _t(case["w2c"], dev).reshape(4, 4)
        rows = torch.arange(capacity + 1, dtype=torch.float32, device=dev)[:, None]
        self.params = {k: (v + 0.001 * rows).repeat(1, dr.COLS[k]).contiguous() for k, v in SENTINEL.items()}
        self.alive = torch.zeros(capacity + 1, dtype=torch.uint8, device=dev)
        self.alive[:min(n_live, capacity)] = 1
        self.n_live = torch.full((1,), n_live, dtype=torch.int64, device=dev)
        self.overflow = torch.zeros(1, dtype=torch.bool, device=dev)
        self.dest = torch.full((self.H * self.W,), -5, dtype=torch.int32, device=dev)
        self.before = self.snapshot()
        self.n_added = None

    def snapshot(self) -> dict:
        out = {k: v.detach().cpu().numpy().copy() for k, v in self.params.items()}
        out.update(alive=self.alive.cpu().numpy().copy(), n_live=int(self.n_live.item()),
                   overflow=int(self.overflow.item()), dest=self.dest.cpu().numpy().copy())
        return out

    def run(self, ws=None):
        from splatam_amd._lib import lib
        ws = dn.make_workspace(self.H, self.W, self.dev) if ws is None else ws
        c, p = self.case, self.params
        if self.entry == "init":
            self.n_added = dn.init_frame_device(p, self.alive, self.n_live, self.overflow, self.curr, self.w2c,
                                                c["intrinsics"], self.capacity, ws, dest=self.dest)
        elif self.entry == "densify":
            self.n_added = dn.densify_device(p, self.alive, self.n_live, self.overflow, self.curr, self.w2c,
                                             c["intrinsics"], c["sil_thres"], self.capacity, self.depth_sil, ws,
                                             dest=self.dest, median_thr=self.median_thr,
                                             median_scale=self.median_scale)
        else:
            self.n_added = torch.empty(1, dtype=torch.int64, device=self.dev)
            rc = lib.gsr_densify_frame_capped(
                self.H, self.W, self.depth_sil.data_ptr(), self.curr["im"].data_ptr(), self.curr["depth"].data_ptr(),
                *(float(v) for v in c["intrinsics"]), self.w2c.data_ptr(), float(c["sil_thres"]), self.capacity,
                *(p[k].data_ptr() for k in dr.ROW_KEYS), self.alive.data_ptr(), self.n_live.data_ptr(),
                self.overflow.data_ptr(), self.n_added.data_ptr(), self.dest.data_ptr(), ws.data_ptr(),
                torch.cuda.current_stream(self.dev).cuda_stream, int(self.median_thr is not None),
                float(self.median_thr or 0.0), float(self.median_scale))
            assert rc == 0, lib.gsr_last_error()
        return ws


def check(call: Call, ref: dict):
    """Every exact quantity of one call against the restatement, log_scales within LOG_SCALES_BOUND."""
    torch.cuda.synchronize()
    b, a = call.before, call.snapshot()
    exp = dr.expected_call(ref, b["n_live"], call.capacity, b["overflow"])
    assert int(call.n_added.item()) == exp["n_added"]
    assert a["n_live"] == exp["n_live"] and a["overflow"] == exp["overflow"]
    assert np.array_equal(a["dest"], exp["dest"])
    lo, n = b["n_live"], exp["written"]
    alive = b["alive"].copy()
    alive[lo:lo + n] = 1
    assert np.array_equal(a["alive"], alive)
    for k in dr.ROW_KEYS:
        want = b[k].copy()
        if k != "log_scales":
            want[lo:lo + n] = ref["rows"][k][:n]
            assert np.array_equal(dr.bits(a[k]), dr.bits(want)), k
            continue
        keep = np.ones(call.capacity + 1, dtype=bool)
        keep[lo:lo + n] = False
        assert np.array_equal(dr.bits(a[k][keep]), dr.bits(want[keep])), k  # the unwritten rows and the sink row
        dist = dr.rel_distance(a[k][lo:lo + n], ref["rows"][k][:n])
        print(f"  log_scales: device relative distance {dist:.3e} (bound {LOG_SCALES_BOUND:.3e})")
        assert dist <= LOG_SCALES_BOUND


def _counters_zero(ws):
    assert int(ws[:16].abs().sum().item()) == 0  # the arrival counters are back to zero


def _same(a: dict, b: dict):
    for k, v in a.items():
        assert (v.tobytes() == b[k].tobytes()) if isinstance(v, np.ndarray) else (v == b[k]), k


# ------------------------------------------------------------------ gsr_densify_frame_capped

def _size_settings(case):
    med = float(dr.restate(case)["med"])
    assert med > 0
    return (("scale1", None, 1.0), ("capped", med / 2, 3.0), ("equal", med, 3.0), ("uncapped", med * 2, 1.0))


@pytest.mark.parametrize("H,W", SIZES)
def test_capped_against_restatement_sizes(cuda, H, W):
    case = dr.make_case(H, W, "random", seed=4)
    counts = {}
    for name, thr, scale in _size_settings(case):
        ref = orf.restate_capped(case, thr, scale)
        call = Call(case, n_live=37, capacity=37 + H * W + 5, dev=cuda, median_thr=thr, median_scale=scale)
        ws = call.run()
        print(f"{H}x{W} {name}: med {ref['med']!r}, thr {ref['thr']!r}, {ref['count']} selected")
        check(call, ref)
        _counters_zero(ws)
        counts[name] = ref["count"]
    assert counts["scale1"] >= counts["capped"] >= counts["equal"] == counts["uncapped"]
    assert H * W < 100 or counts["scale1"] > counts["uncapped"] > 0


@pytest.mark.parametrize("name,case,median_thr,median_scale", THRESHOLD_CASES, ids=[c[0] for c in THRESHOLD_CASES])
def test_capped_threshold_cases(cuda, name, case, median_thr, median_scale):
    ref = orf.restate_capped(case, median_thr, median_scale)
    for entry in ("densify", "raw_capped"):  # (densify_device sends (None, 50) to gsr_densify_frame: the same bits)
        call = Call(case, n_live=11, capacity=11 + 48 * 64, dev=cuda, entry=entry, median_thr=median_thr,
                    median_scale=median_scale)
        ws = call.run()
        check(call, ref)
        _counters_zero(ws)
    print(f"48x64 {name}: med {ref['med']!r}, thr {ref['thr']!r}, {ref['count']} selected")


@pytest.mark.parametrize("H,W,content", [(37, 61, "random"), (48, 64, "random"), (48, 64, "nan_depth"),
                                         (48, 64, "zeros90"), (64, 32, "quantised")])
def test_capped_with_the_defaults_is_densify_frame(cuda, H, W, content):
    case = dr.make_case(H, W, content, seed=2)
    plain = Call(case, n_live=5, capacity=5 + H * W // 2, dev=cuda)  # (densify_device: gsr_densify_frame)
    capped = Call(case, n_live=5, capacity=5 + H * W // 2, dev=cuda, entry="raw_capped", median_thr=None, median_scale=50.0)
    plain.run(), capped.run()
    torch.cuda.synchronize()
    _same(plain.snapshot(), capped.snapshot())
    assert int(plain.n_added.item()) == int(capped.n_added.item()) == dr.restate(case)["count"]


# ------------------------------------------------------------------ gsr_init_frame

def _init_case(H, W, situation):
    case = dr.make_case(H, W, "all_selected", seed=5)  # (every depth measured)
    gt = case["gt"].reshape(H, W)
    if situation == "checkerboard":
        gt[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = 0.0
    elif situation == "none":
        gt[:] = 0.0
    return case


@pytest.mark.parametrize("situation", ["all_valid", "checkerboard", "none", "overflow"])
@pytest.mark.parametrize("H,W", [(5, 7), (37, 61)])
def test_init_frame(cuda, H, W, situation):
    from splatam_amd.sequence import init_map_literal
    case = _init_case(H, W, situation)
    ref = orf.restate_init(case)
    valid = int((case["gt"] > 0).sum())
    assert ref["count"] == valid == {"all_valid": H * W, "checkerboard": H * W // 2, "none": 0, "overflow": H * W}[situation]
    capacity = valid - 3 if situation == "overflow" else valid + 4
    # (a) a general pose, rows on top of live ones, against the numpy restatement
    lo = 0 if situation == "overflow" else 2
    call = Call(case, n_live=lo, capacity=capacity + lo, dev=cuda, entry="init")
    ws = call.run()
    check(call, ref)
    _counters_zero(ws)
    # (b) an empty map against init_map_literal on the device's own tensors (the contract in elementwise torch
    # ops: the same bits, log_scales aside)
    call = Call(case, n_live=0, capacity=capacity, dev=cuda, entry="init")
    call.run()
    torch.cuda.synchronize()
    lit = init_map_literal(call.curr, call.w2c, case["intrinsics"], 3)
    a, n = call.snapshot(), min(valid, capacity)
    assert lit["means3D"].shape[0] == valid and int(call.n_added.item()) == valid
    assert a["n_live"] == n and a["overflow"] == int(situation == "overflow")
    assert np.array_equal(a["alive"][:n], np.ones(n, np.uint8)) and not a["alive"][n:].any()
    assert a["dest"].max() == n - 1 and int((a["dest"] >= 0).sum()) == n
    for k in dr.ROW_KEYS:
        got, want = a[k][:n], lit[k][:n].cpu().numpy()
        if k == "log_scales":  # (the bound is against the float64 logarithm: the restatement's, pose-independent)
            assert dr.rel_distance(got, ref["rows"][k][:n]) <= LOG_SCALES_BOUND
            assert dr.rel_distance(want, ref["rows"][k][:n]) <= LOG_SCALES_BOUND
        else:
            assert np.array_equal(dr.bits(got), dr.bits(want)), k
        assert np.array_equal(dr.bits(a[k][n:]), dr.bits(call.before[k][n:])), k  # the free rows and the sink row
    if situation == "none":  # nothing written but dest
        assert (a["dest"] == -1).all()
        _same({k: v for k, v in call.before.items() if k != "dest"}, {k: v for k, v in a.items() if k != "dest"})


# ------------------------------------------------------------------ one workspace, three entries

def test_one_workspace_across_the_three_entries(cuda):
    """init, densify and capped calls of different sizes interleaved on one stream in one workspace (sized for the
    largest): each leaves what it leaves in a fresh workspace, and the arrival counters end at zero."""
    cases = {s: dr.make_case(*s, "random", seed=6) for s in ((5, 7), (37, 61), (48, 64), (64, 32))}
    med = float(dr.restate(cases[(48, 64)])["med"])
    order = [("init", (37, 61), None, 50.0), ("densify", (5, 7), None, 50.0), ("densify", (48, 64), med / 2, 3.0),
             ("init", (5, 7), None, 50.0), ("densify", (37, 61), None, 1.0), ("densify", (64, 32), None, 50.0),
             ("init", (48, 64), None, 50.0), ("densify", (5, 7), 0.0, 2.0), ("densify", (48, 64), None, 50.0)]
    shared = dn.make_workspace(64, 64, cuda)

    def calls():
        return [Call(cases[s], n_live=3, capacity=3 + s[0] * s[1], dev=cuda, entry=e, median_thr=thr, median_scale=sc)
                for e, s, thr, sc in order]
    fresh, reused = calls(), calls()
    for c in fresh:
        _counters_zero(c.run())
    for c in reused:  # back to back on the stream, no synchronisation in between
        c.run(shared)
    torch.cuda.synchronize()
    _counters_zero(shared)
    for (e, s, thr, sc), f, r in zip(order, fresh, reused):
        _same(f.snapshot(), r.snapshot())
        assert int(f.n_added.item()) == int(r.n_added.item())
        ref = orf.restate_init(cases[s]) if e == "init" else orf.restate_capped(cases[s], thr, sc)
        check(r, ref)


# ------------------------------------------------------------------ the sequence, frame by frame

N_FRAMES = 4
ITERS = dict(tracking_iters=10, track_replay=10, mapping_iters=10)
POLICIES = {"window": dict(keyframe_policy="window", keyframe_every=2, window=3),
            "overlap": dict(keyframe_policy="overlap", keyframe_every=2, window=3, overlap_pixels=200)}


@pytest.fixture(scope="module")
def capture(cuda):
    from splatam_amd.scenes import make_scene
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    scene = make_scene(20_000, 320, 240, seed=7)  # (tests/test_gpu_sequence.py's size)
    cap = sequence_workload(scene, N_FRAMES, torch.device(cuda))
    params, frames, cam, w2c, _, _ = cap
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
    return cap, 4 * n + 400_000


def _sequence(capture, frames, **kw):
    from splatam_amd.sequence import SlamSequence
    (params, _, cam, w2c, intr, _), bin_cap = capture
    kw = dict(dict(ITERS, prune=False, seed=0), **kw)
    capacity = kw.pop("capacity", params["means3D"].shape[0] + 2 * 320 * 240)
    return SlamSequence(kw.pop("params", params), frames, cam, w2c, intr, capacity=capacity, bin_capacity=bin_cap, **kw)


def _given_poses(capture):
    """The workload's true poses relative to frame 0, as [4,4] device matrices."""
    from splatam_amd.keyframes import pose_w2c
    (_, _, _, _, _, (q_gt, t_gt)), _ = capture
    gt = {"cam_unnorm_rots": q_gt, "cam_trans": t_gt}
    return [pose_w2c(gt, t).reshape(4, 4).contiguous() for t in range(N_FRAMES)]


@pytest.mark.parametrize("policy", ["window", "overlap"])
def test_push_equals_run(cuda, capture, policy):
    from splatam_amd.mapper import GAUSS_KEYS
    (_, frames, _, _, _, _), _ = capture
    whole = _sequence(capture, frames, **POLICIES[policy])
    whole.run()
    whole.check()
    fed = _sequence(capture, frames[:1], num_frames=N_FRAMES, **POLICIES[policy])
    fed.frame(0)
    assert [fed.push(f["im"], f["depth"]) for f in frames[1:]] == [1, 2, 3]
    fed.check()
    with pytest.raises(ValueError):
        fed.push(frames[0]["im"], frames[0]["depth"])  # beyond num_frames
    torch.cuda.synchronize()
    assert len(fed.frames) == N_FRAMES and fed.tracking_iters_run == whole.tracking_iters_run == [0, 10, 10, 10]
    assert torch.equal(fed.params["cam_unnorm_rots"], whole.params["cam_unnorm_rots"])
    assert torch.equal(fed.params["cam_trans"], whole.params["cam_trans"])
    assert torch.equal(fed.alive, whole.alive) and torch.equal(fed.n_live, whole.n_live)
    a, b = fed.live_params(), whole.live_params()
    for k in GAUSS_KEYS + ("rgb_colors",):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(fed.draws, whole.draws):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    if policy == "overlap":
        assert fed.bank.n == whole.bank.n and torch.equal(fed.bank.time[:fed.bank.n], whole.bank.time[:whole.bank.n])
    added = int(fed.n_live.item()) - capture[0][0]["means3D"].shape[0]
    print(f"{policy}: appended {added} rows over {N_FRAMES} frames")
    assert added > 1000


def test_given_poses(cuda, capture):
    from splatam_amd.mapper import GAUSS_KEYS
    from splatam_amd.sequence import PerFrameSlam
    from splatam_amd.slam import matrix_to_quaternion
    (params, frames, cam, w2c, intr, _), bin_cap = capture
    poses = _given_poses(capture)
    seq = _sequence(capture, frames[:1], num_frames=N_FRAMES, **POLICIES["window"])
    seq.frame(0)
    for t in range(1, N_FRAMES):
        assert seq.push(frames[t]["im"], frames[t]["depth"], w2c=poses[t]) == t
    seq.check()
    assert seq.tracking_iters_run == [0] * N_FRAMES
    for t in range(1, N_FRAMES):
        assert torch.equal(seq.params["cam_unnorm_rots"][0, :, t], matrix_to_quaternion(poses[t][:3, :3]))
        assert torch.equal(seq.params["cam_trans"][0, :, t], poses[t][:3, 3])
    ref = PerFrameSlam(params, frames, cam, w2c, intr, bin_capacity=bin_cap, prune=False, **ITERS, **POLICIES["window"])
    for t in range(N_FRAMES):
        ref.frame(t, seq.draws[t], w2c=poses[t])
    torch.cuda.synchronize()
    assert ref.tracking_iters_run == [0] * N_FRAMES
    live = seq.live_params()
    assert live["means3D"].shape[0] == ref.p["means3D"].shape[0] > params["means3D"].shape[0] + 1000
    dq = float((seq.params["cam_unnorm_rots"] - ref.p["cam_unnorm_rots"]).abs().max())
    dt = float((seq.params["cam_trans"] - ref.p["cam_trans"]).abs().max())
    errs = {k: float((live[k] - ref.p[k]).abs().max()) for k in GAUSS_KEYS + ("rgb_colors",)}
    print(f"given poses: pose max |d| q {dq:.3e} t {dt:.3e}; map {errs}")
    assert dq == 0.0 and dt == 0.0 and all(e == 0.0 for e in errs.values())


def test_map_born_from_the_first_frame(cuda, capture):
    from splatam_amd.sequence import init_map_literal
    (_, frames, _, w2c, intr, _), _ = capture
    seq = _sequence(capture, frames[:1], params=None, num_frames=N_FRAMES, capacity=4 * 320 * 240,
                    densify_mode="device", **POLICIES["window"])
    torch.cuda.synchronize()
    lit = init_map_literal(frames[0], w2c, intr, N_FRAMES)
    n = int(seq.n_live.item())
    assert n == lit["means3D"].shape[0] == int((frames[0]["depth"] > 0).sum()) > 320 * 240 // 2
    assert int(seq.alive.sum()) == n and bool(seq.alive[:n].all())
    f0 = {k: v.cpu().numpy() for k, v in frames[0].items()}
    case = {"H": 240, "W": 320, "im": f0["im"], "gt": f0["depth"], "w2c": w2c.cpu().numpy().reshape(16).astype(np.float32),
            "intrinsics": intr, "sil_thres": 0.5}
    ref = orf.restate_init(case)
    live = seq.live_params()
    for k in dr.ROW_KEYS:
        if k == "log_scales":  # (against the float64 logarithm, as everywhere)
            assert dr.rel_distance(live[k].cpu().numpy(), ref["rows"][k]) <= LOG_SCALES_BOUND
        else:
            assert torch.equal(live[k], lit[k]), k
    for k in ("cam_unnorm_rots", "cam_trans"):
        assert torch.equal(seq.params[k], lit[k]) and seq.params[k].shape[-1] == N_FRAMES
    seq.frame(0)
    for f in frames[1:3]:
        seq.push(f["im"], f["depth"])
    seq.check()  # three frames: no binning or map capacity overflowed
    te = float((seq.params["cam_trans"][..., 1:3] - capture[0][5][1][..., 1:3]).abs().max())
    print(f"params=None: {n} Gaussians from frame 0, {int(seq.n_live.item())} after 3 frames, translation error {te:.4f} m")


def test_map_every(cuda, capture):
    (params, frames, _, _, _, _), _ = capture
    seq = _sequence(capture, frames[:1], num_frames=N_FRAMES, map_every=2, **POLICIES["window"])
    counts = [int(seq.n_live.item())]
    seq.frame(0)
    counts.append(int(seq.n_live.item()))
    for f in frames[1:]:
        seq.push(f["im"], f["depth"])
        counts.append(int(seq.n_live.item()))
    seq.check()
    print(f"map_every=2: n_live {counts}; draws {[None if d is None else len(d) for d in seq.draws]}")
    assert counts[3] == counts[2]  # frame 2 does not map: (2 + 1) % 2
    assert counts[2] > counts[1] and counts[4] > counts[3]  # frames 1 and 3 densify
    assert [d is None for d in seq.draws] == [False, False, True, False]
    assert seq.tracking_iters_run == [0, 10, 10, 10]  # every frame is tracked
    assert [kf["id"] for kf in seq.keyframes] == [0, 1, 3]  # the keyframe bookkeeping runs on every frame
