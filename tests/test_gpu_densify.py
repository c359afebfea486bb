"""gsr_densify_frame (splatam_amd.densify.densify_device) on the GPU against the numpy restatement of its
contract (tests/densify_ref.py) on seeded synthetic depth / silhouette images (no render), against today's
torch selection (sequence.non_presence_mask), under a reused workspace and a graph replay; and the two SLAM
loops with densify_mode="device", at the frame's resolution and at half of it, bitwise against each other.

log_scales is the one quantity compared with a tolerance: four times the largest relative distance of
densify_literal's float32 log_scales (torch.log on the CPU) from the restatement's float64 logarithm over
the same cases (measured: literal 6.11e-08, so the bound is 2.44e-07; the device's largest distance, 1.82e-07,
is in DESIGN.md section 16)."""
import numpy as np
import pytest
import torch

import densify_ref as dr
from splatam_amd import densify as dn

pytestmark = pytest.mark.gpu

CASES = [(H, W, "random") for H, W in dr.SHAPES] + [(1, 1, "all_selected"), (5, 7, "all_selected")] + \
    [(97, 131, c) for c in dr.CONTENTS[1:]] + [(61, 67, "zeros90"), (96, 130, "quantised")]
BIG = (480, 640)
SENTINEL = {"means3D": 7.25, "rgb_colors": -3.5, "unnorm_rotations": 9.0, "logit_opacities": -20.0,
            "log_scales": -10.0}


@pytest.fixture(scope="module")
def refs():
    """Per case: (case, restatement), computed once and left unchanged; and the log_scales bound."""
    table, worst = {}, 0.0
    for H, W, content in CASES + [BIG + ("random",)]:
        case = dr.make_case(H, W, content, seed=1)
        ref = dr.restate(case)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        rows, _, _ = dn.densify_literal({"im": t(case["im"]), "depth": t(case["gt"])}, t(case["w2c"]).reshape(4, 4),
                                        case["intrinsics"], case["sil_thres"], t(case["depth_sil"]))
        worst = max(worst, dr.rel_distance(rows["log_scales"].numpy(), ref["rows"]["log_scales"]))
        table[(H, W, content)] = (case, ref)
    print(f"densify_literal log_scales: largest relative distance {worst:.3e}; device bound {4 * worst:.3e}")
    return table, 4 * worst


class Call:
    """One call's device buffers: a padded map whose rows hold sentinels (every row's own value), so a row
    the call must not touch is recognised byte for byte."""

    def __init__(self, case: dict, n_live: int, capacity: int, overflow: int, dev, dest: bool = True):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.case, self.capacity, self.dev = case, capacity, dev
        self.H, self.W = case["H"], case["W"]
        self.curr = {"im": t(case["im"]), "depth": t(case["gt"])}
        self.depth_sil, self.w2c = t(case["depth_sil"]), t(case["w2c"]).reshape(4, 4)
        rows = torch.arange(capacity + 1, dtype=torch.float32, device=dev)[:, None]
        self.params = {k: (v + 0.001 * rows).repeat(1, dr.COLS[k]).contiguous() for k, v in SENTINEL.items()}
        self.alive = torch.zeros(capacity + 1, dtype=torch.uint8, device=dev)
        self.alive[:min(n_live, capacity)] = 1
        self.n_live = torch.full((1,), n_live, dtype=torch.int64, device=dev)
        self.overflow = torch.full((1,), bool(overflow), dtype=torch.bool, device=dev)
        self.dest = torch.full((self.H * self.W,), -5, dtype=torch.int32, device=dev) if dest else None
        self.before = self.snapshot()
        self.n_added = None

    def snapshot(self) -> dict:
        out = {k: v.detach().cpu().numpy().copy() for k, v in self.params.items()}
        out.update(alive=self.alive.cpu().numpy().copy(), n_live=int(self.n_live.item()),
                   overflow=int(self.overflow.item()), dest=None if self.dest is None else self.dest.cpu().numpy().copy())
        return out

    def run(self, ws=None):
        ws = dn.make_workspace(self.H, self.W, self.dev) if ws is None else ws
        self.n_added = dn.densify_device(self.params, self.alive, self.n_live, self.overflow, self.curr, self.w2c,
                                         self.case["intrinsics"], self.case["sil_thres"], self.capacity,
                                         self.depth_sil, ws, dest=self.dest)
        return ws


def check(call: Call, ref: dict, bound: float) -> float:
    """Every exact quantity of one call against the restatement; returns the log_scales distance."""
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
    dist = 0.0
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
        print(f"  log_scales: device relative distance {dist:.3e} (bound {bound:.3e})")
        assert dist <= bound
    return dist


def _word_count_zero(ws):
    assert int(ws[:16].abs().sum().item()) == 0  # the arrival counters are back to zero


@pytest.mark.parametrize("H,W,content", CASES)
def test_against_restatement(cuda, refs, H, W, content):
    table, bound = refs
    case, ref = table[(H, W, content)]
    call = Call(case, n_live=37, capacity=37 + H * W + 5, overflow=0, dev=cuda)
    ws = call.run()
    print(f"{H}x{W} {content}: {ref['count']} selected, med {ref['med']!r}")
    check(call, ref, bound)
    _word_count_zero(ws)
    if content in ("random", "quantised", "zeros90", "nan_depth", "nan_sil"):
        assert ref["count"] > 0 or H * W < 100
    if content == "nan_sil":
        assert call.dest[dr.NAN_PIXEL].item() == -1


def test_full_frame_and_todays_mask(cuda, refs):
    """480x640 once: the restatement, and the selected set of today's torch form (torch.median on the GPU)."""
    from splatam_amd.sequence import non_presence_mask
    table, bound = refs
    case, ref = table[BIG + ("random",)]
    call = Call(case, n_live=1000, capacity=1000 + BIG[0] * BIG[1], overflow=0, dev=cuda)
    call.run()
    check(call, ref, bound)
    today = non_presence_mask(call.depth_sil, call.curr["depth"], case["sil_thres"])
    assert torch.equal(today, call.dest >= 0) and int(today.sum()) == ref["count"] > 1000


def test_count_scan_with_two_workgroups_per_thread(cuda, refs):
    """3 x 174763 = 524289 pixels, 257 workgroups of 2048: the last workgroup's scan gives threads 0 .. 127 two
    workgroups each, thread 128 one (the last, a single pixel's) and threads 129 .. 255 none.  No smaller image
    reaches that branch.  (Its restatement stays out of `refs`' table: the log_scales bound is the existing one.)"""
    H, W = 3, 174763
    case = dr.make_case(H, W, "random", seed=1)
    ref = dr.restate(case)
    sel = np.flatnonzero(ref["mask"].reshape(-1))
    assert 0 < ref["count"] == len(sel) < H * W and ((sel // 2048) % 2 == 1).any()  # an odd workgroup's prefix is read
    call = Call(case, n_live=37, capacity=37 + H * W + 5, overflow=0, dev=cuda)
    ws = call.run()
    print(f"{H}x{W} random: {ref['count']} selected, med {ref['med']!r}")
    check(call, ref, refs[1])
    _word_count_zero(ws)


@pytest.mark.parametrize("content", ["random", "quantised", "zeros90", "denormal", "nan_depth", "all_selected"])
def test_selection_equals_todays_mask(cuda, refs, content):
    from splatam_amd.sequence import non_presence_mask
    case, ref = refs[0][(97, 131, content)]
    call = Call(case, n_live=0, capacity=97 * 131, overflow=0, dev=cuda)
    call.run()
    torch.cuda.synchronize()
    today = non_presence_mask(call.depth_sil, call.curr["depth"], case["sil_thres"])
    assert torch.equal(today, call.dest >= 0)
    assert np.array_equal(today.cpu().numpy(), ref["mask"])


@pytest.mark.parametrize("overflow0", [0, 1])
def test_capacity_cuts_the_rows(cuda, refs, overflow0):
    table, bound = refs
    case, ref = table[(97, 131, "random")]
    assert ref["count"] > 300
    call = Call(case, n_live=50, capacity=50 + 300, overflow=overflow0, dev=cuda)  # fewer rows than selected
    call.run()
    check(call, ref, bound)
    assert int(call.n_live.item()) == 350 and bool(call.overflow.item()) and int(call.n_added.item()) == ref["count"]
    assert int((call.dest >= 0).sum()) == 300 and int(call.dest.max()) == 349
    # room for all of it: an overflow flag that was set stays set, a clear one stays clear
    call = Call(case, n_live=50, capacity=50 + ref["count"], overflow=overflow0, dev=cuda, dest=False)
    call.run()
    torch.cuda.synchronize()
    assert int(call.n_live.item()) == 50 + ref["count"] and int(call.overflow.item()) == overflow0
    assert call.alive[:-1].all() and call.alive[-1].item() == 0


def test_determinism_and_shared_workspace(cuda, refs):
    table, bound = refs
    big, big_ref = table[BIG + ("random",)]
    small, small_ref = table[(5, 7, "all_selected")]
    shared = dn.make_workspace(*BIG, cuda)
    runs = []
    for ws in (None, None, shared, shared):  # a fresh workspace twice, then a reused one twice
        call = Call(big, n_live=3, capacity=3 + BIG[0] * BIG[1], overflow=0, dev=cuda)
        used = call.run(ws)
        torch.cuda.synchronize()
        _word_count_zero(used)
        runs.append(call.snapshot())
    for r in runs[1:]:
        for k, v in runs[0].items():
            assert (v.tobytes() == r[k].tobytes()) if isinstance(v, np.ndarray) else (v == r[k]), k
    call = Call(small, n_live=2, capacity=2 + 35, overflow=0, dev=cuda)  # 5x7 after 480x640 in the large workspace
    call.run(shared)
    check(call, small_ref, bound)
    _word_count_zero(shared)


def test_graph_replay_without_host_read(cuda, refs):
    """The call captured on one stream, replayed after depth_sil, the frame, w2c and n_live changed in place:
    equal to a direct call on the new values."""
    table, bound = refs
    ca, _ = table[(97, 131, "random")]
    cb, rb = table[(97, 131, "zeros90")]
    cap = 500 + 97 * 131
    call = Call(ca, n_live=11, capacity=cap, overflow=0, dev=cuda)
    ws = dn.make_workspace(97, 131, cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        call.run(ws)  # (warm-up)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call.run(ws)
    fresh = Call(cb, n_live=123, capacity=cap, overflow=0, dev=cuda)
    for dst, src in ((call.depth_sil, fresh.depth_sil), (call.curr["im"], fresh.curr["im"]),
                     (call.curr["depth"], fresh.curr["depth"]), (call.w2c, fresh.w2c), (call.n_live, fresh.n_live),
                     (call.alive, fresh.alive), *((call.params[k], fresh.params[k]) for k in dr.ROW_KEYS)):
        dst.copy_(src)
    call.dest.fill_(-5)
    call.n_added.fill_(-7777)
    call.case, call.before = cb, fresh.before
    graph.replay()
    torch.cuda.synchronize()
    check(call, rb, bound)
    fresh.run()
    torch.cuda.synchronize()
    assert torch.equal(fresh.dest, call.dest) and torch.equal(fresh.n_live, call.n_live)
    for k in dr.ROW_KEYS:
        assert torch.equal(fresh.params[k], call.params[k]), k
    _word_count_zero(ws)


def test_bad_arguments_touch_nothing(cuda, refs):
    from splatam_amd._lib import lib
    case, _ = refs[0][(5, 7, "all_selected")]
    call = Call(case, n_live=2, capacity=40, overflow=0, dev=cuda)
    ws = dn.make_workspace(5, 7, cuda)
    ws_before = ws.clone()
    p = call.params
    stream = torch.cuda.current_stream(cuda).cuda_stream

    def raw(H, W, workspace):
        return lib.gsr_densify_frame(H, W, call.depth_sil.data_ptr(), call.curr["im"].data_ptr(),
                                     call.curr["depth"].data_ptr(), *(float(v) for v in case["intrinsics"]),
                                     call.w2c.data_ptr(), 0.5, call.capacity, *(p[k].data_ptr() for k in dr.ROW_KEYS),
                                     call.alive.data_ptr(), call.n_live.data_ptr(), call.overflow.data_ptr(),
                                     n_added.data_ptr(), call.dest.data_ptr(), workspace, stream)

    n_added = torch.full((1,), -7777, dtype=torch.int64, device=cuda)
    for H, W, w in ((0, 7, ws.data_ptr()), (5, 0, ws.data_ptr()), (-5, 7, ws.data_ptr()), (5, -7, ws.data_ptr()),
                    (5, 7, None)):
        assert raw(H, W, w) != 0
        assert b"densify_frame" in lib.gsr_last_error()
    torch.cuda.synchronize()
    after = call.snapshot()
    for k, v in call.before.items():
        assert np.array_equal(v, after[k]), k
    assert int(n_added.item()) == -7777 and torch.equal(ws, ws_before)
    with pytest.raises(RuntimeError):
        dn.densify_device(p, call.alive, call.n_live, call.overflow, call.curr, call.w2c, case["intrinsics"], 0.5,
                          call.capacity, call.depth_sil, ws[:8])  # a workspace that is too small


# ------------------------------------------------------------------ the two SLAM loops

N_FRAMES = 3


@pytest.fixture(scope="module")
def capture(cuda):
    from splatam_amd.scenes import make_scene
    from splatam_amd.workloads import sequence_workload
    scene = make_scene(20_000, 320, 240, seed=7)
    cap = sequence_workload(scene, N_FRAMES, torch.device(cuda))
    params, frames, cam, w2c, _, _ = cap
    from splatam_amd.tracker import probe_num_rendered
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
    return cap, 4 * n + 400_000


def _both_loops(capture, prune, **kw):
    """SlamSequence and PerFrameSlam on the capture with the same densification arguments; asserts the poses
    and the live map bitwise equal; returns (sequence, appended rows in all, translation error)."""
    from splatam_amd.mapper import GAUSS_KEYS
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    (params, frames, cam, w2c, intr, (_, t_gt)), bin_cap = capture
    P0 = params["means3D"].shape[0]
    seq = SlamSequence(params, frames, cam, w2c, intr, capacity=P0 + 2 * 320 * 240, bin_capacity=bin_cap, prune=prune,
                       seed=0, **kw)
    counts = [P0]
    for t in range(N_FRAMES):
        seq.frame(t)
        counts.append(int(seq.n_live.item()))
    seq.check()
    ref = PerFrameSlam(params, frames, cam, w2c, intr, prune=prune, bin_capacity=bin_cap, **kw)
    for t in range(N_FRAMES):
        ref.frame(t, seq.draws[t])
    torch.cuda.synchronize()
    live = seq.live_params()
    assert live["means3D"].shape[0] == ref.p["means3D"].shape[0]
    assert torch.equal(seq.params["cam_unnorm_rots"], ref.p["cam_unnorm_rots"])
    assert torch.equal(seq.params["cam_trans"], ref.p["cam_trans"])
    for k in GAUSS_KEYS + ("rgb_colors",):
        assert torch.equal(live[k], ref.p[k]), k
    te = float((seq.params["cam_trans"][..., 1:] - t_gt[..., 1:]).abs().max())
    return seq, [b - a for a, b in zip(counts[1:], counts[2:])], te


@pytest.fixture(scope="module")
def full_resolution_added(capture):
    """The rows the full-resolution device run appends per frame without pruning (shared by the tests below)."""
    _, added, te = _both_loops(capture, False, densify_mode="device")
    return added, te


def test_device_sequence_equals_per_frame_loop(cuda, capture, full_resolution_added):
    added, te = full_resolution_added
    print(f"device densification: appended {added}, translation error {te:.4f} m")
    assert sum(added) > 1000 and te < 1e-2


def test_device_sequence_equals_per_frame_loop_pruning(cuda, capture):
    _, _, te = _both_loops(capture, True, densify_mode="device")
    assert te < 1e-2


def _half(capture, cuda):
    (params, frames, cam, w2c, intr, _), _ = capture
    small, small_intr = dn.downscale_capture(frames, intr, 2)
    return dict(densify_frames=small, densify_cam=dn.downscale_camera(320, 240, intr, 2, cuda),
                densify_intrinsics=small_intr)


@pytest.mark.parametrize("prune", [False, True])
def test_half_resolution_densification(cuda, capture, full_resolution_added, prune):
    seq, added, te = _both_loops(capture, prune, densify_mode="device", **_half(capture, cuda))
    print(f"half-resolution densification (prune={prune}): appended {added} (full resolution {full_resolution_added[0]}), "
          f"translation error {te:.4f} m")
    assert te < 1e-2
    if not prune:  # (pruning compacts the map: n_live then counts the survivors, not the appended rows)
        assert sum(added) > 200
        assert all(a < b for a, b in zip(added, full_resolution_added[0]))


def test_half_resolution_torch_mode(cuda, capture):
    _, added, te = _both_loops(capture, False, densify_mode="torch", **_half(capture, cuda))
    assert sum(added) > 200 and te < 1e-2
