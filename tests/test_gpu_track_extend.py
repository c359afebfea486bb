"""use_depth_loss_thres on the device (scripts/splatam.py:745-758): the loss's two weighted terms published by
every tracking forward (the _terms entry points), and GraphTracker / SlamSequence / PerFrameSlam extending a
frame's tracking from the one float they read.

Scenes: tests/test_gpu_slam.py's (5000 Gaussians, 160x120) and the same at 100x75 -- 7 x 5 tiles of 16 x 16
with a ragged last column (100 = 6 * 16 + 4) and last row (75 = 4 * 16 + 11), so the last workgroup's sum
sees partial tiles.  iters_per_graph 4, num_iters 8."""
import math

import pytest
import torch

from splatam_amd import glue
from splatam_amd.scenes import make_scene
from splatam_amd.slam import TrackingConfig, get_loss_tracking
from splatam_amd.tracker import GraphTracker, probe_num_rendered

from test_gpu_slam import _pose_leaves, _setup

pytestmark = pytest.mark.gpu

S, N = 4, 8
SIZES = [(160, 120), (100, 75)]
# the literal's own sums are float32 in another order: the suite's relative tolerance for a float32 result
# against the literal, tests/test_gpu_parity.py:4 ("north star: 1e-4 relative") and :11
RTOL = 1e-4


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def frame(request, cuda):
    W, H = request.param
    params, curr = _setup(cuda, False, make_scene(5000, W, H, seed=3))
    return params, curr


def _literal_terms(params, curr):
    """(im term, depth term, loss) of the eager literal get_loss at the pose of column 1."""
    out = {}
    get_loss_tracking(_pose_leaves(params), curr, 1, TrackingConfig(), fast=False, fused=False, losses_out=out)
    return tuple(float(out[k].detach()) for k in ("im", "depth", "loss"))


def _ulp(x: float) -> float:
    t = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(math.inf)) - t)


FORMS = ["l1_alone", "l1_alone_eager_iteration", "render_epilogue", "render_epilogue_xf", "render_track",
         "render_track_no_images"]


def _forward(form, params, curr, cuda, terms):
    """One forward of `form` at the pose of column 1; returns the loss tensor."""
    cfg = TrackingConfig()
    p = _pose_leaves(params)
    seed = torch.ones((), device=cuda)
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    n, _ = probe_num_rendered(params, curr, 1)
    cap = n + 1000
    prev = glue._XF_FUSED, glue._RENDER_FUSED
    try:
        if form == "l1_alone":  # gsr_track_l1_fwd / _fwd_bwd behind separate renders
            from splatam_amd.slam import _get_loss_tracking_fused
            l0, _, _ = _get_loss_tracking_fused(p, curr, 1, cfg, dual=True, terms=terms)  # gsr_track_l1_fwd_terms
            t0 = terms.clone()
            terms.zero_()
            loss, _, _ = _get_loss_tracking_fused(p, curr, 1, cfg, dual=True, seed=seed, terms=terms)  # _fwd_bwd_terms
            assert torch.equal(l0.detach(), loss.detach()) and torch.equal(t0, terms)
            return loss.detach()
        if form == "l1_alone_eager_iteration":  # tracking_iteration's eager form: gsr_track_l1_fwd_bwd_terms
            loss, _ = glue.tracking_iteration(p, curr, 1, cfg, seed=seed, terms=terms)
            return loss.detach()
        glue._XF_FUSED = form != "render_epilogue"
        glue._RENDER_FUSED = form.startswith("render_track")
        loss, _ = glue.tracking_iteration(p, curr, 1, cfg, capacity=cap, status=status, seed=seed,
                                          images=form != "render_track_no_images", terms=terms)
        assert int(status[0]) <= cap and int(status[1]) == 0
        return loss.detach()
    finally:
        glue._XF_FUSED, glue._RENDER_FUSED = prev


@pytest.mark.parametrize("form", FORMS)
def test_terms_match_the_literal(cuda, frame, form):
    """terms = (w_im * image sum, w_depth * depth sum) of the literal get_loss, in every forward form; their sum
    is the published loss within 1 ulp (not bitwise: the loss is one fused multiply-add of the first product
    onto the rounded second, fma(w_im, s0, w_depth * s1), while terms[0] is the first product rounded), and the
    loss is the bits the same call publishes without terms."""
    params, curr = frame
    im_ref, depth_ref, loss_ref = _literal_terms(params, curr)
    terms = torch.full((2,), float("nan"), device=cuda)
    loss = _forward(form, params, curr, cuda, terms)
    plain = _forward(form, params, curr, cuda, None) if form != "l1_alone" else loss
    t0, t1, l = float(terms[0]), float(terms[1]), float(loss)
    print(f"{form}: terms ({t0!r}, {t1!r}) literal ({im_ref!r}, {depth_ref!r}) rel "
          f"({abs(t0 - im_ref) / im_ref:.2e}, {abs(t1 - depth_ref) / depth_ref:.2e}); loss {l!r}, "
          f"terms sum - loss = {(t0 + t1 - l) / _ulp(l):+.2f} ulp")
    assert im_ref > 0 and depth_ref > 0
    assert abs(t0 - im_ref) <= RTOL * im_ref
    assert abs(t1 - depth_ref) <= RTOL * depth_ref
    assert abs(l - loss_ref) <= RTOL * loss_ref
    s = float(terms[0] + terms[1])  # (the float32 sum)
    assert abs(s - l) <= _ulp(l)
    assert torch.equal(loss, plain)


def _tracker(params, curr, fuse_pose, loss_terms, capacity=None):
    p = _pose_leaves(params)
    return p, GraphTracker(p, curr, 1, iters_per_graph=S, warmup_iters=1, fuse_pose=fuse_pose, loss_terms=loss_terms,
                           capacity=capacity)


def _pose(p):
    return p["cam_unnorm_rots"].detach().clone(), p["cam_trans"].detach().clone()


@pytest.mark.parametrize("fuse_pose", [False, True])
def test_graph_rows_and_bits_unchanged(cuda, frame, fuse_pose):
    """Captured iteration k publishes into terms[k]; with and without loss_terms the frame gives the same pose,
    best candidate and loss, bit for bit."""
    params, curr = frame
    pa, a = _tracker(params, curr, fuse_pose, True)
    pb, b = _tracker(params, curr, fuse_pose, False)
    assert a.terms.shape == (S, 2) and a.terms.dtype == torch.float32 and b.terms is None
    assert a.track_frame(N) == N and b.track_frame(N) == N
    for x, y in zip(_pose(pa), _pose(pb)):
        assert torch.equal(x, y)
    assert torch.equal(a.adam.best, b.adam.best) and torch.equal(a.adam.state, b.adam.state)
    assert torch.equal(a.loss, b.loss)
    t = a.terms.cpu()
    assert bool((t > 0).all()) and len({float(v) for v in t[:, 1]}) == S  # every row written, by its own iteration
    assert abs(float(t[S - 1, 0] + t[S - 1, 1]) - float(a.loss)) <= _ulp(float(a.loss))


@pytest.mark.parametrize("fuse_pose", [False, True])
def test_extension_equals_the_longer_run(cuda, frame, fuse_pose):
    params, curr = frame
    p0, probe = _tracker(params, curr, fuse_pose, True)
    probe.track_frame(N)
    depth = float(probe.terms[S - 1, 1])  # the depth term of the frame's 8th iteration
    pose_n = _pose(p0)
    p1, t1 = _tracker(params, curr, fuse_pose, True)
    assert t1.track_frame(N, depth_loss_thres=2.0 * depth) == N
    assert all(torch.equal(x, y) for x, y in zip(_pose(p1), pose_n))
    # exactly at the term: not below it, so the frame extends (the rule is `<`)
    p2, t2 = _tracker(params, curr, fuse_pose, True)
    assert t2.track_frame(N, depth_loss_thres=depth) == 2 * N
    p3, t3 = _tracker(params, curr, fuse_pose, True)
    assert t3.track_frame(N, depth_loss_thres=0.0) == 2 * N
    p4, t4 = _tracker(params, curr, fuse_pose, False)
    assert t4.track_frame(2 * N) == 2 * N
    for p in (p2, p3):
        assert all(torch.equal(x, y) for x, y in zip(_pose(p), _pose(p4)))
    assert torch.equal(t3.adam.best, t4.adam.best) and torch.equal(t3.adam.state, t4.adam.state)
    assert not all(torch.equal(x, y) for x, y in zip(_pose(p4), pose_n))  # the extension moved the pose
    # the threshold needs the terms
    with pytest.raises(RuntimeError, match="loss_terms=True"):
        t4.track_frame(N, depth_loss_thres=1.0)


def test_overflowed_frame_raises_whatever_its_terms_say(cuda, frame):
    params, curr = frame
    n, _ = probe_num_rendered(params, curr, 1)
    p, tr = _tracker(params, curr, True, True, capacity=n - 1)
    pose0 = _pose(p)
    tr.run()
    torch.cuda.synchronize()
    assert tr.overflowed()
    for thres in (0.0, float("inf")):
        with pytest.raises(RuntimeError, match="capacity"):
            tr.track_frame(N, check=True, depth_loss_thres=thres)
    assert all(torch.equal(x, y) for x, y in zip(_pose(p), pose0))  # every step was skipped on the device


# ------------------------------------------------------------- a sequence --
N_FRAMES = 3


@pytest.fixture(scope="module")
def capture(cuda):
    from splatam_amd.workloads import sequence_workload
    return sequence_workload(make_scene(20_000, 320, 240, seed=7), N_FRAMES, torch.device(cuda))


def test_sequence_extends_like_the_per_frame_loop(cuda, capture):
    """Three frames of tests/test_gpu_sequence.py's capture (8 tracking and 8 mapping iterations each): with a
    threshold between the two tracked frames' depth terms one frame extends and one does not, in SlamSequence
    and in PerFrameSlam alike, and their poses and maps agree bitwise (test_sequence_equals_per_frame_loop's
    standard)."""
    from splatam_amd.mapper import GAUSS_KEYS
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    params, frames, cam, w2c, intr, _ = capture
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
    bin_cap = 4 * n + 400_000
    P0 = params["means3D"].shape[0]
    kw = dict(tracking_iters=N, track_replay=S, mapping_iters=8, prune=False)

    def run(cfg):
        seq = SlamSequence(params, frames, cam, w2c, intr, capacity=P0 + 2 * 320 * 240, bin_capacity=bin_cap, seed=0,
                           track_cfg=cfg, **kw)
        depth = []
        for t in range(N_FRAMES):
            seq.frame(t)
            if t > 0 and seq.tracker.terms is not None:
                depth.append(float(seq.tracker.terms[S - 1, 1]))
        seq.check()
        return seq, depth

    plain, _ = run(TrackingConfig())
    assert plain.tracker.terms is None and plain.tracking_iters_run == [0, N, N]
    # the plain run's depth terms: the option on with a threshold nothing reaches -- the same frames, bit for bit
    first, depth = run(TrackingConfig(use_depth_loss_thres=True, depth_loss_thres=float("inf")))
    assert first.tracking_iters_run == [0, N, N]
    assert torch.equal(first.params["cam_trans"], plain.params["cam_trans"])
    assert torch.equal(first.params["cam_unnorm_rots"], plain.params["cam_unnorm_rots"])
    assert len(depth) == 2 and depth[0] != depth[1]
    thres = 0.5 * (depth[0] + depth[1])
    cfg = TrackingConfig(use_depth_loss_thres=True, depth_loss_thres=thres)
    seq, depth2 = run(cfg)
    print(f"depth terms {depth} -> threshold {thres}; iterations {seq.tracking_iters_run}, terms then {depth2}")
    assert sorted(seq.tracking_iters_run) == [0, N, 2 * N]
    ref = PerFrameSlam(params, frames, cam, w2c, intr, bin_capacity=bin_cap, track_cfg=cfg, **kw)
    for t in range(N_FRAMES):
        ref.frame(t, seq.draws[t])
    torch.cuda.synchronize()
    assert ref.tracking_iters_run == seq.tracking_iters_run
    assert torch.equal(seq.params["cam_unnorm_rots"], ref.p["cam_unnorm_rots"])
    assert torch.equal(seq.params["cam_trans"], ref.p["cam_trans"])
    live = seq.live_params()
    for k in GAUSS_KEYS + ("rgb_colors",):
        assert torch.equal(live[k], ref.p[k]), k
    assert not torch.equal(seq.params["cam_trans"], plain.params["cam_trans"])  # the extension changed a pose


def test_literal_loop_extends(cuda, frame):
    """slam.track_frame_literal runs the reference's while-loop: N iterations below the threshold, 2 N otherwise,
    N with the option off."""
    from splatam_amd.slam import as_parameters, track_frame_literal, tracking_variables
    params, curr = frame
    P = params["means3D"].shape[0]

    def literal(cfg):
        p, n, losses = as_parameters(params), [], []
        track_frame_literal(p, tracking_variables(P, cuda), curr, 1, 2, cfg, iters_out=n, losses_out=losses)
        assert len(losses) == n[0]
        return n[0]

    assert literal(TrackingConfig()) == 2
    assert literal(TrackingConfig(use_depth_loss_thres=True)) == 2          # the default threshold, 1e5
    assert literal(TrackingConfig(use_depth_loss_thres=True, depth_loss_thres=0.0)) == 4
    assert literal(TrackingConfig(use_depth_loss_thres=False, depth_loss_thres=0.0)) == 2
