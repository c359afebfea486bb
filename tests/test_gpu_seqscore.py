"""View scoring on a running sequence's capacity-padded map, on the GPU: gsr_fisher_score against the numpy
restatement, gsr_forward_static_alive against gsr_forward_static on the compacted rows, fisher.SequenceFisher
against BatchedFisher on the compacted map, and SlamSequence.view_scorer / fit_visited / view_gains across
frames that densify, prune and compact, and across a map moved to a larger buffer.

Tolerances (derived, none measured):
* a float64 sum of n non-negative terms taken in any order is within (n - 1) 2^-53 of the exact sum, relative; the
  kernel adds n = 4 P float32 products, the reference here is the exact sum (math.fsum) of the same products, so
  |kernel - exact| <= 4 P 2^-53 exact.  All-dead masks and P == 0 give exactly 0.0.
* the same argument at float32 for BatchedFisher's torch sum of the same products: 4 P 2^-24, relative.
* everything else is an integer or bitwise: counts, status rows, radii, images, the live rows' Hessians (the tile
  lists sort by (depth, id) and compaction keeps the id order; gsr_backward_power.hip's per-Gaussian sums run in
  a fixed order over the instance records), the dead rows' Hessians (+0).

Dead rows: tests/test_gpu_online.py's sentinels for colour (-3.5) and rotation (9.0) and its mean's depth (7.25),
but moved into view and made opaque (opacity 0.9 / logit 2, scale 0.05 / log -3): a row the mask failed to cull
then gets a radius, instances and a visible splat, where the original invisible sentinels would change nothing.
One case beyond the issue's sizes: P = 65 836 rows, the smallest shape class at which gsr_fisher_score's
bounded grid (256 workgroups) strides -- a path no P <= 5000 takes."""
import math

import numpy as np
import pytest
import torch

from splatam_amd.fisher import (BatchedFisher, FisherScorer, SequenceFisher, fisher_score, score_workspace)
from splatam_amd.scenes import make_scene
from splatam_amd.slam import camera_settings, init_tracking_params
from test_seqscore_cpu import _static_alive, restate_score

pytestmark = pytest.mark.gpu

U64, U32 = 2.0 ** -53, 2.0 ** -24
ROWS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
DEAD = {"means3D": (0.25, -0.25, 7.25), "rgb_colors": -3.5, "unnorm_rotations": 9.0, "logit_opacities": 2.0,
        "log_scales": -3.0}


def _pose(deg, t):
    a = math.radians(deg)
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    w2c[:3, 3] = torch.tensor(t)
    return w2c


def _mask(n_live: int, tail: int, dev) -> torch.Tensor:
    """Every third row dead among the first 3 n_live / 2, then a dead tail: n_live live rows."""
    assert n_live % 2 == 0
    body = 3 * n_live // 2
    alive = torch.zeros(body + tail, dtype=torch.uint8, device=dev)
    alive[:body] = (torch.arange(body, device=dev) % 3 != 2).to(torch.uint8)
    assert int(alive.sum()) == n_live
    return alive


def _scatter(compact: torch.Tensor, alive: torch.Tensor, fill) -> torch.Tensor:
    out = torch.empty((alive.numel(),) + tuple(compact.shape[1:]), dtype=compact.dtype, device=compact.device)
    out[:] = torch.as_tensor(fill, dtype=compact.dtype, device=compact.device)
    out[alive.bool()] = compact
    return out.contiguous()


def _exact(prod: torch.Tensor) -> float:
    return math.fsum(prod.detach().cpu().numpy().astype(np.float64).ravel().tolist())


# ------------------------------------------------------------------ gsr_fisher_score

def _score_inputs(P, seed=11):
    """Non-negative, exact zeros among them: H is a sum of squares, H_inv = 1 / (H_train + 0.1) > 0."""
    rng = np.random.RandomState(seed + P % 1000)
    dm = (rng.rand(P, 3).astype(np.float32) ** 2 * 50.0).astype(np.float32)
    dop = (rng.rand(P, 1).astype(np.float32) ** 2 * 5.0).astype(np.float32)
    dm[rng.rand(P, 3) < 0.2] = 0.0
    dop[rng.rand(P, 1) < 0.2] = 0.0
    hinv = (1.0 / (rng.rand(P, 4).astype(np.float32) * 30.0 + np.float32(0.1))).astype(np.float32)
    return dm, dop, hinv


def _np_mask(kind, P):
    if kind == "null":
        return None
    if kind == "ones":
        return np.ones(P, np.uint8)
    if kind == "zeros":
        return np.zeros(P, np.uint8)
    m = (np.arange(P) % 3 != 2).astype(np.uint8)  # "third": every third row dead, and a dead tail
    m[P - P // 5:] = 0
    return m


def _run_score(dm, dop, hinv, alive, dev, ws=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ws = score_workspace(dev) if ws is None else ws
    out = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    fisher_score(t(dm), t(dop), t(hinv), t(alive), ws, out)
    torch.cuda.synchronize()
    assert int(ws[:128].sum()) == 0  # the arrival counter is back to zero
    return float(out[0]), ws


@pytest.mark.parametrize("kind", ["null", "ones", "zeros", "third"])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 5003, 65_836])
def test_fisher_score_against_restatement(cuda, P, kind):
    """5003: 20 workgroups, the last one partial; 65 836: the 256-workgroup grid strides (257 full rounds of
    workgroup 0, a partial one)."""
    dm, dop, hinv = _score_inputs(P)
    alive = _np_mask(kind, P)
    got, ws = _run_score(dm, dop, hinv, alive, cuda)
    sel = np.ones(P, bool) if alive is None else alive != 0
    H = np.concatenate([dm, dop], 1)
    want = math.fsum((H[sel] * hinv[sel]).astype(np.float32).astype(np.float64).ravel().tolist())
    n_rows = int(sel.sum())
    print(f"P {P} {kind}: kernel {got!r}, exact {want!r}, numpy {restate_score(dm, dop, hinv, alive)!r}, "
          f"relative distance {abs(got - want) / want if want else 0.0:.3e} (bound {4 * n_rows * U64:.3e})")
    if P == 0 or kind == "zeros":
        assert got == 0.0 and not math.copysign(1.0, got) < 0
    else:
        assert want > 0 and abs(got - want) <= 4 * n_rows * U64 * want
        assert abs(restate_score(dm, dop, hinv, alive) - want) <= 4 * n_rows * U64 * want
    again, _ = _run_score(dm, dop, hinv, alive, cuda, ws)  # the same workspace, the same bits
    assert np.float64(again).tobytes() == np.float64(got).tobytes()
    if alive is not None and P:  # a dead row is selected out: NaN in its H and H_inv does not reach the sum
        dead = alive == 0
        dm2, dop2, hinv2 = dm.copy(), dop.copy(), hinv.copy()
        dm2[dead], dop2[dead], hinv2[dead] = np.nan, np.nan, np.nan
        poisoned, _ = _run_score(dm2, dop2, hinv2, alive, cuda, ws)
        assert np.float64(poisoned).tobytes() == np.float64(got).tobytes()


def test_fisher_score_one_workspace_across_sizes(cuda):
    """Calls of different P back to back on one stream in one workspace give what a fresh workspace gives."""
    sizes = (5003, 1, 65_836, 257, 0, 256)
    cases = [(_score_inputs(P), _np_mask("third", P)) for P in sizes]
    fresh = [_run_score(*c, a, cuda)[0] for c, a in cases]
    ws = score_workspace(cuda)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    out = torch.zeros(len(sizes), dtype=torch.float64, device=cuda)
    dev_cases = [tuple(t(x) for x in (*c, a)) for c, a in cases]
    for k, (dm, dop, hinv, alive) in enumerate(dev_cases):
        fisher_score(dm, dop, hinv, alive, ws, out[k:k + 1])
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == np.array(fresh, np.float64).tobytes()
    assert int(ws[:128].sum()) == 0


# ------------------------------------------------------------------ the compact map and its padded form

P_LIVE, W, H, K = 3000, 96, 72, 4


class Maps:
    """One scene as a compact map (FisherScorer, BatchedFisher graphs) and as a padded map under an alive mask
    whose live rows are the compact map's rows in order; the poses, and the references every test shares."""

    def __init__(self, dev):
        scene = make_scene(P_LIVE, W, H, seed=22)  # (tests/test_gpu_viewgain.py's: the counts decide both ways)
        self.compact = init_tracking_params(scene, num_frames=1, device=dev)
        self.cam = camera_settings(scene.cam, dev)
        self.alive = _mask(P_LIVE, 200, dev)
        self.padded = {k: (_scatter(v.detach(), self.alive, DEAD[k]) if k in ROWS else v)
                       for k, v in self.compact.items()}
        self.poses = [_pose(d, [0.01 * d, -0.005 * d, 0.02]).to(dev) for d in (-4.0, 0.0, 3.0, 12.0)]
        self.cands = [_pose(d, [0.02, 0.01 * d, -0.03]).to(dev) for d in (-8.0, 2.0, 6.0)]
        self.fs = FisherScorer(self.compact, self.cam)
        every = self.poses + self.cands
        self.bsum = BatchedFisher(self.fs, K, mode="sum", probe_w2cs=every)
        self.bgains = BatchedFisher(self.fs, K, mode="gains", probe_w2cs=every)
        self.bin_capacity = self.bsum.capacity
        self.H_live = self.bsum.hessian_sum(self.poses).clone()
        assert self.H_live is not None
        self.hinv_live = torch.reciprocal(self.H_live + 0.1)
        g = self.bgains.gains(self.cands, self.hinv_live)
        self.gains_live, self.counts_live = g.clone(), self.bgains.counts[:len(self.cands)].clone()
        self.exact = [_exact(self.fs.hessian(w) * self.hinv_live) for w in self.cands]


@pytest.fixture(scope="module")
def maps(cuda):
    return Maps(cuda)


def _rendervars(fs, rows=None):
    rv = (fs.params["means3D"].detach(), fs.colors.detach(), fs.opacities.detach(), fs.scales.detach(),
          fs.rotations.detach())
    return rv if rows is None else tuple(t[rows].contiguous() for t in rv)


def _static(cam, rv, capacity, alive=None):
    from splatam_amd import _C
    e = torch.Tensor([])
    status = torch.zeros(4, dtype=torch.int32, device=rv[0].device)
    means, colors, opac, scales, rot = rv
    out = _C.rasterize_gaussians(cam.bg, means, colors, opac, scales, rot, cam.scale_modifier, e, cam.viewmatrix,
                                 cam.projmatrix, cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, e,
                                 cam.sh_degree, cam.campos, cam.prefiltered, capacity=capacity, status=status,
                                 alive=alive)
    torch.cuda.synchronize()
    return out, status


def test_forward_static_alive(cuda):
    """3000 Gaussians at 64x48 under a mask that drops every third row and a tail, the dead rows opaque sentinels
    in view, against gsr_forward_static on the compacted rows."""
    scene = make_scene(3000, 64, 48, seed=34)
    fs = FisherScorer(init_tracking_params(scene, num_frames=1, device=cuda), camera_settings(scene.cam, cuda))
    rv = _rendervars(fs)
    alive = _mask(3000, 200, cuda)
    # (rotations are rendervars here: (9, 0, 0, 0) is the identity rotation unnormalised, so the splat stays small)
    fills = (DEAD["means3D"], DEAD["rgb_colors"], 0.9, 0.05, (DEAD["unnorm_rotations"], 0.0, 0.0, 0.0))
    padded = tuple(_scatter(t, alive, f) for t, f in zip(rv, fills))
    cap = 400_000
    ref, st_ref = _static(fs.cam, rv, cap)
    got, st = _static(fs.cam, padded, cap, alive)
    unmasked, st_un = _static(fs.cam, padded, cap, torch.ones_like(alive))
    live = alive.bool()
    print(f"status compact {st_ref.tolist()}, padded {st.tolist()}, padded without culling {st_un.tolist()}")
    assert int(st_ref[0]) > 3000 and int(st_ref[0]) <= cap
    assert torch.equal(got[1], ref[1]) and torch.equal(got[6], ref[6])          # image, depth
    assert torch.equal(got[2][live], ref[2]) and int(got[2][~live].abs().sum()) == 0  # radii
    assert torch.equal(st, st_ref)
    # the dead rows are not inert: unculled they get radii and instances and change the image
    assert int((unmasked[2][~live] > 0).sum()) > 0 and int(st_un[0]) > int(st[0])
    assert not torch.equal(unmasked[1], ref[1])
    # all ones: gsr_forward_static itself
    ones, st_1 = _static(fs.cam, rv, cap, torch.ones(3000, dtype=torch.uint8, device=cuda))
    assert torch.equal(ones[1], ref[1]) and torch.equal(ones[6], ref[6]) and torch.equal(ones[2], ref[2])
    assert torch.equal(st_1, st_ref)
    assert _static_alive(alive=None) == (-1, "alive mask required")  # a NULL mask is refused


# ------------------------------------------------------------------ SequenceFisher against BatchedFisher

def test_padded_hessians_are_the_compact_ones(cuda, maps):
    sf = SequenceFisher(maps.padded, maps.alive, maps.cam, K, "sum", maps.bin_capacity)
    Hp = sf.hessian_sum(maps.poses)
    assert Hp is not None and not sf.overflowed()
    live = maps.alive.bool()
    assert float(maps.H_live.abs().max()) > 0
    assert torch.equal(Hp[live], maps.H_live)
    dead = Hp[~live]
    assert int((dead != 0).sum()) == 0 and not bool(torch.signbit(dead).any())  # exactly +0
    # fewer poses than K: the padded slots weigh 0
    H2 = sf.hessian_sum(maps.poses[:2]).clone()
    assert torch.equal(H2[live], maps.bsum.hessian_sum(maps.poses[:2]))


@pytest.mark.parametrize("mode", ["gains", "scores"])
def test_padded_scores_and_gains(cuda, maps, mode):
    sf = SequenceFisher(maps.padded, maps.alive, maps.cam, K, mode, maps.bin_capacity)
    hinv = _scatter(maps.hinv_live, maps.alive, float("nan"))  # dead rows of H_inv are not read
    n = len(maps.cands)
    if mode == "gains":
        g = sf.gains(maps.cands, hinv)
        assert g.dtype == torch.float64 and g.shape == (n, 3)
        assert torch.equal(sf.counts[:n], maps.counts_live)
        assert len(set(maps.counts_live.tolist())) > 1 and 0 < int(maps.counts_live.min())
        assert torch.equal(g[:, 0], maps.gains_live[:, 0])
        eig = g[:, 1]
        assert torch.equal(g[:, 2], g[:, 0] + g[:, 1])
    else:
        eig = sf.scores(maps.cands, hinv)
        assert eig.dtype == torch.float64 and eig.shape == (n,)
    for k in range(n):
        got, exact, f32 = float(eig[k]), maps.exact[k], float(maps.gains_live[k, 1])
        print(f"{mode} pose {k}: kernel {got!r}, exact {exact!r} (relative {abs(got - exact) / exact:.3e}, bound "
              f"{4 * P_LIVE * U64:.3e}), float32 torch sum {f32!r} (relative {abs(got - f32) / f32:.3e}, bound "
              f"{4 * P_LIVE * U32:.3e})")
        assert exact > 0
        assert abs(got - exact) <= 4 * P_LIVE * U64 * exact
        assert abs(got - f32) <= 4 * P_LIVE * U32 * f32
    assert not sf.overflowed()


def test_isotropic_rule_and_modes(cuda, maps):
    aniso = dict(maps.padded, log_scales=maps.padded["log_scales"].repeat(1, 3).contiguous())
    with pytest.raises(ValueError, match="isotropic"):
        SequenceFisher(aniso, maps.alive, maps.cam, K, "gains", maps.bin_capacity)
    sf = SequenceFisher(maps.padded, maps.alive, maps.cam, 2, "scores", maps.bin_capacity)
    with pytest.raises(RuntimeError, match="built for mode"):
        sf.hessian_sum(maps.poses[:1])
    with pytest.raises(ValueError, match="at most 2"):
        sf.scores(maps.poses[:3], torch.ones_like(sf.H_inv))


def test_binning_capacity_overflow(cuda, maps):
    """tests/test_gpu_viewgain.py's test_batched_gains_capacity_overflow on the padded map: a bin_capacity below
    one pose's instance count gives None from a checked call, overflowed(), and a pose that fits still scores."""
    eye, behind = torch.eye(4, device=cuda), torch.eye(4, device=cuda)
    behind[2, 3] = -100.0  # sees nothing
    _, st = _static(maps.cam, _rendervars(maps.fs), 400_000)
    need = int(st[0])  # the identity pose's instance count
    assert need > 1000
    sf = SequenceFisher(maps.padded, maps.alive, maps.cam, 2, "gains", bin_capacity=need // 2)
    hinv = torch.ones_like(sf.H_inv)
    assert sf.gains([eye], hinv) is None
    torch.cuda.synchronize()
    assert sf.overflowed(1) and int(sf.status[0, 0]) > sf.capacity
    g = sf.gains([behind, behind], hinv)
    assert g is not None and torch.equal(g[:, 0], torch.ones(2, dtype=torch.float64, device=cuda))
    assert float(g[:, 1].abs().max()) == 0.0


# ------------------------------------------------------------------ the sequence

N_FRAMES = 3
SEQ = dict(tracking_iters=10, track_replay=10, mapping_iters=10, keyframe_every=2, window=3, prune=True, seed=0)


def _mark_prunable(seq):
    """Every seventh live row's opacity below the removal threshold: the next mapped frame prunes and compacts."""
    n = int(seq.n_live.item())
    with torch.no_grad():
        seq.params["logit_opacities"].data[torch.arange(0, n, 7, device=seq.alive.device)] = math.log(0.002 / 0.998)
    return len(range(0, n, 7))


class Runs:
    """The same small sequence twice: `a` with a view scorer built after frame 0 and fit_visited(n_monte=2)
    between the frames, `b` without.  Frames 1-2 densify, prune (the rows _mark_prunable marked) and compact."""

    def __init__(self, dev):
        from splatam_amd.sequence import SlamSequence
        from splatam_amd.tracker import probe_num_rendered
        from splatam_amd.workloads import sequence_workload
        scene = make_scene(3000, 64, 48, seed=7)
        params, frames, cam, w2c, intr, _ = sequence_workload(scene, N_FRAMES, dev)
        n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
        self.cam, self.P0 = cam, params["means3D"].shape[0]
        self.cands = [_pose(d, [0.02, 0.01 * d, -0.03]).to(dev) for d in (-8.0, 2.0, 6.0, 10.0, -3.0)]
        self.live_counts = {}
        for name in ("a", "b"):
            seq = SlamSequence(params, frames, cam, w2c, intr, capacity=self.P0 + 2 * 64 * 48,
                               bin_capacity=4 * n + 400_000, **SEQ)
            counts = []
            for t in range(N_FRAMES):
                seq.frame(t)
                if t == 0 and name == "a":
                    seq.view_scorer(K=K, seed=3)
                if name == "a":
                    seq.fit_visited(n_monte=2)
                counts.append(int(seq.n_live.item()))
                if t < N_FRAMES - 1:
                    self.pruned = _mark_prunable(seq)
            seq.check()
            self.live_counts[name] = counts
            setattr(self, name, seq)
        torch.cuda.synchronize()
        self.snap = {name: self._snapshot(getattr(self, name)) for name in ("a", "b")}

    @staticmethod
    def _snapshot(seq):
        out = {k: v.detach().clone() for k, v in seq.live_params().items() if torch.is_tensor(v)}
        out["draws"] = [None if d is None else np.asarray(d).copy() for d in seq.draws]
        return out


@pytest.fixture(scope="module")
def runs(cuda):
    return Runs(cuda)


def _fresh(seq, cam, cands):
    """The rebuild path: a FisherScorer and two BatchedFisher graphs on the live rows and the explicit poses."""
    live = seq.live_params()
    fs = FisherScorer(live, cam)
    poses = seq.visited_w2cs()
    bsum = BatchedFisher(fs, K, mode="sum", probe_w2cs=poses + cands)
    bg = BatchedFisher(fs, K, mode="gains", probe_w2cs=poses + cands)
    hinv = fs.fit_visited(poses, batch=bsum).clone()
    gains = fs.view_gains(cands, batch=bg).clone()
    exact = [_exact(fs.hessian(w) * hinv) for w in cands]
    return hinv, gains, exact


def _check_gains(got, fresh_gains, exact, n_live, what):
    assert got.dtype == torch.float64 and got.shape == fresh_gains.shape
    assert torch.equal(got[:, 0], fresh_gains[:, 0])  # the counts, as integers over W H
    for k in range(got.shape[0]):
        g, f32 = float(got[k, 1]), float(fresh_gains[k, 1])
        print(f"{what} pose {k}: eig {g!r}, exact {exact[k]!r} (relative {abs(g - exact[k]) / exact[k]:.3e}, bound "
              f"{4 * n_live * U64:.3e}), float32 {f32!r} (relative {abs(g - f32) / f32:.3e}, bound {4 * n_live * U32:.3e})")
        assert exact[k] > 0
        assert abs(g - exact[k]) <= 4 * n_live * U64 * exact[k]
        assert abs(g - f32) <= 4 * n_live * U32 * f32
    assert torch.equal(got[:, 2], got[:, 0] + got[:, 1])


def test_scorer_leaves_the_sequence_alone(cuda, runs):
    """With and without a scorer: the same poses, live map and draws, bit for bit; and the Monte-Carlo sample is
    two distinct poses of the three, from the scorer's own stream (it repeats for the seed)."""
    a, b = runs.snap["a"], runs.snap["b"]
    assert runs.live_counts["a"] == runs.live_counts["b"]
    for k in a:
        if k == "draws":
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) and len(a[k]) == len(b[k]) == N_FRAMES
        else:
            assert torch.equal(a[k], b[k]), k
    used = runs.a.scorer.used[:N_FRAMES]
    want = [int(i) for i in np.random.RandomState(3).choice(3, size=2, replace=False)]
    print(f"visited poses used per fit: {used}")
    assert used[:2] == [[0], [0, 1]]  # at most n_monte poses: all of them, nothing drawn
    assert used[2] == want and len(set(used[2])) == 2 and set(used[2]) <= {0, 1, 2}


def test_one_capture_across_map_changes(cuda, runs):
    seq = runs.a
    counts = runs.live_counts["a"]
    print(f"live rows after each frame {counts} (P0 {runs.P0}), {runs.pruned} marked prunable before the last frame")
    assert seq.scorer_captures == 1  # built after frame 0; frames 1-2 densified, pruned and compacted
    assert counts[1] != counts[0] and counts[2] != counts[1]
    n_live = counts[-1]
    live = seq.alive.bool()
    assert int(live.sum()) == n_live and bool(live[:n_live].all())  # compacted
    hinv_f, gains_f, exact = _fresh(seq, runs.cam, runs.cands)
    hinv = seq.fit_visited(check=True)
    assert seq.scorer.used[-1] == [0, 1, 2]
    assert torch.equal(hinv[live], hinv_f)
    assert torch.equal(hinv[~live], torch.reciprocal(torch.zeros_like(hinv[~live]) + 0.1))
    gains = seq.view_gains(runs.cands, check=True)  # five candidates: two launches of K = 4
    _check_gains(gains, gains_f, exact, n_live, "one capture")
    w = dict(k_sil=250.0, k_eig=0.3, k_sum=2.5)
    from splatam_amd.fisher import combine_gains
    npix = runs.cam.image_width * runs.cam.image_height
    cnt = (gains[:, 0] * npix).round().to(torch.int32)
    assert torch.equal(seq.view_gains(runs.cands, **w), combine_gains(cnt, gains[:, 1], npix, **w))
    assert seq.scorer_captures == 1
    # the map moves to a larger buffer: the scorer is stale, the next call rebuilds it and keeps H_train_inv
    old_capacity = seq.capacity
    assert seq.ensure_headroom(seq.capacity) and seq.capacity > old_capacity
    assert seq.scorer.stale and seq.scorer_captures == 1
    grown = seq.view_gains(runs.cands, check=True)
    assert seq.scorer_captures == 2 and not seq.scorer.stale
    _check_gains(grown, gains_f, exact, n_live, "after growth")
    live2 = seq.alive.bool()
    assert torch.equal(seq.fit_visited(check=True)[live2], hinv_f)
    _check_gains(seq.view_gains(runs.cands, check=True), gains_f, exact, n_live, "after growth, refitted")
    assert seq.scorer_captures == 2
