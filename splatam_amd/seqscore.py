"""View scoring on a running sequence's padded map (scripts/ros_handler.py:251-359, 807-836; splatam_amd.fisher).

The active-mapping node around the realtime loop scores candidate views after every frame: view_scorer builds
fisher.SequenceFisher graphs on the padded map once, fit_visited and view_gains replay them on the map as it
stands -- nothing on the frame() / push() path changes, and the scorer's Monte-Carlo draws come from a stream of
its own (`draws` and every result of the sequence are untouched).  SlamSequence inherits these methods
(ViewScoring); they read its params, alive, cam, bin_capacity, sil_thres and tracking_iters_run.
"""
from __future__ import annotations

import numpy as np
import torch

from .fisher import H_EPS, SequenceFisher
from .keyframes import pose_w2c


class ViewScorer:
    """What SlamSequence.view_scorer caches: the two SequenceFisher graphs (`sum`, `gains`; gains.H_inv holds
    H_train_inv once `fitted`), the Monte-Carlo settings with the scorer's own random stream, and `used`, the
    visited-pose indices of every fit_visited call.  `stale`: the map moved to other buffers; the graphs are
    rebuilt by the next scoring call (`carried`: H_train_inv's live rows until then)."""

    def __init__(self, K: int, n_monte, seed: int):
        self.K, self.n_monte, self.seed = K, (None if n_monte is None else int(n_monte)), seed
        self.rng = np.random.RandomState(seed)
        self.used = []
        self.sum = self.gains = None
        self.fitted, self.stale, self.carried = False, False, None


class ViewScoring:
    """SlamSequence's view-scoring methods."""

    scorer = None         # the cached ViewScorer (view_scorer)
    scorer_captures = 0   # how often its two graphs were built: once, plus once per ensure_headroom that grew

    def _retire_scorer(self):
        """The map is about to move to other buffers (_build): the cached scorer's graphs read the old ones.
        Its H_train_inv is kept by live row -- the new buffers hold the live rows first, in order -- and the
        next scoring call rebuilds the graphs.  (Called where the host already synchronises.)"""
        sc = self.scorer
        if sc is None or sc.stale:
            return
        sc.stale = True
        sc.carried = sc.gains.H_inv[self.alive.bool()].clone() if sc.fitted else None
        sc.sum = sc.gains = None

    def view_scorer(self, K: int = 16, n_monte: int | None = None, seed: int = 0):
        """The sequence's view scorer: fisher.SequenceFisher graphs (modes "sum" and "gains", K poses per
        launch) on self.params / self.alive / self.cam / self.bin_capacity, built once and cached -- every
        replay sees the map as it then stands, so frames that densify, prune and compact need no rebuild.
        n_monte: fit_visited's Monte-Carlo sample size (the reference's N_monte_carlo); its draws come from the
        scorer's own RandomState(seed), never from the sequence's stream.  Returns the ViewScorer."""
        old = self.scorer
        sc = ViewScorer(int(K), n_monte, seed)
        mk = lambda mode: SequenceFisher(self.params, self.alive, self.cam, sc.K, mode, self.bin_capacity,  # noqa: E731
                                         self.sil_thres)
        sc.sum, sc.gains = mk("sum"), mk("gains")
        if old is not None and old.stale and (old.K, old.n_monte, old.seed) == (sc.K, sc.n_monte, sc.seed):
            sc.rng, sc.used = old.rng, old.used  # the same scorer on new buffers: its stream goes on
            if old.carried is not None:
                with torch.no_grad():
                    sc.gains.H_inv.copy_(torch.reciprocal(torch.zeros_like(sc.gains.H_inv) + H_EPS))
                    sc.gains.H_inv[:old.carried.shape[0]] = old.carried
                sc.fitted = True
        self.scorer = sc
        self.scorer_captures += 1
        return sc

    def _scorer(self):
        sc = self.scorer
        if sc is None:
            return self.view_scorer()
        return self.view_scorer(sc.K, sc.n_monte, sc.seed) if sc.stale else sc

    def visited_w2cs(self) -> list:
        """The poses of the frames run so far, relative to frame 0 ([4,4] device tensors; nothing read back):
        the identity for frame 0, pose_w2c of the estimated (or given) pose column for the others."""
        dev = self.alive.device
        return [torch.eye(4, device=dev) if t == 0 else pose_w2c(self.params, t)
                for t in range(len(self.tracking_iters_run))]

    def fit_visited(self, w2cs=None, n_monte: int | None = None, check: bool = False) -> torch.Tensor:
        """compute_H_visited_inv (scripts/ros_handler.py:807-829) on the map as it stands: H_train_inv =
        reciprocal(H_train + 0.1) over the padded rows [capacity + 1, 4] (a dead row's H_train is +0), H_train
        the sum of the visited poses' Hessians, K per graph launch.  w2cs None: visited_w2cs().  With n_monte
        (default: view_scorer's) and more poses than that, a sample without replacement
        (RandomState.choice, the reference's np.random.choice) from the scorer's own stream; `scorer.used`
        records each call's pose indices.  Nothing is read back unless `check` (raises on a binning overflow)."""
        sc = self._scorer()
        w2cs = self.visited_w2cs() if w2cs is None else list(w2cs)
        n_monte = sc.n_monte if n_monte is None else int(n_monte)
        idx = list(range(len(w2cs)))
        if n_monte is not None and len(w2cs) > n_monte:
            idx = [int(i) for i in sc.rng.choice(len(w2cs), size=n_monte, replace=False)]
        sc.used.append(idx)
        H = None
        for c in range(0, len(idx), sc.K):
            h = sc.sum.hessian_sum([w2cs[i] for i in idx[c:c + sc.K]], check=check)
            if h is None:
                raise RuntimeError("SlamSequence.fit_visited: a pose overflowed the binning capacity")
            H = h.clone() if H is None else H + h
        with torch.no_grad():
            if H is None:
                H = torch.zeros_like(sc.gains.H_inv)
            torch.reciprocal(H + H_EPS, out=sc.gains.H_inv)
        sc.fitted = True
        return sc.gains.H_inv

    def view_gains(self, w2cs, check: bool = False, **weights) -> torch.Tensor:
        """send_gains' (g_sil, g_eig, gain) of every candidate pose against fit_visited's H_train_inv: float64
        [n,3] on the device, like FisherScorer.view_gains (weights: combine_gains').  K candidates per graph
        launch; nothing is read back unless `check` (raises on a binning overflow)."""
        sc = self._scorer()
        if not sc.fitted:
            raise RuntimeError("fit_visited() first (H_train_inv)")
        w2cs = list(w2cs)
        out = torch.zeros(len(w2cs), 3, dtype=torch.float64, device=self.alive.device)
        for c in range(0, len(w2cs), sc.K):
            g = sc.gains.gains(w2cs[c:c + sc.K], sc.gains.H_inv, check=check, **weights)
            if g is None:
                raise RuntimeError("SlamSequence.view_gains: a pose overflowed the binning capacity")
            out[c:c + g.shape[0]] = g
        return out
