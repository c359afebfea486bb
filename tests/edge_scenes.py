"""Constructed scenes whose tile-list lengths and block-mask popcounts are chosen, not drawn
(tests/test_edge_scenes_cpu.py checks the construction on the CPU oracle, tests/test_gpu_edges.py
uses it to put the rasterizer's tile pipeline on its exact edges).

Images are one tile high and 1-3 tiles wide, the pose is the identity, fx = fy = 100, the principal
point is the image centre, every Gaussian is isotropic.  A tile's list is given front to back as
tokens; each token is a footprint class (the 4x4 blocks its alpha >= 1/255 ellipse reaches):

  full   16 blocks: 2D sigma 20 px, centre within 0.3 px of the tile centre, opacity 0.01
         (alpha in [0.0085, 0.01] at every pixel of the tile);
  flat   16 blocks: sigma 60 px exactly on the tile centre, opacity 0.01 (alpha within 2 % over the
         tile: the stopper scenes' ordinary entries, so that T is nearly uniform);
  block / pair / quad   1 / 2 / 4 blocks: sigma^2 = 0.5 px^2 centred on a block centre / a vertical
         block edge / a block corner.  Opacity 0.1412: alpha >= 2.9/255 at the pixels within d^2 <= 2.5
         of the centre and <= 0.4/255 from d^2 = 4.5 on; `dim` scenes use 0.0194 (alpha = 3/255 at the
         four nearest pixels, <= 0.41/255 elsewhere) so that several hundred entries fit on one block;
  ("flat", o)   a flat entry of opacity o: the stoppers (0.93), the trimming last contributor and the
         blocker (0.97) of a stopper scene (stop_tokens).

Depths come from eight values, so most keys tie on depth and the id half of the sort key decides.
`order` says how ids go with depth: "asc" (ids ascend with depth), "desc" (ids descend with depth),
"equal" (one depth), "random" (a random assignment; inside a depth tie ids ascend along the list,
as the sort demands).  Small classes of a multi-tile image sit at least 3 px inside their tile
(`inner` sites), so their radius-3 rect touches no neighbouring tile."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

from splatam_amd.scenes import Scene, setup_camera

FX = 100.0
LEVELS = 2.0 + 0.25 * np.arange(8)
SIGMA = dict(full=20.0, flat=60.0, small=np.sqrt(0.5))
O_FULL, O_SMALL, O_DIM = 0.01, 0.1412, 0.0194
O_STOP, O_BLOCKER = 0.93, 0.97
POPCOUNT = dict(full=16, flat=16, block=1, pair=2, quad=4)

# Batch size BB and slot budget BS of every render-backward variant (csrc/gsr_render_bwd.h bwd_batch() /
# bwd_slots(), render_bwd_fisher_kernel and PowerShape::BATCH in csrc/gsr_backward_power.hip; the power
# path has no slot budget).  test_edge_scenes_cpu.py::test_budget_table_matches_sources reads the sources.
BUDGETS = {
    "wide": (128, 384), "wide_dual": (128, 384), "tracking": (128, 512), "mom1": (128, 256), "mom2": (128, 128),
    "power_sh0": (64, None), "power_sh3": (32, None), "fisher": (128, 512),
}
RENDER_BATCH = 256
TILE_SORT_CAP = 4096


def block_of_pixel():
    """Pixel (px, py) inside the tile and 4x4-block bit of each of the 256 threads of a tile."""
    tid = np.arange(256)
    px = 8 * ((tid >> 6) & 1) + 4 * ((tid >> 4) & 1) + (tid & 3)
    py = 8 * (tid >> 7) + 4 * ((tid >> 5) & 1) + ((tid >> 2) & 3)
    return px, py, tid >> 4


def exact_masks(m2, co, W, H, tx, ty):
    """float64 ellipse-vs-block masks (the kernel's construction without its margins): the alpha >= 1/255
    ellipse's x-extent over each block row's y-span against the block columns' pixel-centre spans."""
    ax, ay = m2[:, 0], m2[:, 1]
    A, B, C, o = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
    det = A * C - B * B
    tau = np.log(np.maximum(255.0 * o, 1e-30))
    out = np.zeros(len(ax), np.int64)
    ok = (det > 0) & (A > 0) & (tau > 0)
    x0, y0 = 16.0 * tx, 16.0 * ty
    with np.errstate(invalid="ignore", divide="ignore"):
        hy = np.sqrt(2 * tau * A / det)
        us = B * np.sqrt(2 * tau / (det * C))
        for r in range(4):
            lo = np.maximum(y0 + 4 * r - ay, -hy)
            hi = np.minimum(y0 + 4 * r + 3 - ay, hy)
            row = lo <= hi
            ul = np.clip(us, lo, hi)
            ur = np.clip(-us, lo, hi)
            wl = np.sqrt(np.maximum(2 * tau * A - det * ul * ul, 0))
            wr = np.sqrt(np.maximum(2 * tau * A - det * ur * ur, 0))
            xmin = ax + (-B * ul - wl) / A
            xmax = ax + (-B * ur + wr) / A
            for c in range(4):
                hit = ok & row & (xmax >= x0 + 4 * c) & (xmin <= x0 + 4 * c + 3)
                bit = 4 * (2 * (r >> 1) + (c >> 1)) + 2 * (r & 1) + (c & 1)
                out |= hit.astype(np.int64) << bit
    return out


def _sites(cls, inner):
    if cls == "block":
        cols = (1, 2) if inner else (0, 1, 2, 3)
        return [(4 * c + 1.5, 4 * r + 1.5) for r in range(4) for c in cols]
    if cls == "pair":
        return [(4 * c + 3.5, 4 * r + 1.5) for r in range(4) for c in range(3)]
    if cls == "quad":
        return [(4 * c + 3.5, 4 * r + 3.5) for r in range(3) for c in range(3)]
    raise ValueError(cls)


@dataclass
class EdgeScene:
    scene: Scene
    lists: list            # per tile: Gaussian ids front to back (the designed list)
    cls: np.ndarray        # [P] class name of each Gaussian
    popcount: np.ndarray   # [P] blocks its footprint reaches
    render: bool = True    # the scene meets the no-threshold conditions (False: sort-only scenes whose
                           # long lists run every pixel out of transmittance)
    n_contrib: int | None = None   # stopper scenes: every pixel's last contributor (a count)
    batches: list = field(default_factory=list)  # designed backward batches of tile 0, from the list's back

    @property
    def lengths(self):
        return [len(x) for x in self.lists]


def build(tiles, *, order="asc", seed=0, sh_degree=0, dim=False, render=True, n_contrib=None, batches=()):
    """tiles: per tile the list of tokens front to back.  Returns the EdgeScene."""
    rs = np.random.RandomState(seed)
    nt = len(tiles)
    W, H = 16 * nt, 16
    P = sum(len(t) for t in tiles)
    # ids of each tile
    if order == "random":
        perm = rs.permutation(P)
    else:
        perm = np.arange(P)
    bounds = np.cumsum([0] + [len(t) for t in tiles])
    px, py, sg, op, zz = (np.zeros(P) for _ in range(5))
    cls, lists, counters = np.empty(P, object), [], {}
    for t, toks in enumerate(tiles):
        n = len(toks)
        ids = np.sort(perm[bounds[t]:bounds[t + 1]])
        lev = np.minimum(7, (np.arange(n) * 8) // max(n, 1)) if order != "equal" else np.full(n, 3)
        groups = [np.nonzero(lev == k)[0] for k in range(8)]
        # which ids each depth group gets; inside a group ids ascend along the list
        if order == "desc":
            take, hi = [], n
            for g in groups:
                take.append(ids[hi - len(g):hi])
                hi -= len(g)
        elif order == "random":
            sh = rs.permutation(ids)
            cut = np.cumsum([0] + [len(g) for g in groups])
            take = [np.sort(sh[cut[k]:cut[k + 1]]) for k in range(8)]
        else:
            cut = np.cumsum([0] + [len(g) for g in groups])
            take = [ids[cut[k]:cut[k + 1]] for k in range(8)]
        gid = np.zeros(n, np.int64)
        for g, tk in zip(groups, take):
            gid[g] = tk
        lists.append(gid)
        for k, tok in enumerate(toks):
            c, o = (tok, None) if isinstance(tok, str) else tok
            i = gid[k]
            cls[i], zz[i] = c, LEVELS[lev[k]]
            if c == "full":
                jit = rs.uniform(-0.3, 0.3, 2)
                px[i], py[i], sg[i], op[i] = 7.5 + jit[0], 7.5 + jit[1], SIGMA["full"], O_FULL
            elif c == "flat":
                px[i], py[i], sg[i], op[i] = 7.5, 7.5, SIGMA["flat"], O_FULL if o is None else o
            else:
                s = _sites(c, inner=nt > 1)
                j = counters.get((t, c), 0)
                counters[(t, c)] = j + 1
                px[i], py[i] = s[j % len(s)]
                sg[i], op[i] = SIGMA["small"], (O_DIM if dim else O_SMALL)
            px[i] += 16 * t
    cx, cy = W / 2.0, H / 2.0
    means = np.stack([(px - (cx - 0.5)) * zz / FX, (py - (cy - 0.5)) * zz / FX, zz], 1)
    scale = np.sqrt(sg * sg - 0.3) * zz / FX
    rot = np.zeros((P, 4))
    rot[:, 0] = 1.0
    rgb = rs.uniform(0.2, 0.8, (P, 3))
    shs = None
    if sh_degree > 0:
        M = (sh_degree + 1) ** 2
        shs = 0.02 * rs.randn(P, M, 3)  # far from the colour clamp at 0
        shs[:, 0] = (rgb - 0.5) / 0.28209479177387814
        shs = torch.tensor(shs, dtype=torch.float32)
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32)  # noqa: E731
    scene = Scene(means3D=f32(means), scales=f32(np.repeat(scale[:, None], 3, 1)), rotations=f32(rot),
                  opacities=f32(op[:, None]), colors=f32(rgb), shs=shs, sh_degree=sh_degree,
                  cam=setup_camera(W, H, FX, FX, cx, cy))
    pc = np.array([POPCOUNT[c] for c in cls], np.int64)
    return EdgeScene(scene=scene, lists=lists, cls=cls, popcount=pc, render=render, n_contrib=n_contrib,
                     batches=list(batches))


def stop_tokens(n_contrib, n_tail, tail="full"):
    """A one-tile list whose every pixel's last contributor is entry n_contrib - 1: flat entries, 0.93
    stoppers, a trimming flat entry that leaves T near 3e-4 everywhere, then a 0.97 blocker whose test_T
    is below 5e-5 everywhere (it ends every pixel without contributing) and n_tail more entries."""
    X, Y, _ = block_of_pixel()
    d2 = (X - 7.5) ** 2 + (Y - 7.5) ** 2
    g = np.exp(-d2 / (2 * SIGMA["flat"] ** 2))
    for m in range(6):
        n_pre = n_contrib - m - 1
        if n_pre < 0:
            break
        T = (1 - O_FULL * g) ** n_pre * (1 - O_STOP * g) ** m
        o_t = 1 - 3e-4 / float(np.sqrt(T.min() * T.max()))
        if not 0.05 <= o_t <= 0.96:
            continue
        Ta = T * (1 - o_t * g)
        if Ta.min() >= 2.2e-4 and (Ta * (1 - O_BLOCKER * g)).max() <= 4.5e-5:
            return (["flat"] * n_pre + [("flat", O_STOP)] * m + [("flat", o_t), ("flat", O_BLOCKER)] +
                    [tail] * n_tail)
    raise ValueError(f"no stopper sequence for n_contrib = {n_contrib}")


def cut_batches(popcounts_back, BB, BS):
    """The backward's batch rule restated: walking from the last contributor, a batch is the longest
    prefix of at most BB entries whose popcounts sum to at most BS (BS None: no slot budget)."""
    out, i, n = [], 0, len(popcounts_back)
    while i < n:
        k, s = 0, 0
        while i + k < n and k < BB and (BS is None or s + popcounts_back[i + k] <= BS):
            s += popcounts_back[i + k]
            k += 1
        assert k > 0
        out.append(k)
        i += k
    return out


# ------------------------------------------------------------------ the scenes the GPU tests use --
SORT_LENGTHS = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4095, 4096,
                4097)
SORT_ORDER_LENGTHS = (257, 513, 1025, 2049, 4096, 4097)
ORDERS = ("asc", "desc", "equal", "random")
SORT_LAYOUTS = ((1025, 1, 257), (257, 2049, 2))
FWD_LENGTHS = (255, 256, 257, 511, 512, 513, 769)
FWD_STOPS = (255, 256, 257, 258)  # n_contrib: the last contributor is entry 254 ... 257


@functools.lru_cache(maxsize=None)
def sort_scene(L, order="random"):
    return build([["full"] * L], order=order, seed=L, render=L <= 769)


@functools.lru_cache(maxsize=None)
def sort_layout(lengths):
    return build([["block"] * n for n in lengths], order="random", seed=sum(lengths), dim=True)


@functools.lru_cache(maxsize=None)
def forward_scene(L):
    return build([["full"] * L], order="random", seed=1000 + L)


@functools.lru_cache(maxsize=None)
def forward_stop_scene(n_contrib):
    return build([stop_tokens(n_contrib, 100)], order="random", seed=2000 + n_contrib, n_contrib=n_contrib)


def backward_names(variant):
    BB, BS = BUDGETS[variant]
    names = [f"entries_{L}" for L in (BB - 1, BB, BB + 1, 2 * BB, 2 * BB + 1)]
    if BS is not None:
        n = BS // 16
        names += [f"slots_{L}" for L in (n - 1, n, n + 1, 2 * n + 1)]
        names += ["mixed_exact", "mixed_short", "mixed_refetch", "mixed_last_one"]
    names += ["stop_tail_bb", "stop_tail_bb1"]
    return names


@functools.lru_cache(maxsize=None)
def backward_scene(variant, name):
    """The backward edge scenes of a variant (one tile); .batches holds the designed batch sizes from the
    list's back."""
    BB, BS = BUDGETS[variant]
    sh = {"mom2": 1, "power_sh3": 3}.get(variant, 0)
    seed = 3000 + 17 * sorted(BUDGETS).index(variant)
    kind, _, arg = name.partition("_")
    if kind == "entries":
        L = int(arg)
        return build([["block"] * L], order="random", seed=seed + L, sh_degree=sh,
                     batches=cut_batches([1] * L, BB, BS))
    if kind == "slots":
        L = int(arg)
        return build([["full"] * L], order="random", seed=seed + L, sh_degree=sh,
                     batches=cut_batches([16] * L, BB, BS))
    if kind == "stop":
        tail = BB - 1 if arg == "tail_bb" else BB  # with the blocker: BB / BB + 1 entries behind the last contributor
        nc = 6
        return build([stop_tokens(nc, tail, tail="block")], order="asc", seed=seed + tail, sh_degree=sh,
                     n_contrib=nc, batches=[nc])
    n = BS // 16
    if arg == "exact":     # the running popcount lands exactly on BS at a pair: it stays in the batch
        back, want = ["full"] * (n - 1) + ["quad"] * 3 + ["pair", "pair", "full", "block", "block"], [n + 4, 3]
    elif arg == "short":   # BS - 1 slots, then a full entry: the cut falls before it
        back, want = ["full"] * (n - 1) + ["quad"] * 3 + ["pair", "block", "full", "block", "block"], [n + 4, 3]
    elif arg == "refetch":  # a batch cut by its slots, then a batch of BB entries, then the rest
        back, want = ["full"] * n + ["block"] * (BB + 5), [n, BB, 5]
    elif arg == "last_one":  # a cut leaves a last batch of one entry
        back, want = ["full"] * (n - 1) + ["pair"] * 8 + ["quad"], [n + 7, 1]
    else:
        raise ValueError(name)
    assert cut_batches([POPCOUNT[c] for c in back], BB, BS) == want, (variant, name)
    return build([back[::-1]], order="random", seed=seed + len(back), sh_degree=sh, batches=want)


def all_scenes():
    """(name, EdgeScene) of every scene the GPU tests use."""
    for L in SORT_LENGTHS:
        yield f"sort_{L}", sort_scene(L)
    for L in SORT_ORDER_LENGTHS:
        for o in ORDERS:
            yield f"sort_{L}_{o}", sort_scene(L, o)
    for lay in SORT_LAYOUTS:
        yield "layout_" + "_".join(map(str, lay)), sort_layout(lay)
    for L in FWD_LENGTHS:
        yield f"fwd_{L}", forward_scene(L)
    for n in FWD_STOPS:
        yield f"fwd_stop_{n}", forward_stop_scene(n)
    for v in BUDGETS:
        for name in backward_names(v):
            yield f"bwd_{v}_{name}", backward_scene(v, name)
