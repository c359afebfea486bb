"""Cases and assertions of the comparison with the reference's own kernels (oracle/reference.py: its
forward.cu / backward.cu / rasterizer_impl.cu compiled by hipcc for gfx950).  Shared by
tests/test_gpu_reference.py (the live library on the GPU: product, float32 oracle and float64 oracle
against it), tests/test_reference_goldens_cpu.py (both oracle builds against results recorded from it,
tests/golden/ref_raster/) and tools/record_reference_goldens.py (which records them).

The reference is the truth here.  Its backward is always BACKWARD::renderFused, so the oracle runs in
its fused form -- in mode VENDORED, which also replicates the two SH bugs of that kernel that the
oracle's FUSED mode and the product deliberately do not have (backward.cu:1067 reads the SH
coefficients of Gaussian g at float offset M g instead of 3 M g, which changes dmeans3D at degree >= 1;
backward.cu:1117 adds dL_dsh only if D > 0).  The product is compared after adding the float32 oracle's
own VENDORED - FUSED difference: zero on every tensor those two lines do not touch.

Asserted (`compare`), discrete state:
  * num_rendered, ranges, point_list equal.  Where a list differs, the lists are compared per tile as
    sets and the case is reported and counted against the cap (a float32 depth that differs by
    contraction reorders two keys); the float64 oracle's lists are compared that way throughout
    (its depths are not the float32 sort keys);
  * radii, tiles_touched: equal except on rows where the float32 and float64 oracles themselves
    disagree (a rect edge or a radius within float32 rounding of a decision); n_contrib: equal except at
    pixels either oracle build flags unstable_pix (an alpha within a relative 2e-5 of 1/255 or a
    T (1 - alpha) within 1e-4 of 1e-4);
  * at most CAP = 0.1 % of the Gaussians and of the pixels may be excused that way per case.
Values:
  * colour and depth image within 1e-4 max(1, |ref|) on >= 99.9 % of the pixels;
  * every gradient tensor within BOUND = 1e-4 relative L2 of the reference.  A tensor that is
    identically zero in the float64 oracle (drot of isotropic Gaussians: rounding noise of the atomics)
    must stay below 1e-5 of the largest reference gradient instead, harness.grad_accuracy's rule;
  * where a tensor misses 1e-4: the reference's own relative L2 distance d to the float64 oracle is
    taken (the larger of two runs; recorded with the goldens).  The candidate may then be no farther
    from float64 than max(1e-4, 2 d) -- farther is a finding, not a tolerance -- and its bound against
    the reference becomes max(1e-4, 2 d), harness.check_grad_accuracy's margin.  Every use of that rule
    is printed with d;
  * per row (test_gpu_edges._row_check with the reference as the truth), on the rows neither oracle
    build marks unstable: no row differs by more than the larger of 1e-3 of the row's norm and the row's
    float32 error scale; a row whose bound is zero is exactly zero.  The float32 error scale of a row is
    the larger of 3 x the float32 oracle's own error on it (_row_check's measure) and
    (n + 8) u |scale row|, where scale is the float64 oracle's error scale (oracle.backward(error_scale=True):
    the sums of the pairs' |terms| pushed through |Jacobian|), u = 2^-24 and n the frame's largest n_contrib:
    a pair's term carries the transmittance, a product of up to n rounded (1 - alpha) factors, so its
    relative error is bounded by gamma_n ~ n u (Higham 3.1), plus the handful of operations of the term
    itself; the sum's error is that times the sum of |terms|, whatever its cancellation.  (edge_stop257's
    dopacity row 31 is 3.0e-4 out of terms that sum to 0.84 in absolute value: 1e-3 of the row is 0.36 u of
    that sum, less than one rounding of one term.)
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import camera_scenes as cs
import edge_scenes as es
import sh_scenes as ss
from oracle import harness, oracle
from splatam_amd.scenes import make_scene

CAP = 1e-3
BOUND = 1e-4
SEEDS = ("randn", "fisher")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    build: object                 # () -> Scene
    kw: tuple = ()                # run kwargs: bg, use_sh, use_cov, scale_modifier
    runs: tuple = ((1, "randn"),)  # (power, seed kind)

    def scene(self):
        return self.build()

    def kwargs(self):
        return dict(self.kw)


def _runs(powers):
    """Power 1 with the random-sign seed; every higher power with both seeds."""
    out = [(1, "randn")]
    for p in powers:
        if p > 1:
            out += [(p, "randn"), (p, "fisher")]
    return tuple(out)


def dpix(scene, kind):
    """dL/dpixel [3,H,W] float32: random sign at scale 1e-2, or the constant 1e-3 Fisher seed."""
    c = scene.cam
    if kind == "fisher":
        return np.full((3, c.H, c.W), 1e-3, np.float32)
    return (np.random.RandomState(11).randn(3, c.H, c.W) * 1e-2).astype(np.float32)


def _widened(scene, M, seed):
    """`scene` with its SH rows widened to M stored coefficients (finite random values the active degree
    never reads -- except through the reference's M g offset, which the VENDORED oracle follows)."""
    n = scene.shs.shape[1]
    if M == n:
        return scene
    g = torch.Generator().manual_seed(seed)
    tail = torch.randn(scene.P, M - n, 3, generator=g) * 0.2
    return dataclasses.replace(scene, shs=torch.cat([scene.shs, tail], 1).contiguous())


# seeds: the first of 0.. at which the float32 and float64 oracles agree within CAP on the discrete state
# (tests/test_reference_goldens_cpu.py::test_inputs_sit_within_the_cap checks every case again)
R250 = [dict(name="iso", aniso=False, sh=0, cov=False, bg=(0.0, 0.0, 0.0)),
        dict(name="aniso", aniso=True, sh=0, cov=False, bg=(0.0, 0.0, 0.0)),
        dict(name="sh3", aniso=True, sh=3, cov=False, bg=(0.0, 0.0, 0.0)),
        dict(name="sh1_bg", aniso=True, sh=1, cov=False, bg=(0.3, 0.1, 0.7)),
        dict(name="cov3D", aniso=True, sh=0, cov=True, bg=(0.0, 0.0, 0.0))]
SEED_2500 = {"iso": 1, "aniso": 1}
SEED_250 = 2
SEED_RAGGED = 3
SEED_MOD = 4


# camera_scenes.SEED = 2 puts two of its 15 integer-centred `opaque` members with a rect edge exactly on a tile
# boundary (0.7 % of the rows; the float64 oracle then bins 7 more instances): 14 is the first seed of 0..119
# at which every case's float32 and float64 oracle agree on every row and every n_contrib
CAM_SEED = 14


def _camera_scene(c):
    return cs.build(c["pose"], c["aniso"], c["sh"], 1.0 if c.get("cov") else c["mod"], seed=CAM_SEED)[0]


def _cases():
    out = []
    for n, aniso in (("iso", False), ("aniso", True)):
        out.append(Case(f"r2500_{n}", functools.partial(make_scene, 2500, 96, 72, seed=SEED_2500[n], anisotropic=aniso),
                        runs=_runs((2, 3))))
    for c in R250:
        out.append(Case(f"r250_{c['name']}",
                        functools.partial(make_scene, 250, 64, 48, seed=SEED_250, anisotropic=c["aniso"],
                                          sh_degree=c["sh"]),
                        kw=(("bg", c["bg"]), ("use_sh", c["sh"] > 0), ("use_cov", c["cov"])),
                        runs=_runs((2, 3)) if c["name"] == "sh3" else _runs(())))
    out.append(Case("r250_ragged_100x75", functools.partial(make_scene, 250, 100, 75, seed=SEED_RAGGED, anisotropic=True)))
    out.append(Case("r250_mod0.7", functools.partial(make_scene, 250, 64, 48, seed=SEED_MOD, anisotropic=True),
                    kw=(("scale_modifier", 0.7),)))
    for D, M in ss.PAIRS:
        out.append(Case(f"sh_D{D}_M{M}", functools.partial(lambda D, M: _widened(ss.edge_scene(257, D), M, 100 + M), D, M),
                        kw=(("use_sh", True),)))
    for c in cs.CASES:
        kw = cs.run_kwargs(c)
        power = kw.pop("power")
        out.append(Case(f"cam_{c['name']}", functools.partial(_camera_scene, c), kw=tuple(kw.items()),
                        runs=((power, "randn"),) if power == 1 else ((power, "randn"), (power, "fisher"))))
    for o in es.ORDERS:
        out.append(Case(f"edge_sort257_{o}", functools.partial(lambda o: es.sort_scene(257, o).scene, o)))
    out.append(Case("edge_forward257", lambda: es.forward_scene(257).scene))
    for n in (256, 257):
        out.append(Case(f"edge_stop{n}", functools.partial(lambda n: es.forward_stop_scene(n).scene, n)))
    out.append(Case("edge_bwd_wide_129", lambda: es.backward_scene("wide", "entries_129").scene, runs=_runs((2, 3))))
    out.append(Case("edge_bwd_sh3_33", lambda: es.backward_scene("power_sh3", "entries_33").scene,
                    kw=(("use_sh", True),), runs=_runs((2, 3))))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c.name, p, s) for c in CASES for p, s in c.runs]
RUN_IDS = [f"{n}-p{p}-{s}" for n, p, s in RUNS]
# the cases recorded under tests/golden/ref_raster/ (tools/record_reference_goldens.py), at powers 1 and 2
GOLDEN_CASES = [f"r250_{c['name']}" for c in R250] + ["r250_mod0.7", "cam_posed_aniso_mod1.7", "cam_posed_sh3"]
GOLDEN_RUNS = [(n, p, "randn") for n in GOLDEN_CASES for p in (1, 2)]
FRAME_KEYS = ("color", "depth", "radii", "n_contrib", "ranges", "point_list", "tiles_touched", "final_T")


def mark_visible_inputs():
    """The inputs of tests/test_gpu_parity.py::test_mark_visible_matches_oracle."""
    from splatam_amd.scenes import setup_camera
    g = torch.Generator().manual_seed(21)
    pts = torch.randn(5000, 3, generator=g) * 2.0
    pts[:16, 2] = torch.tensor([0.001, 0.0010001, 0.0009999, -0.001, 0.0, 1e-7, -1e-7, 0.002] * 2)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    return pts, setup_camera(64, 48, 50.0, 50.0, 31.5, 23.5, w2c=w2c)


def scene_inputs(scene, kw):
    """The inputs of a case as the arrays recorded with its golden file (keys in_*)."""
    c = scene.cam
    d = dict(means3D=scene.means3D.numpy(), scales=scene.scales.numpy(), rotations=scene.rotations.numpy(),
             opacities=scene.opacities.numpy(), colors=scene.colors.numpy(), view=c.viewmatrix.numpy(),
             proj=c.projmatrix.numpy(), campos=c.campos.numpy(), tanfov=np.array([c.tanfovx, c.tanfovy], np.float64),
             size=np.array([c.H, c.W], np.int32), bg=np.asarray(kw.get("bg", (0.0, 0.0, 0.0)), np.float32),
             scale_modifier=np.float32(kw.get("scale_modifier", 1.0)), sh_degree=np.int32(scene.sh_degree),
             use_sh=np.bool_(kw.get("use_sh", False)), use_cov=np.bool_(kw.get("use_cov", False)))
    if scene.shs is not None:
        d["shs"] = scene.shs.numpy()
    return {"in_" + k: v for k, v in d.items()}


def frame_dict(fr):
    d = {k: np.asarray(getattr(fr, k)) for k in FRAME_KEYS}
    d["num_rendered"] = int(fr.num_rendered)
    return d


def frames_of(scene, kw):
    """(float32 frame, float64 frame) of the oracle on a scene."""
    fr32, _ = harness.run_oracle(scene, backward=False, **kw)
    fr64, _ = harness.run_oracle(scene, backward=False, dtype=np.float64, **kw)
    return fr32, fr64


def grads_of(fr32, fr64, d, power):
    """(float32 VENDORED, float32 FUSED, float64 VENDORED with error scale) gradients for dL/dpixel d."""
    v32 = oracle.backward(fr32, d, power=power, mode=oracle.VENDORED)
    f32 = oracle.backward(fr32, d, power=power, mode=oracle.FUSED)
    v64 = oracle.backward(fr64, np.asarray(d, np.float64), power=power, mode=oracle.VENDORED, error_scale=True)
    return v32, f32, v64


@functools.lru_cache(maxsize=None)
def oracle_frames(name):
    """(scene, float32 frame, float64 frame) of a case."""
    case = BY_NAME[name]
    scene = case.scene()
    return (scene,) + frames_of(scene, case.kwargs())


@functools.lru_cache(maxsize=None)
def oracle_grads(name, power, seed):
    scene, fr32, fr64 = oracle_frames(name)
    return grads_of(fr32, fr64, dpix(scene, seed), power)


def recorded_scene(z):
    """(scene, run kwargs) from the in_* arrays of a golden file: the inputs the reference ran on, bit for bit
    (make_scene is not bit-reproducible across hosts: torch's CPU exp differs in the last place)."""
    import types
    t = lambda k: torch.from_numpy(np.array(z["in_" + k]))  # noqa: E731
    H, W = (int(x) for x in z["in_size"])
    cam = types.SimpleNamespace(H=H, W=W, viewmatrix=t("view"), projmatrix=t("proj"), campos=t("campos"),
                                tanfovx=float(z["in_tanfov"][0]), tanfovy=float(z["in_tanfov"][1]))
    from splatam_amd.scenes import Scene
    scene = Scene(means3D=t("means3D"), scales=t("scales"), rotations=t("rotations"), opacities=t("opacities"),
                  colors=t("colors"), shs=t("shs") if "in_shs" in z else None, sh_degree=int(z["in_sh_degree"]), cam=cam)
    kw = dict(bg=tuple(float(x) for x in z["in_bg"]), use_sh=bool(z["in_use_sh"]), use_cov=bool(z["in_use_cov"]),
              scale_modifier=float(z["in_scale_modifier"]))
    return scene, kw


def _tile_sets_equal(a, ra, b, rb):
    if ra.shape != rb.shape:
        return False
    for (a0, a1), (b0, b1) in zip(ra, rb):
        if a1 - a0 != b1 - b0 or not np.array_equal(np.sort(a[a0:a1]), np.sort(b[b0:b1])):
            return False
    return True


def excused(fr32, fr64):
    """(rows, pixels) on which a float32 implementation may decide differently: see the module docstring."""
    rows = (fr32.radii != fr64.radii) | (fr32.tiles_touched != fr64.tiles_touched)
    return rows, fr32.unstable_pix | fr64.unstable_pix


def input_check(fr32, fr64):
    """The float32 oracle against the float64 oracle alone: the share of rows / pixels whose discrete
    state differs, and whether the lists agree exactly / as per-tile sets."""
    rows = (fr32.radii != fr64.radii) | (fr32.tiles_touched != fr64.tiles_touched)
    pix = fr32.n_contrib != fr64.n_contrib
    exact = (fr32.num_rendered == fr64.num_rendered and np.array_equal(fr32.ranges, fr64.ranges)
             and np.array_equal(fr32.point_list, fr64.point_list))
    sets = exact or _tile_sets_equal(fr32.point_list, fr32.ranges, fr64.point_list, fr64.ranges)
    return dict(rows=float(rows.mean()), pixels=float(pix.mean()), lists_exact=exact, lists_as_sets=sets,
                unflagged_pixels=int((pix & ~(fr32.unstable_pix | fr64.unstable_pix)).sum()))


def compare_frame(tag, ref, cand, fr32, fr64, *, lists="exact"):
    """Discrete state and images of `cand` (a frame dict; keys it lacks are not compared) against the
    reference's `ref`.  Returns (report string, failures)."""
    fails, notes = [], []
    ex_rows, ex_pix = excused(fr32, fr64)
    P, N = ex_rows.size, ex_pix.size
    used_rows = np.zeros(P, bool)
    used_pix = np.zeros(ex_pix.shape, bool)
    list_diverged = False
    same = (cand["num_rendered"] == ref["num_rendered"] and np.array_equal(cand["ranges"], ref["ranges"])
            and np.array_equal(cand["point_list"], ref["point_list"]))
    if not same:
        as_sets = _tile_sets_equal(cand["point_list"], cand["ranges"], ref["point_list"], ref["ranges"])
        if lists == "exact" and as_sets:
            list_diverged = True  # reported, counted against the cap
            moved = np.unique(ref["point_list"][cand["point_list"] != ref["point_list"]])
            used_rows[moved] = True
            notes.append(f"LISTS DIVERGE in order only ({moved.size} Gaussians reordered)")
        elif not as_sets:
            if cand["num_rendered"] != ref["num_rendered"] and ex_rows.any():
                notes.append("lists differ with excused rows present")
                used_rows |= ex_rows
            else:
                fails.append(f"{tag}: lists differ (num_rendered {cand['num_rendered']} vs {ref['num_rendered']})")
    for k in ("radii", "tiles_touched"):
        if k in cand and k in ref:
            d = cand[k] != ref[k]
            if (d & ~ex_rows).any():
                fails.append(f"{tag}: {k} differs on rows {np.nonzero(d & ~ex_rows)[0][:8].tolist()} away from any decision")
            used_rows |= d
    d = cand["n_contrib"].reshape(ex_pix.shape) != ref["n_contrib"].reshape(ex_pix.shape)
    if (d & ~ex_pix).any():
        fails.append(f"{tag}: n_contrib differs at {int((d & ~ex_pix).sum())} pixels away from any decision")
    used_pix |= d
    share_r, share_p = used_rows.sum() / P, used_pix.sum() / N
    if share_r > CAP or share_p > CAP:
        fails.append(f"{tag}: excused {share_r:.2%} of the Gaussians, {share_p:.2%} of the pixels: cap {CAP:.1%}")
    vals = []
    for k in ("color", "depth"):
        c = np.asarray(cand[k], np.float64).reshape(ref[k].shape)
        r = np.asarray(ref[k], np.float64)
        bad = (np.abs(c - r) > 1e-4 * np.maximum(1.0, np.abs(r))).any(axis=0)
        vals.append(f"{k} max|d| {np.abs(c - r).max():.1e} bad {bad.mean():.2%}")
        if bad.mean() > 1e-3:
            fails.append(f"{tag}: {k} off on {bad.mean():.2%} of the pixels")
    rep = (f"{tag}: lists {'equal' if same else 'DIVERGED' if list_diverged else 'as sets' if not fails else 'DIFFER'}, "
           f"excused rows {share_r:.2%} pixels {share_p:.2%} (cap {CAP:.1%}), " + ", ".join(vals)
           + ("; " + "; ".join(notes) if notes else ""))
    return rep, fails


def _mag(g):
    return max(float(np.abs(np.asarray(v)).max()) for k, v in g.items() if k in harness.GRAD_KEYS and np.asarray(v).size)


def compare_grads(tag, ref, ref_dist64, cand, v32, v64, stable, nmax, keys=None):
    """Gradients `cand` against the reference's `ref`.  ref_dist64[k]: the reference's own relative L2
    distance to the float64 oracle (the larger of two runs).  Returns (report, failures)."""
    fails, parts = [], []
    mag = _mag(ref)
    for k in harness.GRAD_KEYS:
        if k not in cand or (keys is not None and k not in keys) or np.asarray(ref[k]).size == 0:
            continue
        r = np.asarray(ref[k], np.float64)
        P = r.shape[0]
        x = np.asarray(cand[k], np.float64).reshape(r.shape)
        b64 = np.asarray(v64[k], np.float64).reshape(r.shape)
        if not b64.any():
            worst = float(np.abs(x - r).max())
            parts.append(f"{k} zero in float64, max|d| {worst:.1e}")
            if worst > 1e-5 * mag:
                fails.append(f"{tag}: {k} is zero in float64, differs by {worst:.2e} > 1e-5 x {mag:.2e}")
            continue
        e = harness.rel_l2(x, r)
        bound = BOUND
        if e > BOUND:
            d = float(ref_dist64[k])
            mine = harness.rel_l2(x, b64)
            bound = max(BOUND, 2 * d)
            parts.append(f"{k} {e:.2e} RAISED bound {bound:.2e} (reference is {d:.2e} from float64, candidate {mine:.2e})")
            if mine > bound:
                fails.append(f"{tag}: {k} is {mine:.2e} from float64, the reference only {d:.2e}: a finding")
            if e > bound:
                fails.append(f"{tag}: {k} rel L2 {e:.2e} > {bound:.2e}")
        else:
            parts.append(f"{k} {e:.1e}")
        # per row, stable rows
        o32 = np.asarray(v32[k], np.float64).reshape(P, -1)
        xr, rr, br = x.reshape(P, -1), r.reshape(P, -1), b64.reshape(P, -1)
        err = np.linalg.norm(xr - rr, axis=1)
        sc = np.asarray(v64["scale"][k], np.float64).reshape(P, -1)
        rb = np.maximum(1e-3 * np.linalg.norm(rr, axis=1),
                        np.maximum(3 * np.linalg.norm(o32 - br, axis=1), (nmax + 8) * 2.0 ** -24 * np.linalg.norm(sc, axis=1)))
        zero = rb == 0
        if (err[zero & stable] != 0).any():
            fails.append(f"{tag}: {k} rows {np.nonzero((err != 0) & zero & stable)[0][:8].tolist()} are not exactly zero")
        ratio = np.where(zero | ~stable, 0.0, err / np.where(zero, 1.0, rb))
        if ratio.max() > 1.0:
            fails.append(f"{tag}: {k} row {int(ratio.argmax())} is {ratio.max():.2f} x its bound")
        parts[-1] += f" row {ratio.max():.2f}"
    return f"{tag}: " + ", ".join(parts), fails


def reference_distance(runs, v64):
    """The reference's relative L2 distance to the float64 oracle per tensor: the larger of `runs`."""
    out = {}
    for k in harness.GRAD_KEYS:
        b = np.asarray(v64[k], np.float64)
        out[k] = max(harness.rel_l2(np.asarray(g[k], np.float64).reshape(b.shape), b) for g in runs) if b.size else 0.0
    return out
