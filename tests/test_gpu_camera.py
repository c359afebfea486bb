"""The HIP rasterizer against the CPU oracle off the identity camera, class by class, on the constructed
scenes of tests/camera_scenes.py (a rotated and translated camera, the +-1.3 tanfov clamp, the near plane
at 0.001, off-screen centres, scale_modifier != 1, alpha at the 0.99 clamp, the SH colour clamp per channel;
tests/test_camera_scenes_cpu.py pins the oracle itself there and bounds the near-threshold sets).

Criteria, all from what the suite already uses:
  * colour: |gpu - f32 oracle| <= 1e-4 max(1, |ref|) at every pixel neither oracle build flags unstable_pix;
  * median depth: equal at every pixel neither build flags unstable_depth_pix;
  * radii: equal to the float32 oracle's wherever the float32 and float64 oracles agree;
  * the culled class: radius 0 and every gradient row exactly 0.0;
  * power-1 gradients: harness.check_grad_accuracy over all Gaussians and over each class's stable members;
  * power-2 gradients: relative L2 <= 1e-4 against the float32 oracle (test_backward_power_parity's bound)
    over all Gaussians and over each class's stable members.
"""
import functools

import numpy as np
import pytest

import camera_scenes as cs
from oracle import harness

pytestmark = pytest.mark.gpu

CASE_IDS = [c["name"] for c in cs.CASES]


@functools.lru_cache(maxsize=None)
def _run(name):
    """One case through the rasterizer and both oracle builds, shared by the tests of the case."""
    case = next(c for c in cs.CASES if c["name"] == name)
    scene, classes = cs.case_scene(case)
    dpix = cs.upstream_grad()
    kw = cs.run_kwargs(case)
    gpu = harness.run_gpu(scene, dpix, **kw)
    fr32, g32 = harness.run_oracle(scene, dpix, **kw)
    fr64, g64 = harness.run_oracle(scene, dpix, dtype=np.float64, error_scale=True, **kw)
    return scene, classes, gpu, fr32, g32, fr64, g64


@pytest.mark.parametrize("name", CASE_IDS)
def test_forward_outputs(cuda, name):
    scene, classes, gpu, fr32, _, fr64, _ = _run(name)
    col, ref = np.asarray(gpu["color"], np.float64), fr32.color.astype(np.float64)
    bad = (np.abs(col - ref) > 1e-4 * np.maximum(1.0, np.abs(ref))).any(axis=0)
    settled = ~(fr32.unstable_pix | fr64.unstable_pix)
    print(f"{name}: colour max |d| {np.abs(col - ref)[:, settled].max():.2e}, {int((~settled).sum())} unsettled pixels")
    assert not (bad & settled).any(), (int((bad & settled).sum()), np.argwhere(bad & settled)[:8])
    depth_ok = (np.asarray(gpu["depth"])[0] == fr32.depth[0]) | fr32.unstable_depth_pix | fr64.unstable_depth_pix
    assert depth_ok.all(), np.argwhere(~depth_ok)[:8]
    agree = fr32.radii == fr64.radii
    assert agree.mean() > 0.99
    diff = np.nonzero((gpu["radii"] != fr32.radii) & agree)[0]
    assert diff.size == 0, {n: int(m[diff].sum()) for n, m in classes.items()}


@pytest.mark.parametrize("name", CASE_IDS)
def test_culled_class_is_exactly_zero(cuda, name):
    _, classes, gpu, _, _, _, _ = _run(name)
    m = classes["culled"]
    assert (gpu["radii"][m] == 0).all(), gpu["radii"][m]
    for k, v in gpu["grads"].items():
        assert (v[m] == 0.0).all(), k
    assert (gpu["radii"][classes["near"]] > 0).all()  # in front of 0.001, behind upstream 3DGS's 0.2


@pytest.mark.parametrize("name", CASE_IDS)
def test_gradients_per_class(cuda, name):
    scene, classes, gpu, fr32, g32, fr64, g64 = _run(name)
    case = next(c for c in cs.CASES if c["name"] == name)
    grads = gpu["grads"]
    assert all(np.isfinite(v).all() for v in grads.values())
    stable = ~(fr32.unstable | fr64.unstable)
    # "all": every row in the per-tensor figures; the per-element ones leave out the near-threshold Gaussians
    subsets = [("all", stable if case.get("power", 1) == 1 else np.ones(scene.P, bool))]
    subsets += [(str(n), m & stable) for n, m in classes.items()]
    failed = {}
    if case.get("power", 1) == 1:
        for n, m in subsets:
            try:
                g, o = harness.check_grad_accuracy(grads, g32, g64, m)
            except AssertionError as e:
                g, o = e.args[0]["gpu"], e.args[0]["oracle_f32"]
                # ("rel_l2" is the figure over every row, whatever the subset: it is reported under "all")
                why = {k: [w for w in v if n == "all" or w != "rel_l2"] for k, v in e.args[0]["failed"].items()}
                if any(why.values()):
                    failed[n] = {k: v for k, v in why.items() if v}
            print(f"{name} {n}: " + ", ".join(
                f"{k} L2 {g[k]['rel_l2_stable']:.1e} ({o[k]['rel_l2_stable']:.1e}) r {g[k]['max']:.1e} ({o[k]['max']:.1e})"
                for k in g))
    else:
        for n, m in subsets:
            errs = {k: harness.rel_l2(v[m], np.asarray(g32[k]).reshape(v.shape)[m]) for k, v in grads.items()}
            print(f"{name} {n}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
            over = {k: e for k, e in errs.items() if not e <= 1e-4}
            if over:
                failed[n] = over
    assert not failed, failed
