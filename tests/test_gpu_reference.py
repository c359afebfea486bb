"""The product and the oracle against the reference's own kernels, run on the GPU (oracle/reference.py:
the reference's forward.cu / backward.cu / rasterizer_impl.cu compiled by hipcc for gfx950 -- not its nvcc
build -- behind oracle/ref_driver.cpp).  The reference is the truth; the product (its lists taken under
_C.reference_binning()), the float32 oracle and the float64 oracle are each compared with it.  Cases,
criteria and the rule for a tensor that misses 1e-4 are in tests/reference_cases.py; every figure is printed
(pytest -s; profiles/reference_parity_gpu_tests.log is such a run).

Measured on an MI355X (that log).  Discrete state: on every case num_rendered, ranges, point_list, radii,
tiles_touched and n_contrib of the product and of both oracle builds equal the reference's, with nothing
excused and no list divergence.  Values: every tensor of every run is within 1e-4 of the reference except
on the two one-tile backward edge scenes at power 3 under the constant Fisher seed, where dmeans2D (both
scenes) and dmeans3D (edge_bwd_wide_129) are sums of cubes of an antisymmetric term over a centred
footprint that cancel: the reference itself is 1.7-1.8 (dmeans2D) and 1.8e-3 (dmeans3D) relative L2 from
float64 there, the product and the float32 oracle are closer to float64 than it is (1.5-1.6 and 1.6e-3), and
the rule of tests/reference_cases.py sets their bounds to twice the reference's distance (3.4-3.5, 3.7e-3).
The same scenes under the random-sign seed, and every other run, stay at 1e-4.

The tests skip where the library is not built (no reference checkout at build time).
"""
import functools

import numpy as np
import pytest
import torch

import reference_cases as rc
from oracle import harness, reference

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not reference.available(), reason="reference library: " + reference.why_unavailable())]


@functools.lru_cache(maxsize=None)
def _reference_frame(name):
    case = rc.BY_NAME[name]
    fr, _ = harness.run_reference(case.scene(), backward=False, **case.kwargs())
    return fr


def _product_frame(case, scene, cuda):
    """The product's forward through the C ABI binding with the reference's lists: a frame dict."""
    from splatam_amd import _C
    from splatam_amd.layout import views
    kw = case.kwargs()
    c = scene.cam
    e = torch.Tensor([])
    use_sh, use_cov = kw.get("use_sh", False), kw.get("use_cov", False)
    cov = harness.cov3d_from(scene.scales, scene.rotations, 1.0).to(cuda) if use_cov else e
    with _C.reference_binning():
        out = _C.rasterize_gaussians(
            torch.tensor(kw.get("bg", (0.0, 0.0, 0.0)), dtype=torch.float32, device=cuda), scene.means3D.to(cuda),
            e if use_sh else scene.colors.to(cuda), scene.opacities.to(cuda), e if use_cov else scene.scales.to(cuda),
            e if use_cov else scene.rotations.to(cuda), float(kw.get("scale_modifier", 1.0)), cov,
            c.viewmatrix.to(cuda), c.projmatrix.to(cuda), c.tanfovx, c.tanfovy, c.H, c.W,
            scene.shs.to(cuda) if use_sh else e, scene.sh_degree if use_sh else 0, c.campos.to(cuda), False)
    n, color, radii, _, binning, img, depth = out
    v = views(img, binning, c.W, c.H, n)
    return dict(num_rendered=int(n), color=color.cpu().numpy(), depth=depth.cpu().numpy(), radii=radii.cpu().numpy(),
                n_contrib=v["n_contrib"].cpu().numpy().reshape(c.H, c.W), ranges=v["ranges"].cpu().numpy(),
                point_list=v["point_list"].cpu().numpy())


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_forward_state(cuda, name):
    """Discrete state and images of the product and both oracle builds against the reference's."""
    case = rc.BY_NAME[name]
    scene, fr32, fr64 = rc.oracle_frames(name)
    ref = rc.frame_dict(_reference_frame(name))
    assert ref["num_rendered"] > 0
    fails = []
    for tag, cand, lists in (("product", _product_frame(case, scene, cuda), "exact"),
                             ("oracle32", rc.frame_dict(fr32), "exact"), ("oracle64", rc.frame_dict(fr64), "sets")):
        rep, f = rc.compare_frame(f"{name} {tag}", ref, cand, fr32, fr64, lists=lists)
        print(rep)
        fails += f
    assert not fails, fails


@pytest.mark.parametrize("name,power,seed", rc.RUNS, ids=rc.RUN_IDS)
def test_gradients(cuda, name, power, seed):
    """Every gradient tensor of the product and both oracle builds against the reference's backward (two
    runs of it: its float atomics make it non-deterministic, and the larger distance to float64 is the
    basis of any raised bound)."""
    case = rc.BY_NAME[name]
    scene, fr32, fr64 = rc.oracle_frames(name)
    d = rc.dpix(scene, seed)
    fr = _reference_frame(name)
    runs = [reference.backward(fr, d, power=power) for _ in range(2)]
    ref = runs[0]
    assert all(np.isfinite(v).all() for v in ref.values())
    v32, f32, v64 = rc.oracle_grads(name, power, seed)
    dist = rc.reference_distance(runs, v64)
    spread = {k: harness.rel_l2(runs[1][k], runs[0][k]) for k in harness.GRAD_KEYS if runs[0][k].size}
    print(f"{name} p{power} {seed}: reference to float64 " + ", ".join(f"{k} {v:.1e}" for k, v in dist.items())
          + "; two-run spread max " + f"{max(spread.values()):.1e}")
    stable = ~(fr32.unstable | fr64.unstable)
    gpu = harness.run_gpu(scene, d, device=cuda, power=power, **case.kwargs())["grads"]
    # the product has neither SH bug of the reference's fused kernel: add the oracle's own difference
    corrected = {k: v + (np.asarray(v32[k]) - np.asarray(f32[k])).reshape(v.shape) for k, v in gpu.items()}
    fails = []
    tag = f"{name} p{power} {seed}"
    for who, cand in (("product", corrected), ("oracle32", v32), ("oracle64", v64)):
        rep, f = rc.compare_grads(f"{tag} {who}", ref, dist, cand, v32, v64, stable, int(fr64.n_contrib.max()))
        print(rep)
        fails += f
    assert not fails, fails


def test_mark_visible(cuda):
    """Rasterizer::markVisible on the inputs of test_mark_visible_matches_oracle: reference, oracle, product."""
    from oracle import oracle
    from splatam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    pts, cam = rc.mark_visible_inputs()
    ref = reference.mark_visible(pts.numpy(), cam.viewmatrix.numpy(), cam.projmatrix.numpy())
    assert 0 < int(ref.sum()) < ref.size
    np.testing.assert_array_equal(oracle.mark_visible(pts.numpy(), cam.viewmatrix.numpy()), ref)
    st = GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                       bg=torch.zeros(3, device=cuda), scale_modifier=1.0,
                                       viewmatrix=cam.viewmatrix.to(cuda), projmatrix=cam.projmatrix.to(cuda),
                                       sh_degree=0, campos=cam.campos.to(cuda), prefiltered=False)
    np.testing.assert_array_equal(GaussianRasterizer(st).markVisible(pts.to(cuda)).cpu().numpy(), ref)
