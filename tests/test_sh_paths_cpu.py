"""The oracle pinned with the active SH degree D and the stored coefficient count M unequal, and at degree 0
with SH input, on the scenes of tests/sh_scenes.py -- before tests/test_gpu_sh_paths.py holds the rasterizer's
per-lane SH path to it.

  * NaN padding changes nothing: the float64 oracle's forward and backward on the padded scene equal the
    unpadded scene's bit for bit (colour, depth, radii, clamp bits, every non-SH gradient, dsh[:, :(D+1)^2]),
    dsh[:, (D+1)^2:] is exactly 0.0 and nothing is non-finite -- at power 1 for every pair of sh_scenes.PAIRS,
    and at power 2 (fused mode) for (1, 16) and (3, 25);
  * the float64 oracle's backward equals torch.autograd through dense_ref.render_dense on the padded scene,
    over all rows and over each class's rows (image 1e-12, gradients 1e-6: the criteria of
    tests/test_camera_scenes_cpu.py), the sh_clamp class reporting its designed clamp bits.  Power 2 has no
    autograd form at this size (tests/test_oracle_cpu.py squares per-pixel gradients of a 32x16 image), so, as
    tests/test_camera_scenes_cpu.py does for its power-2 cases, it is pinned through the stability caps, the
    bitwise equality above, and the fused decomposition agreeing with the upstream one at power 1;
  * the same two checks on degree0 with M = 1;
  * the near-threshold caps of tests/test_camera_scenes_cpu.py on every scene used here;
  * every edge_scene has the visible and culled rows the GPU tests rely on (float32 oracle), for every degree.
"""
import functools

import numpy as np
import pytest

import camera_scenes as cs
import sh_scenes as ss
from oracle import harness, oracle
from test_camera_scenes_cpu import _dense_grads

NON_SH = ("dmeans3D", "dmeans2D", "dopacity", "dcolors", "dcov3D", "dscales", "drot")
POWER2_PAIRS = ((1, 16), (3, 25))
ALL_CASES = ss.PAIRS + ((0, 1),)
ALL_IDS = ss.PAIR_IDS + ["D0_M1"]
CASE = dict(sh=1, mod=1.0, aniso=True)  # what _dense_grads / camera_scenes.run_kwargs read: SH colours, modifier 1


@functools.lru_cache(maxsize=None)
def _oracle(D, M, f64=True, power=1):
    scene, _ = ss.posed(D, M)
    dpix = ss.upstream_grad()
    return harness.run_oracle(scene, dpix.astype(np.float64) if f64 else dpix, use_sh=True, power=power,
                              dtype=np.float64 if f64 else np.float32)


def _same_as_unpadded(D, M, power):
    n = ss.nsh(D)
    scene, _ = ss.posed(D, M)
    assert scene.shs.shape == (scene.P, M, 3) and scene.sh_degree == D
    assert M == n or bool(scene.shs[:, n:].isnan().all())
    fp, gp = _oracle(D, M, True, power)
    fu, gu = _oracle(D, n, True, power)
    for k in ("color", "depth", "radii", "clamped", "tiles_touched", "rgb", "final_T", "n_contrib", "point_list"):
        a, b = getattr(fp, k), getattr(fu, k)
        assert np.isfinite(a).all(), k
        np.testing.assert_array_equal(a, b, err_msg=k)
    for k in NON_SH:
        assert np.isfinite(gp[k]).all(), k
        np.testing.assert_array_equal(gp[k], gu[k], err_msg=k)
    assert gp["dsh"].shape == (scene.P, M, 3) and np.isfinite(gp["dsh"]).all()
    np.testing.assert_array_equal(gp["dsh"][:, :n], gu["dsh"])
    assert (gp["dsh"][:, n:] == 0.0).all()
    assert np.abs(gp["dsh"][:, :n]).sum() > 0 and np.abs(gp["dmeans3D"]).sum() > 0


@pytest.mark.parametrize("D,M", ss.PAIRS, ids=ss.PAIR_IDS)
def test_nan_padding_changes_no_bit(D, M):
    _same_as_unpadded(D, M, 1)


@pytest.mark.parametrize("D,M", POWER2_PAIRS)
def test_nan_padding_changes_no_bit_power2(D, M):
    _same_as_unpadded(D, M, 2)
    # fused mode itself, on the padded scene: its power-1 decomposition is the upstream one (which the autograd
    # test below pins), tests/test_oracle_cpu.py::test_upstream_and_fused_agree_at_power_1's bound
    fr, up = _oracle(D, M, True, 1)
    fu = oracle.backward(fr, ss.upstream_grad().astype(np.float64), power=1, mode=oracle.FUSED)
    for k in harness.GRAD_KEYS:
        assert np.linalg.norm(up[k] - fu[k]) <= 1e-10 * max(np.linalg.norm(up[k]), 1.0), k
    assert (fu["dsh"][:, ss.nsh(D):] == 0.0).all()


def test_big_padding_is_the_same_scene():
    """poison="big" differs from "nan" in the tail alone (the GPU test renders both and wants equal bits)."""
    for D, M in ss.PAIRS:
        a, b = ss.posed(D, M, "nan")[0], ss.posed(D, M, "big")[0]
        n = ss.nsh(D)
        assert bool((a.shs[:, :n] == b.shs[:, :n]).all()) and bool((b.shs[:, n:].abs() == 1e30).all())
        assert bool((b.shs[:, n:] > 0).any()) and bool((b.shs[:, n:] < 0).any())
        for k in ("means3D", "scales", "rotations", "opacities"):
            assert getattr(a, k) is getattr(b, k)


@pytest.mark.parametrize("D,M", ALL_CASES, ids=ALL_IDS)
def test_oracle_backward_matches_autograd_per_class(D, M):
    scene, classes = ss.posed(D, M)
    n = ss.nsh(D)
    fr, g = _oracle(D, M)
    assert set(classes) == {"body", "clamp_x", "clamp_y", "clamp_xy", "edge_in", "near", "culled", "opaque", "sh_clamp"}
    m = classes["sh_clamp"]
    assert (fr.radii[m] > 0).all()
    np.testing.assert_array_equal(fr.clamped[m].astype(bool), cs.sh_clamp_bits(classes))
    rows = np.abs(g["dsh"].reshape(scene.P, -1)).sum(1)
    np.testing.assert_array_equal(rows[m] == 0, cs.sh_clamp_bits(classes).all(1))
    img, d = _dense_grads(scene, fr, ss.upstream_grad(), CASE)
    assert np.abs(img - fr.color).max() < 1e-12
    assert d["dsh"].shape == (scene.P, M, 3) and (d["dsh"][:, n:] == 0.0).all()  # autograd: unused coefficients
    bad = {}
    for k, v in d.items():
        ref = g[k].reshape(v.shape)
        assert np.isfinite(ref).all() and np.abs(v).sum() > 0, k
        for name, mask in [("all", np.ones(scene.P, bool))] + list(classes.items()):
            err = np.linalg.norm(ref[mask] - v[mask]) / max(np.linalg.norm(v[mask]), 1e-30)
            if np.linalg.norm(v[mask]) == 0:  # the culled class: exactly zero
                err = np.abs(ref[mask]).max()
            if not err < 1e-6:
                bad[(k, name)] = err
    assert not bad, bad


def test_degree0_scene():
    """degree0: one coefficient per Gaussian, the colour it was built from, and the sh_clamp members at least
    0.05 from zero on the designed side."""
    scene, classes = ss.posed(0)
    assert scene.shs.shape == (scene.P, 1, 3) and scene.sh_degree == 0
    colour = cs.SH_C0 * scene.shs[:, 0].double().numpy() + 0.5
    m = classes["sh_clamp"]
    bits = cs.sh_clamp_bits(classes)
    np.testing.assert_array_equal(colour[m] < 0, bits)
    assert np.abs(colour[m]).min() >= 0.05 - 1e-6 and colour[m].max() <= 0.55 + 1e-6 and colour[m].min() >= -0.35 - 1e-6
    assert np.abs(colour[~m] - scene.colors.double().numpy()[~m]).max() < 1e-6
    fr, _ = _oracle(0, 1)
    np.testing.assert_array_equal(fr.clamped[m].astype(bool), bits)
    _same_as_unpadded(0, 1, 1)  # (trivially itself: the finiteness and non-zero checks)


@pytest.mark.parametrize("D,M,power", [(d, m, 1) for d, m in ALL_CASES] + [(d, m, 2) for d, m in POWER2_PAIRS] +
                         [(0, 16, 3)])
def test_stability_caps(D, M, power):
    """tests/test_camera_scenes_cpu.py::test_stability_caps on the scenes of this module (the unstable sets do
    not depend on the backward's power; the cases are those tests/test_gpu_sh_paths.py runs)."""
    _, classes = ss.posed(D, M)
    fr32, _ = _oracle(D, M, False)
    fr64, _ = _oracle(D, M, True)
    unstable = fr32.unstable | fr64.unstable
    for name, m in classes.items():
        assert unstable[m].sum() <= 0.1 * m.sum(), (name, int(unstable[m].sum()), int(m.sum()))
        assert (m & ~unstable).sum() >= 8, name
    npix = cs.W * cs.H
    assert (fr32.unstable_pix | fr64.unstable_pix).sum() <= 0.02 * npix
    assert (fr32.unstable_depth_pix | fr64.unstable_depth_pix).sum() <= 0.02 * npix


@pytest.mark.parametrize("P", ss.EDGE_P)
def test_edge_scenes_have_visible_and_culled_rows(P):
    assert set(ss.EDGE_SEEDS) == set(ss.EDGE_P)
    dpix = ss.upstream_grad()
    for D in range(4):
        scene = ss.edge_scene(P, D)
        assert scene.P == P and scene.sh_degree == D and scene.shs.shape == (P, ss.nsh(D), 3)
        fr, g = harness.run_oracle(scene, dpix, use_sh=True)
        f64, _ = harness.run_oracle(scene, dpix, use_sh=True, dtype=np.float64, backward=False)
        assert (fr.radii > 0).sum() >= 1
        np.testing.assert_array_equal(fr.radii == 0, ss.culled_rows(P))
        assert P < 63 or (fr.radii == 0).sum() >= 1
        assert (fr.color != 0).any() and np.abs(g["dsh"]).sum() > 0
        # how EDGE_SEEDS was chosen: nothing near a threshold, so every pixel and every row is compared
        assert not (fr.unstable | f64.unstable).any()
        assert not (fr.unstable_pix | f64.unstable_pix | fr.unstable_depth_pix | f64.unstable_depth_pix).any()
        np.testing.assert_array_equal(fr.radii, f64.radii)
