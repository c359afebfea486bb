"""The references pinned off the identity camera, on the constructed scenes of tests/camera_scenes.py: each
class has the property it is named for (float64 oracle), the float64 oracle's backward equals torch.autograd
through the dense formulation over all rows and over each class's rows, a rotated and translated camera
renders the rotated scene identically and rotates dL/dmeans3D (no autograd involved), and few enough
Gaussians and pixels sit near a threshold that tests/test_gpu_camera.py may compare every class."""
import functools

import numpy as np
import pytest
import torch

import camera_scenes as cs
from dense_ref import render_dense
from oracle import harness, oracle

CASE_IDS = [c["name"] for c in cs.CASES]
POWER1_IDS = [c["name"] for c in cs.POWER1_CASES]
GRAD_TENSORS = ("dmeans3D", "dmeans2D", "dopacity", "dcolors", "dsh", "dcov3D", "dscales", "drot")


@functools.lru_cache(maxsize=None)
def _oracle(name, f64, backward=True):
    case = next(c for c in cs.CASES if c["name"] == name)
    scene, _ = cs.case_scene(case)
    dpix = cs.upstream_grad()
    return harness.run_oracle(scene, dpix.astype(np.float64) if f64 else dpix, backward=backward,
                              dtype=np.float64 if f64 else np.float32, **cs.run_kwargs(case))


def _view_ratios(scene):
    """t.x/t.z, t.y/t.z and t.z of the float32 inputs (float64 arithmetic)."""
    ph = np.concatenate([scene.means3D.double().numpy(), np.ones((scene.P, 1))], 1)
    t = ph @ scene.cam.viewmatrix[0].double().numpy()
    with np.errstate(divide="ignore"):
        return t[:, 0] / t[:, 2], t[:, 1] / t[:, 2], t[:, 2]


@pytest.mark.parametrize("case", cs.POWER1_CASES, ids=POWER1_IDS)
def test_classes_land_in_their_branches(case):
    scene, classes = cs.case_scene(case)
    cam = scene.cam
    fr, g = _oracle(case["name"], True)
    assert set(classes) == {"body", "clamp_x", "clamp_y", "clamp_xy", "edge_in", "near", "culled", "opaque"} | (
        {"sh_clamp"} if case["sh"] else set())
    assert scene.P <= 400 and all(m.sum() >= 8 for m in classes.values())
    rx, ry, tz = _view_ratios(scene)
    limx, limy = cs.LIMIT * cam.tanfovx, cs.LIMIT * cam.tanfovy
    rows = {k: np.abs(g[k].reshape(scene.P, -1)).sum(1) for k in GRAD_TENSORS}
    for name, over_x, over_y in (("clamp_x", True, False), ("clamp_y", False, True), ("clamp_xy", True, True)):
        m = classes[name]
        assert ((np.abs(rx[m]) > limx) == over_x).all() and ((np.abs(ry[m]) > limy) == over_y).all(), name
        for axis, over in ((rx, over_x), (ry, over_y)):
            if over:  # both signs
                assert (axis[m] > 0).any() and (axis[m] < 0).any(), name
        assert (fr.radii[m] > 0).all() and (rows["dmeans3D"][m] > 0).all(), name
    m = classes["edge_in"]
    assert (np.abs(rx[m]) <= limx).all() and (np.abs(ry[m]) <= limy).all()
    assert ((np.abs(rx[m]) > cam.tanfovx) | (np.abs(ry[m]) > cam.tanfovy)).all()  # off screen all the same
    assert (fr.radii[m] > 0).all() and (rows["dmeans3D"][m] > 0).all()
    m = classes["near"]
    assert ((tz[m] > 0.04) & (tz[m] < 0.16)).all() and (fr.radii[m] > 0).all() and (rows["dmeans3D"][m] > 0).all()
    m = classes["culled"]
    assert (tz[m] < 0).any() and ((tz[m] > 0) & (tz[m] <= 0.001)).any() and (tz[m] > 1).any()
    assert (fr.radii[m] == 0).all() and (fr.tiles_touched[m] == 0).all()
    for k, v in rows.items():
        assert (v[m] == 0.0).all(), k
    # opaque: o G at the best pixel of each member, from the oracle's own conic and 2D mean
    ids = np.nonzero(classes["opaque"])[0]
    yy, xx = np.mgrid[0:cs.H, 0:cs.W]
    dx = fr.means2D[ids, 0, None, None] - xx[None]
    dy = fr.means2D[ids, 1, None, None] - yy[None]
    co = fr.conic_opacity[ids]
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    best = (co[:, 3, None, None] * np.exp(power)).reshape(len(ids), -1).max(1)
    o = scene.opacities.numpy()[ids, 0]
    assert sorted(set(np.round(o.astype(np.float64), 4))) == sorted(cs.OPAQUE_CYCLE)
    above = o > np.float32(0.99)
    assert above.sum() >= 8 and (best[above] > 0.99).all(), best
    # 0.99 itself cannot exceed the clamp: those members come within 1e-4 of it from below
    assert (~above).sum() >= 4 and ((best[~above] > 0.9899) & (best[~above] <= float(np.float32(0.99)))).all(), best
    assert (rows["dopacity"][ids] > 0).all()
    if case["sh"]:
        m = classes["sh_clamp"]
        assert (fr.radii[m] > 0).all()
        np.testing.assert_array_equal(fr.clamped[m].astype(bool), cs.sh_clamp_bits(classes))
        margin = np.abs(_raw_sh_colour(scene)[m])
        assert margin.min() >= 0.05 - 1e-6, margin.min()
        np.testing.assert_array_equal(rows["dsh"][m] == 0, cs.sh_clamp_bits(classes).all(1))


def _raw_sh_colour(scene):
    from dense_ref import eval_sh
    d = scene.means3D.double() - scene.cam.campos.double()[None]
    return eval_sh(scene.sh_degree, scene.shs.double(), d / d.norm(dim=1, keepdim=True)).numpy()


def _dense_grads(scene, fr, dpix, case):
    """torch.autograd through render_dense (float64).  dscales is divided by scale_modifier: render_dense
    differentiates with respect to the scale itself, the reference with respect to (modifier * scale) --
    backward.cu:455-459 forms dL_dscale as the dot products of R^T's rows with dL_dM^T's, M = S R with
    S = diag(mod * scale) (backward.cu:429-434), and never multiplies by mod."""
    c = scene.cam
    kw = cs.run_kwargs(case)
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    leaves = dict(dmeans3D=T(scene.means3D), dmeans2D=T(np.zeros((scene.P, 3))), dopacity=T(scene.opacities))
    args = {}
    if kw["use_sh"]:
        leaves["dsh"] = args["shs"] = T(scene.shs)
        args["sh_degree"] = scene.sh_degree
    else:
        leaves["dcolors"] = args["colors"] = T(scene.colors)
    if kw["use_cov"]:
        leaves["dcov3D"] = args["cov3D"] = T(harness.cov3d_from(scene.scales, scene.rotations).double())
    else:
        leaves["dscales"], leaves["drot"] = T(scene.scales), T(scene.rotations)
        args.update(scales=leaves["dscales"], rotations=leaves["drot"], scale_modifier=kw["scale_modifier"])
    img = render_dense(fr, means3D=leaves["dmeans3D"], means2D=leaves["dmeans2D"], opacities=leaves["dopacity"],
                       view=c.viewmatrix.double(), proj=c.projmatrix.double(), campos=c.campos.double(),
                       tanfovx=c.tanfovx, tanfovy=c.tanfovy, H=c.H, W=c.W,
                       bg=torch.tensor(kw["bg"], dtype=torch.float64), **args)
    (img * torch.tensor(dpix, dtype=torch.float64)).sum().backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    if "dscales" in out:
        out["dscales"] = out["dscales"] / kw["scale_modifier"]
    return img.detach().numpy(), out


@pytest.mark.parametrize("case", cs.POWER1_CASES, ids=POWER1_IDS)
def test_oracle_backward_matches_autograd_per_class(case):
    scene, classes = cs.case_scene(case)
    fr, g = _oracle(case["name"], True)
    img, d = _dense_grads(scene, fr, cs.upstream_grad(), case)
    assert np.abs(img - fr.color).max() < 1e-12
    bad = {}
    for k, v in d.items():
        ref = g[k].reshape(v.shape)
        assert np.abs(v).sum() > 0 or k == "drot" and not case["aniso"], k
        for name, m in [("all", np.ones(scene.P, bool))] + list(classes.items()):
            err = np.linalg.norm(ref[m] - v[m]) / max(np.linalg.norm(v[m]), 1e-30)
            if np.linalg.norm(v[m]) == 0:  # the culled class (and drot of isotropic Gaussians): exactly zero
                err = np.abs(ref[m]).max()
            if not err < 1e-6:
                bad[(k, name)] = err
    assert not bad, bad


def _oracle_arrays(L, w2c, backward_grad):
    """The float64 oracle on a float64 layout moved to the world frame of w2c (float64 camera)."""
    cam = cs.camera_arrays(w2c)
    fr = oracle.forward(cs.to_world(L["means"], w2c), L["opacities"], colors=L["colors"], scales=L["scales"],
                        rotations=L["rotations"], H=cs.H, W=cs.W, dtype=np.float64, **cam)
    return fr, oracle.backward(fr, backward_grad)


def test_pose_equivariance():
    """An isotropic scene with precomputed colours seen through [R|t] after p_w = R^T (p_c - t) is the scene
    seen through the identity: the same image, and dL/dp_w = (dL/dp_c) R row by row.  Everything in float64,
    camera included (a float32 rotation is orthogonal only to 6e-8)."""
    L = cs.layout(aniso=False)
    dpix = cs.upstream_grad().astype(np.float64)
    w2c = cs.pose_matrix("posed")
    R = w2c[:3, :3]
    assert len({round(abs(float(x)), 6) for x in R.ravel()}) == 9 and np.abs(R).min() > 0.05
    fi, gi = _oracle_arrays(L, cs.pose_matrix("identity"), dpix)
    fp, gp = _oracle_arrays(L, w2c, dpix)
    assert np.abs(fp.color - fi.color).max() < 1e-9
    np.testing.assert_array_equal(fp.radii, fi.radii)
    want = gi["dmeans3D"] @ R
    vis = np.abs(want).sum(1) > 0
    assert vis.sum() > 250
    err = np.linalg.norm(gp["dmeans3D"] - want, axis=1)[vis] / np.linalg.norm(want, axis=1)[vis]
    assert err.max() < 1e-7, err.max()
    assert not gp["dmeans3D"][~vis].any()
    for k in ("dopacity", "dcolors"):  # scalars of the camera frame: unchanged
        assert harness.rel_l2(gp[k], gi[k]) < 1e-9, k
    # (the three scale axes are world axes, so only their sum -- the gradient of the common radius -- is)
    assert harness.rel_l2(gp["dscales"].sum(1), gi["dscales"].sum(1)) < 1e-9


@pytest.mark.parametrize("case", cs.CASES, ids=CASE_IDS)
def test_stability_caps(case):
    """Conditions on the inputs (where a case misses one, Gaussians move: camera_scenes.SEED)."""
    _, classes = cs.case_scene(case)
    fr32, _ = _oracle(case["name"], False)
    fr64, _ = _oracle(case["name"], True)
    unstable = fr32.unstable | fr64.unstable
    for name, m in classes.items():
        assert unstable[m].sum() <= 0.1 * m.sum(), (name, int(unstable[m].sum()), int(m.sum()))
        assert (m & ~unstable).sum() >= 8, name
    npix = cs.W * cs.H
    assert (fr32.unstable_pix | fr64.unstable_pix).sum() <= 0.02 * npix
    assert (fr32.unstable_depth_pix | fr64.unstable_depth_pix).sum() <= 0.02 * npix
