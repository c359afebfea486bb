"""The RGB render's own means2D gradient from ONE dual rasterization (gsr_backward_dual_m2d, the render
backward's M2D1 variant), the densification statistics kernel (gsr_accumulate_mean2d) and the fused mapping
frame with Gaussian-splatting densification (slam.map_frame_fused) against the literal one.

Scenes: a 3000-Gaussian map on a ragged 52 x 40 image (tile lists of ~250 entries: the two accumulators cross
batch boundaries; some Gaussians behind the camera: radius 0), with and without a background, and the one-tile
edge scenes whose lists are cut by the slot budget (tests/edge_scenes.py, the wide dual variant's budgets,
which the M2D1 variant shares)."""
import dataclasses

import numpy as np
import pytest
import torch

import edge_scenes as es
import test_gpu_prune as tp
from oracle import harness
from splatam_amd import slam, surgery
from splatam_amd.glue import accumulate_mean2d
from splatam_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians_dual
from splatam_amd.scenes import make_scene

pytestmark = pytest.mark.gpu
OTHERS = ("dmeans3D", "dopacity", "dcolors", "dcolors2", "dscales", "drot")


def _ragged_scene():
    s = make_scene(3000, 52, 40, seed=21, anisotropic=True)
    m = s.means3D.clone()
    m[::37, 2] = -1.0  # behind the camera: radius 0, no instances
    return dataclasses.replace(s, means3D=m)


def _colors2(s):
    z = s.means3D[:, 2:3]
    return torch.cat([z, torch.ones_like(z), z * z], 1)


def _dpix(s, seed):
    return (np.random.RandomState(seed).randn(3, s.cam.H, s.cam.W)).astype(np.float32)


def _dual(s, cuda, dpix, dpix2, mode, bg=(0.0, 0.0, 0.0), alive=None):
    """Every gradient of one dual rasterization in the mapping form; mode: 'color1', 'sum' or None (means2D)."""
    c = s.cam
    st = GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, torch.tensor(bg, device=cuda), 1.0,
                                       c.viewmatrix.to(cuda), c.projmatrix.to(cuda), 0, c.campos.to(cuda), False)
    leaf = lambda t: t.detach().to(cuda).clone().requires_grad_(True)  # noqa: E731
    m3, col, col2, op, sc, ro = (leaf(t) for t in (s.means3D, s.colors, _colors2(s), s.opacities, s.scales,
                                                   s.rotations))
    m2 = torch.zeros_like(m3, requires_grad=True)
    kw = {}
    if alive is not None:
        kw = dict(capacity=1 << 20, status=torch.zeros(4, dtype=torch.int32, device=cuda), alive=alive)
    im, im2, radii, _ = rasterize_gaussians_dual(m3, m2, None, col, col2, op, sc, ro, None, st, grad2_channels=1,
                                                 means2D_grad_sum=mode == "sum", means2D_grad_color1=mode == "color1",
                                                 **kw)
    ((im * torch.as_tensor(dpix, device=cuda)).sum() + (im2 * torch.as_tensor(dpix2, device=cuda)).sum()).backward()
    g = dict(dmeans3D=m3.grad, dopacity=op.grad, dcolors=col.grad, dcolors2=col2.grad, dscales=sc.grad, drot=ro.grad)
    if mode is not None:
        g["dmeans2D"] = m2.grad
    else:
        assert m2.grad is None
    out = {k: v.cpu().numpy() for k, v in g.items()}
    out["radii"] = radii.cpu().numpy()
    return out


def _depth_grad(s, seed):
    d = _dpix(s, seed)
    d[1:] = 0.0  # the mapping loss differentiates the depth channel only
    return d


CASES = {"ragged": (_ragged_scene, (0.0, 0.0, 0.0)), "ragged_bg": (_ragged_scene, (0.3, 0.6, 0.1)),
         "slots_25": (lambda: es.backward_scene("wide_dual", "slots_25").scene, (0.0, 0.0, 0.0)),
         "mixed_refetch": (lambda: es.backward_scene("wide_dual", "mixed_refetch").scene, (0.2, 0.1, 0.4))}
_cache = {}


def _case(name, cuda):
    """(scene, bg, dpix, dpix2, the color1 run, the float32 oracle's and the two-call path's dmeans2D): once."""
    if name not in _cache:
        make, bg = CASES[name]
        s = make()
        dpix, dpix2 = _dpix(s, 6), _depth_grad(s, 7)
        run = _dual(s, cuda, dpix, dpix2, "color1", bg)
        _, r32 = harness.run_oracle(s, dpix, bg=bg)
        two = harness.run_gpu(s, dpix, device=cuda, bg=bg)["grads"]["dmeans2D"]
        _cache[name] = (s, bg, dpix, dpix2, run, np.asarray(r32["dmeans2D"]).reshape(s.P, -1), two)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_color1_gradient_against_the_float32_oracle(cuda, name):
    """dmeans2D_color1 against a single RGB pass of the float32 oracle with the same dL/dpix: relative L2 <= 1e-4
    (the standing gradient tolerance), z exactly 0, radius-0 rows exactly 0."""
    s, _, _, _, run, ref, _ = _case(name, cuda)
    got = run["dmeans2D"]
    assert np.isfinite(got).all() and np.abs(got[:, :2]).sum() > 0
    rel = harness.rel_l2(got[:, :2], ref[:, :2])
    print(f"{name}: dmeans2D_color1 against the float32 oracle, rel L2 {rel:.2e}")
    assert rel <= 1e-4, rel
    assert not got[:, 2].any()
    assert not got[run["radii"] == 0].any()
    if name.startswith("ragged"):
        assert (run["radii"] == 0).sum() >= 80


@pytest.mark.parametrize("name", list(CASES))
def test_color1_gradient_against_the_two_call_path(cuda, name):
    """... and against means2D.grad of a GaussianRasterizer call on the RGB colours alone (the two-call path the
    literal loop takes): the recurrence is written in the single-image variant's operation order, the batches, the
    row reduction's tree, the block order and the per-Gaussian sum are the same, so the result is bitwise equal."""
    _, _, _, _, run, _, two = _case(name, cuda)
    rel = harness.rel_l2(run["dmeans2D"], two)
    print(f"{name}: dmeans2D_color1 against the two-call path, rel L2 {rel:.2e}, "
          f"bitwise {np.array_equal(run['dmeans2D'], two)}")
    assert rel <= 1e-4, rel
    assert np.array_equal(run["dmeans2D"], two)


@pytest.mark.parametrize("name", ["ragged_bg", "mixed_refetch"])
def test_zero_first_gradient_gives_exact_zero(cuda, name):
    """dL/dpix == 0 with a non-zero dL/dpix2: the first colour set's share is exactly zero everywhere (a shared
    accumulator would leak the depth render's share)."""
    s, bg, dpix, dpix2, _, _, _ = _case(name, cuda)
    run = _dual(s, cuda, np.zeros_like(dpix), dpix2, "color1", bg)
    assert not run["dmeans2D"].any()
    assert np.abs(run["dmeans3D"]).sum() > 0  # (the depth render's gradient did flow)


@pytest.mark.parametrize("name", ["ragged_bg", "slots_25"])
def test_zero_second_gradient_equals_the_sum(cuda, name):
    """dL/dpix2 == 0: the first set's share is the whole means2D gradient -- the means2D_grad_sum output, within
    the oracle bound (the sum's accumulator adds the second set's zero products in another order)."""
    s, bg, dpix, dpix2, _, _, _ = _case(name, cuda)
    z = np.zeros_like(dpix2)
    a, b = _dual(s, cuda, dpix, z, "color1", bg), _dual(s, cuda, dpix, z, "sum", bg)
    rel = harness.rel_l2(a["dmeans2D"], b["dmeans2D"])
    print(f"{name}: color1 against the sum with dL/dpix2 = 0, rel L2 {rel:.2e}")
    assert rel <= 1e-4, rel


@pytest.mark.parametrize("name", list(CASES))
def test_other_gradients_bitwise_those_of_the_existing_dual_backward(cuda, name):
    """means3D, opacity, both colour sets, scales and rotations: bit for bit gsr_backward_dual's, with and without
    its means2D sum -- the extra accumulator and sums move nothing."""
    s, bg, dpix, dpix2, run, _, _ = _case(name, cuda)
    for mode in (None, "sum"):
        base = _dual(s, cuda, dpix, dpix2, mode, bg)
        for k in OTHERS:
            assert np.array_equal(run[k], base[k]), (mode, k)
        assert np.array_equal(run["radii"], base["radii"])


def test_alive_mask_rows_are_zero_and_the_rest_the_compacted_set(cuda):
    """Static forward with an alive mask: culled rows get zeros; the others the gradient of the compacted map."""
    s, bg, dpix, dpix2, _, _, _ = _case("ragged_bg", cuda)
    keep = torch.ones(s.P, dtype=torch.bool)
    keep[5::11] = False
    run = _dual(s, cuda, dpix, dpix2, "color1", bg, alive=keep.to(torch.uint8).to(cuda))
    sub = dataclasses.replace(s, **{k: getattr(s, k)[keep] for k in ("means3D", "scales", "rotations", "opacities",
                                                                      "colors")})
    ref = _dual(sub, cuda, dpix, dpix2, "color1", bg)
    dead = ~keep.numpy()
    assert not run["dmeans2D"][dead].any() and not run["radii"][dead].any()
    assert np.array_equal(run["dmeans2D"][~dead], ref["dmeans2D"])


def test_statistics_kernel_against_float64(cuda):
    """gsr_accumulate_mean2d on random gradients with zeros, denormals and radius-0 rows, over more than one
    workgroup and a ragged tail.  One accumulation from zero: two squares, an add and a square root, each
    correctly rounded, stay under 2 ulp = 2^-22 relative; a denormal result cannot be closer than the format's
    spacing there, 2^-149, which the bound adds.  denom and max_2D_radius exact, untouched rows byte-identical."""
    P = 5003
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(P, 3, generator=g) * torch.exp(8 * torch.randn(P, 1, generator=g))
    grad[::7, :2] = 0.0
    grad[1::7, 0] = 0.0
    grad[2::13, :2] = torch.randn(len(grad[2::13]), 2, generator=g) * 1e-41      # denormal inputs
    grad[3::13, :2] = torch.randn(len(grad[3::13]), 2, generator=g) * 3e-23      # squares underflow to denormals
    radii = torch.randint(0, 40, (P,), generator=g, dtype=torch.int32)
    radii[::5] = 0
    mx0 = torch.randint(0, 40, (P,), generator=g).float()
    fresh = {"means2D_gradient_accum": torch.zeros(P), "denom": torch.zeros(P), "max_2D_radius": mx0.clone()}
    v = {k: t.to(cuda) for k, t in fresh.items()}
    accumulate_mean2d(v, radii.to(cuda), grad.to(cuda))
    seen = radii > 0
    assert torch.equal(v["seen"].cpu(), seen) and 0 < int(seen.sum()) < P
    ref = torch.sqrt(grad[:, 0].double() ** 2 + grad[:, 1].double() ** 2)
    got = v["means2D_gradient_accum"].cpu().double()
    err = (got - ref).abs()[seen]
    bound = 2.0 ** -22 * ref[seen] + 2.0 ** -149
    worst = float((err / bound).max())
    print(f"statistics kernel: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    assert (ref[seen] > 0).float().mean() > 0.5 and bool((ref[seen] < 1e-38).any())
    assert torch.equal(v["denom"].cpu(), seen.float())
    assert torch.equal(v["max_2D_radius"].cpu(), torch.where(seen, torch.max(mx0, radii.float()), mx0))
    # a second accumulation on filled statistics: rows with radius 0 byte-identical, the others one rounded add
    acc1 = torch.rand(P, generator=g)
    v2 = {"means2D_gradient_accum": acc1.to(cuda), "denom": (3 * torch.ones(P)).to(cuda), "max_2D_radius": mx0.to(cuda)}
    accumulate_mean2d(v2, radii.to(cuda), grad.to(cuda))
    a2 = v2["means2D_gradient_accum"].cpu()
    assert torch.equal(a2[~seen].view(torch.int32), acc1[~seen].view(torch.int32))
    assert torch.equal(a2[seen], acc1[seen] + got.float()[seen])
    assert torch.equal(v2["denom"].cpu(), 3 + seen.float())


def _sets(accum, denom, log_scales, r, thresh):
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    big = torch.exp(log_scales).max(dim=1).values > 0.01 * r
    return (grads >= thresh) & ~big, (grads >= thresh) & big, grads


def _rows_close(a, r, tol=1e-4):
    """tests/test_gpu_mapping.py's rule for fused against literal: (fraction of rows within tol, rel L2 of those)."""
    a, r = a.double().reshape(a.shape[0], -1), r.double().reshape(r.shape[0], -1)
    rn = r.norm(dim=1)
    row = (a - r).norm(dim=1) / (rn + 1e-3 * rn.mean() + 1e-30)
    ok = row <= tol
    return float(ok.float().mean()), float((a[ok] - r[ok]).norm() / r[ok].norm())


def test_map_frame_fused_follows_the_literal_frame(cuda, monkeypatch):
    """Four mapping iterations with one densification (iteration 2) over the same keyframe draws and generator
    seed: map_frame_fused (one dual rasterization, the statistics kernel, glue.FusedAdam) against map_frame_literal
    (two GaussianRasterizer calls, accumulate_mean2d_gradient, torch.optim.Adam).  Precondition, on the literal
    path: no Gaussian's accum / denom within 1e-3 relative of grad_thresh.  Then the same clones and splits, the
    same P, and parameters by the fused-against-literal rule (>= 98 % of rows within 1e-4, those within 1e-5)."""
    scene = make_scene(3000, 64, 48, seed=5, anisotropic=False)
    params = slam.init_mapping_params(scene, num_frames=3, device=cuda)
    cam = slam.camera_settings(scene.cam, cuda)
    kfs = tp._keyframes(params, cam, cuda)
    dd = dict(start_after=2, remove_big_after=0, stop_after=2, densify_every=2, grad_thresh=2e-4,
              num_to_split_into=2, removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005,
              reset_opacities_every=3000)
    # The reference's split is defined for isotropic maps only (tests/test_gpu_prune.py), whose rotation gradient is
    # zero in exact arithmetic: with eps = 1e-15 Adam turns its rounding noise into +-lr steps of either sign on
    # either path, and the split rotates its samples by those rotations (children 3e-3 apart).  The rotation's
    # learning rate is therefore 0 here; every other group keeps the configuration's.
    lrs = dict(slam.MappingConfig().lrs, unnorm_rotations=0.0)
    cfg = slam.MappingConfig(prune_gaussians=False, use_gaussian_splatting_densification=True, densify_dict=dd,
                             lrs=lrs)
    assert slam.fused_densify_eligible(params, kfs[0], cfg) and not slam.fused_mapping_eligible(params, kfs[0], cfg)
    r = torch.max(kfs[0]["depth"]) / 3.0
    snap = {}
    real_acc, real_densify = surgery.accumulate_mean2d_gradient, surgery.densify

    def acc_spy(variables):  # the literal path accumulates inside densify: the last call before the surgery
        out = real_acc(variables)
        snap["literal"] = (variables["means2D_gradient_accum"].clone(), variables["denom"].clone())
        return out

    def densify_spy(p, variables, opt, it, d, accumulate=True):
        if not accumulate and it == 2:
            snap["fused"] = (variables["means2D_gradient_accum"].clone(), variables["denom"].clone())
        if it == 2:
            snap["scales"] = p["log_scales"].detach().clone()
        return real_densify(p, variables, opt, it, d, accumulate=accumulate)

    monkeypatch.setattr(surgery, "accumulate_mean2d_gradient", acc_spy)
    monkeypatch.setattr(surgery, "densify", densify_spy)
    runs = {}
    for name in ("literal", "fused"):
        p = slam.as_parameters(params)
        for k in ("cam_unnorm_rots", "cam_trans"):
            p[k].requires_grad_(False)  # do_ba=False: the fused glue takes a fixed camera
        variables = slam.tracking_variables(scene.P, cuda)
        variables["scene_radius"] = r
        del variables["timestep"]  # (the reference's densify does not resize it: tests/test_gpu_prune.py)
        torch.cuda.manual_seed(1234)
        frame = slam.map_frame_fused if name == "fused" else slam.map_frame_literal
        frame(p, variables, kfs, 4, cfg, rng=np.random.RandomState(2))
        runs[name] = (p, _sets(*snap[name], snap["scales"], r, dd["grad_thresh"]))
    (pl, (clone_l, split_l, g_l)), (pf, (clone_f, split_f, g_f)) = runs["literal"], runs["fused"]
    near = ((g_l - dd["grad_thresh"]).abs() <= 1e-3 * dd["grad_thresh"]).sum()
    assert int(near) == 0, "precondition: a statistic of the literal path within 1e-3 of grad_thresh"
    print(f"literal frame: {int(clone_l.sum())} clones, {int(split_l.sum())} splits of {scene.P}")
    assert int((clone_l | split_l).sum()) > 0
    assert torch.equal(clone_l, clone_f) and torch.equal(split_l, split_f)
    assert pl["means3D"].shape[0] == pf["means3D"].shape[0] != scene.P
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        frac, rel = _rows_close(pf[k].detach(), pl[k].detach())
        print(f"map_frame_fused against literal, {k}: {frac:.4f} of rows within 1e-4, those at {rel:.2e}")
        assert frac >= 0.98 and rel <= 1e-5, (k, frac, rel)
