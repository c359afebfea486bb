"""Parity harness: runs the same scene through the product rasterizer
(splatam_amd, HIP) and through the CPU oracle, and compares.

TEST INFRASTRUCTURE ONLY (used by tests/, __graft_entry__.smoke and bench.py's
cpu_baseline).  The product path never imports this module.
"""
from __future__ import annotations

import numpy as np
import torch

from . import oracle

GRAD_KEYS = ("dmeans2D", "dcolors", "dopacity", "dmeans3D", "dcov3D", "dsh", "dscales", "drot")


def cov3d_from(scales, rotations, mod=1.0):
    """Upper-triangle Sigma = R S^2 R^T (forward.cu:118-152) in float64 torch."""
    q = rotations.double()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s = mod * scales.double()
    S = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()


def run_oracle(scene, dL_dcolor=None, *, bg=(0.0, 0.0, 0.0), use_sh=False, use_cov=False, power=1,
               mode=oracle.UPSTREAM, dtype=np.float32, scale_modifier=1.0, backward=True, error_scale=False):
    c = scene.cam
    kw = dict(view=c.viewmatrix.numpy(), proj=c.projmatrix.numpy(), campos=c.campos.numpy(), tanfovx=c.tanfovx,
              tanfovy=c.tanfovy, H=c.H, W=c.W, bg=np.asarray(bg, dtype), scale_modifier=scale_modifier,
              dtype=dtype)
    if use_sh:
        kw.update(shs=scene.shs.numpy(), sh_degree=scene.sh_degree)
    else:
        kw.update(colors=scene.colors.numpy())
    if use_cov:
        kw.update(cov3D=cov3d_from(scene.scales, scene.rotations, 1.0).numpy())
    else:
        kw.update(scales=scene.scales.numpy(), rotations=scene.rotations.numpy())
    fr = oracle.forward(scene.means3D.numpy(), scene.opacities.numpy(), **kw)
    grads = None
    if backward:
        if dL_dcolor is None:
            dL_dcolor = np.ones((3, c.H, c.W), np.float32)
        m = mode if power == 1 else oracle.FUSED
        grads = oracle.backward(fr, np.asarray(dL_dcolor), power=power, mode=m, error_scale=error_scale)
    return fr, grads


def run_reference(scene, dL_dcolor=None, *, bg=(0.0, 0.0, 0.0), use_sh=False, use_cov=False, power=1,
                  scale_modifier=1.0, backward=True):
    """run_oracle's scene through the reference's own kernels on the GPU (oracle/reference.py; float32,
    its backward is always the fused one).  Returns (frame, grads) in run_oracle's form."""
    from . import reference
    c = scene.cam
    kw = dict(view=c.viewmatrix.numpy(), proj=c.projmatrix.numpy(), campos=c.campos.numpy(), tanfovx=c.tanfovx,
              tanfovy=c.tanfovy, H=c.H, W=c.W, bg=np.asarray(bg, np.float32), scale_modifier=scale_modifier)
    if use_sh:
        kw.update(shs=scene.shs.numpy(), sh_degree=scene.sh_degree)
    else:
        kw.update(colors=scene.colors.numpy())
    if use_cov:
        kw.update(cov3D=cov3d_from(scene.scales, scene.rotations, 1.0).numpy())
    else:
        kw.update(scales=scene.scales.numpy(), rotations=scene.rotations.numpy())
    fr = reference.forward(scene.means3D.numpy(), scene.opacities.numpy(), **kw)
    grads = None
    if backward:
        if dL_dcolor is None:
            dL_dcolor = np.ones((3, c.H, c.W), np.float32)
        grads = reference.backward(fr, np.asarray(dL_dcolor), power=power)
    return fr, grads


def run_gpu(scene, dL_dcolor=None, *, device="cuda:0", bg=(0.0, 0.0, 0.0), use_sh=False, use_cov=False, power=1,
            scale_modifier=1.0, backward=True, grads_for=None):
    """Runs the product rasterizer (splatam_amd.GaussianRasterizer) and returns numpy results.
    grads_for: names of the inputs that require grad (means3D, means2D, opacities, colors, shs, cov3D,
    scales, rotations; default all) -- the others are passed detached and get no gradient."""
    want = (lambda k: True) if grads_for is None else (lambda k: k in grads_for)  # noqa: E731
    from splatam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    c = scene.cam
    dev = torch.device(device)
    st = GaussianRasterizationSettings(
        image_height=c.H, image_width=c.W, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
        bg=torch.tensor(bg, dtype=torch.float32, device=dev), scale_modifier=scale_modifier,
        viewmatrix=c.viewmatrix.to(dev), projmatrix=c.projmatrix.to(dev), sh_degree=scene.sh_degree if use_sh else 0,
        campos=c.campos.to(dev), prefiltered=False)
    def leaf(t, name):
        return t.detach().to(dev).clone().requires_grad_(want(name))
    means3D = leaf(scene.means3D, "means3D")
    means2D = torch.zeros_like(means3D, requires_grad=want("means2D"))
    opac = leaf(scene.opacities, "opacities")
    kw = {}
    if use_sh:
        kw["shs"] = leaf(scene.shs, "shs")
    else:
        kw["colors_precomp"] = leaf(scene.colors, "colors")
    if use_cov:
        kw["cov3D_precomp"] = leaf(cov3d_from(scene.scales, scene.rotations, 1.0), "cov3D")
    else:
        kw["scales"] = leaf(scene.scales, "scales")
        kw["rotations"] = leaf(scene.rotations, "rotations")
    ras = GaussianRasterizer(st, backward_power=power)
    color, radii, depth = ras(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    out = dict(color=color.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(),
               radii=radii.cpu().numpy())
    if backward:
        if dL_dcolor is None:
            dL_dcolor = np.ones((3, c.H, c.W), np.float32)
        color.backward(torch.as_tensor(np.asarray(dL_dcolor, np.float32), device=dev))
        g = dict(dmeans3D=means3D.grad, dmeans2D=means2D.grad, dopacity=opac.grad)
        if use_sh:
            g["dsh"] = kw["shs"].grad
        else:
            g["dcolors"] = kw["colors_precomp"].grad
        if use_cov:
            g["dcov3D"] = kw["cov3D_precomp"].grad
        else:
            g["dscales"] = kw["scales"].grad
            g["drot"] = kw["rotations"].grad
        out["grads"] = {k: v.detach().cpu().numpy() for k, v in g.items() if v is not None}
    return out


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))


def compare_forward(gpu, fr, *, atol=1e-4):
    """SURVEY.md 8(c) forward criterion: |d| <= atol*max(1,|ref|) on >= 99.9 % of pixels."""
    c = np.asarray(gpu["color"], np.float64)
    r = fr.color.astype(np.float64)
    bad = np.abs(c - r) > atol * np.maximum(1.0, np.abs(r))
    pix_bad = bad.any(axis=0)
    depth_match = float((np.asarray(gpu["depth"]) == fr.depth).mean())
    return dict(frac_bad=float(pix_bad.mean()), max_abs=float(np.abs(c - r).max()),
                radii_match=float((gpu["radii"] == fr.radii).mean()), depth_match=depth_match)


def compare_grads(gpu_grads, ref_grads):
    out = {}
    for k, v in gpu_grads.items():
        ref = ref_grads[k].reshape(v.shape)
        out[k] = rel_l2(v, ref)
    return out


def binning_gpu(scene, device="cuda:0", use_sh=False):
    """num_rendered, radii and the binning state (ranges, sorted Gaussian ids, n_contrib) of the
    product forward (through the C ABI's _C binding) as numpy arrays."""
    from splatam_amd import _C
    from splatam_amd.layout import views
    c = scene.cam
    dev = torch.device(device)
    e = torch.Tensor([])
    sh = scene.shs.to(dev) if use_sh else e
    col = e if use_sh else scene.colors.to(dev)
    with _C.reference_binning():  # the reference's lists (tile culling would drop never-evaluated instances)
        out = _C.rasterize_gaussians(torch.zeros(3, device=dev), scene.means3D.to(dev), col,
                                     scene.opacities.to(dev), scene.scales.to(dev), scene.rotations.to(dev), 1.0, e,
                                     c.viewmatrix.to(dev), c.projmatrix.to(dev), c.tanfovx, c.tanfovy, c.H, c.W, sh,
                                     scene.sh_degree if use_sh else 0, c.campos.to(dev), False)
    n, color, radii, geom, binning, img, depth = out
    v = views(img, binning, c.W, c.H, n)
    res = {k: t.cpu().numpy() for k, t in v.items()}
    res.update(num_rendered=int(n), radii=radii.cpu().numpy())
    return res


def grad_accuracy(grads, ref64, stable):
    """Per gradient tensor: relative L2 error against the float64 oracle over all Gaussians and
    over the `stable` ones, and the per-element ratio r = |x - ref64| / (1e-4 |ref64| + scale)
    over the stable Gaussians (scale = ref64["scale"], oracle.backward(error_scale=True)):
    its 99.99 % quantile, maximum and the count of elements with r > 1e-3.  A tensor that is
    identically zero in float64 reports max = |x|max / (1e-5 * the largest reference gradient) * 0.1
    (so the max <= 0.1 criterion reads |x| <= 1e-5 of it) and zeros elsewhere."""
    out = {}
    mag = max(float(np.abs(ref64[k]).max()) for k in ("dmeans3D", "dscales", "dcov3D", "dcolors", "dsh")
              if k in ref64 and isinstance(ref64[k], np.ndarray) and ref64[k].size)
    for k, v in grads.items():
        if k not in ref64 or not isinstance(ref64[k], np.ndarray) or v.size == 0:
            continue
        P = v.shape[0]
        x = np.asarray(v, np.float64).reshape(P, -1)
        b = np.asarray(ref64[k], np.float64).reshape(P, -1)
        if not b.any():  # identically zero in float64 (e.g. drot of isotropic Gaussians): rounding noise only
            out[k] = dict(rel_l2=0.0, rel_l2_stable=0.0, q9999=0.0, n_over_1e3=0,
                          max=float(np.abs(x).max()) / (1e-5 * mag) * 0.1 if mag > 0 else float(np.abs(x).max()))
            continue
        s = np.asarray(ref64["scale"][k], np.float64).reshape(P, -1)
        r = (np.abs(x - b) / (1e-4 * np.abs(b) + s + 1e-30))[stable]
        out[k] = dict(rel_l2=rel_l2(x, b), rel_l2_stable=rel_l2(x[stable], b[stable]),
                      q9999=float(np.quantile(r, 0.9999)) if r.size else 0.0, max=float(r.max()) if r.size else 0.0,
                      n_over_1e3=int((r > 1e-3).sum()))
    return out


def check_grad_accuracy(gpu_grads, ref32, ref64, stable):
    """SURVEY.md 8(c) gradient criterion against float64, calibrated on the float32 restatement of
    the reference itself (a float32 implementation of this algorithm is not within 1e-4 of float64:
    the oracle's own float32 build is 1-4e-4 off in relative L2): per tensor, the product's
    relative L2 error against float64 is at most max(1e-4, 2x) the float32 oracle's, over all
    Gaussians and over the stable ones; per element (stable Gaussians, away from every alpha / T /
    clamp threshold), the 99.99 % quantile of r is at most max(2e-3, 3x) the float32 oracle's, no
    element exceeds r = 0.1, and at most max(10, 3x the oracle's) elements exceed r = 1e-3.  (r is
    relative to the element's float32 error scale; the fixed 0.1 is a tenth of it.  The worst element
    is a cancellation-dominated near-zero gradient whose r moves with any ulp of the alpha arithmetic:
    config 4's dscales[553617, 0] = -2.9e-9 at a scale of 2.9e-8 reads 0.05-0.32 across float32
    evaluation orders of forward.cu:341; the reference-order float32 oracle itself reads 0.05 on the GPU
    box's host and 0.18 in the build container -- tools/alpha_forms.py, profiles/r7_alpha_forms_cpu.txt.)
    Returns (gpu stats, oracle stats); raises AssertionError with both on failure."""
    g = grad_accuracy(gpu_grads, ref64, stable)
    o = grad_accuracy({k: ref32[k].reshape(v.shape) for k, v in gpu_grads.items() if k in ref32}, ref64, stable)
    bad = {}
    for k, a in g.items():
        b = o[k]
        why = []
        if a["rel_l2"] > max(1e-4, 2 * b["rel_l2"]):
            why.append("rel_l2")
        if a["rel_l2_stable"] > max(1e-4, 2 * b["rel_l2_stable"]):
            why.append("rel_l2_stable")
        if a["q9999"] > max(2e-3, 3 * b["q9999"]):
            why.append("q9999")
        if a["max"] > 0.1:
            why.append("max")
        if a["n_over_1e3"] > max(10, 3 * b["n_over_1e3"]):
            why.append("n_over_1e3")
        if why:
            bad[k] = why
    assert not bad, dict(failed=bad, gpu=g, oracle_f32=o)
    return g, o


def unstable_grad_stats(gpu_grads, ref32, ref64, unstable):
    """The Gaussians check_grad_accuracy excludes (a pair of theirs sits near an alpha / T
    decision, so a float32 implementation may legitimately include or drop it): per gradient
    tensor, relative L2 error against float64 over that subset and the 99 % quantile of the
    per-element ratio r (as in grad_accuracy), for the product and for the float32 oracle.
    Returns {tensor: dict(gpu_rel_l2, f32_rel_l2, gpu_q99, f32_q99)}."""
    out = {}
    if not unstable.any():
        return out
    for k, v in gpu_grads.items():
        if k not in ref64 or k not in ref32 or not isinstance(ref64[k], np.ndarray) or v.size == 0:
            continue
        P = v.shape[0]
        x = np.asarray(v, np.float64).reshape(P, -1)[unstable]
        o = np.asarray(ref32[k], np.float64).reshape(P, -1)[unstable]
        b = np.asarray(ref64[k], np.float64).reshape(P, -1)[unstable]
        if not b.any():
            continue
        s = np.asarray(ref64["scale"][k], np.float64).reshape(P, -1)[unstable]
        den = 1e-4 * np.abs(b) + s + 1e-30
        out[k] = dict(gpu_rel_l2=rel_l2(x, b), f32_rel_l2=rel_l2(o, b),
                      gpu_q99=float(np.quantile(np.abs(x - b) / den, 0.99)),
                      f32_q99=float(np.quantile(np.abs(o - b) / den, 0.99)))
    return out
