"""The rasterizer's tile pipeline on its exact edges, on constructed scenes (tests/edge_scenes.py; the CPU
checks of the construction are in tests/test_edge_scenes_cpu.py): the per-tile sort's branch lengths and
chunk write-back, the forward's 256-entry batches, and the render backward's batch and slot-budget cuts in
every variant with a budget of its own.  No scene has a pair or a transmittance near a threshold, so every
pixel and every Gaussian is compared: nothing is excluded as unstable."""
import contextlib
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import edge_scenes as es
from oracle import harness, oracle

pytestmark = pytest.mark.gpu


def _forward(scene, cuda, *, reference=False, use_sh=False, colors=None):
    """The dynamic forward through the C ABI binding: outputs and the binning / image state as numpy."""
    from splatam_amd import _C
    from splatam_amd.layout import views
    c = scene.cam
    e = torch.Tensor([])
    col = e if use_sh else (scene.colors if colors is None else colors).to(cuda)
    sh = scene.shs.to(cuda) if use_sh else e
    with (_C.reference_binning() if reference else contextlib.nullcontext()):
        out = _C.rasterize_gaussians(torch.zeros(3, device=cuda), scene.means3D.to(cuda), col,
                                     scene.opacities.to(cuda), scene.scales.to(cuda), scene.rotations.to(cuda), 1.0, e,
                                     c.viewmatrix.to(cuda), c.projmatrix.to(cuda), c.tanfovx, c.tanfovy, c.H, c.W, sh,
                                     scene.sh_degree if use_sh else 0, c.campos.to(cuda), False)
    n, color, radii, geom, binning, img, depth = out
    res = {k: t.cpu().numpy() for k, t in views(img, binning, c.W, c.H, n).items() if t is not None}
    res.update(n=int(n), color=color.cpu().numpy(), depth=depth.cpu().numpy(), radii=radii.cpu().numpy())
    res["final_T"] = res["final_T"].reshape(c.H, c.W)
    res["n_contrib"] = res["n_contrib"].reshape(c.H, c.W)
    return res


def _dual(scene, colors2, cuda, capacity=0, status=None):
    from splatam_amd import _C
    c = scene.cam
    e = torch.Tensor([])
    return _C.rasterize_gaussians_dual(torch.zeros(3, device=cuda), scene.means3D.to(cuda), scene.colors.to(cuda),
                                       colors2.to(cuda), scene.opacities.to(cuda), scene.scales.to(cuda),
                                       scene.rotations.to(cuda), 1.0, e, c.viewmatrix.to(cuda), c.projmatrix.to(cuda),
                                       c.tanfovx, c.tanfovy, c.H, c.W, e, 0, c.campos.to(cuda), False,
                                       capacity=capacity, status=status)


def _dual_static_into(scene, colors2, cuda, capacity, status, fill):
    """gsr_forward_dual_static called as the binding calls it, but into outputs prefilled with `fill`."""
    from splatam_amd import _C
    c = scene.cam
    dev = torch.device(cuda)
    e = torch.Tensor([])
    with torch.cuda.device(dev):
        st, keep_s = _C._settings(torch.zeros(3, device=dev), c.viewmatrix.to(dev), c.projmatrix.to(dev),
                                  c.campos.to(dev), c.tanfovx, c.tanfovy, c.H, c.W, 1.0, 0, False, dev)
        g, keep_g, _ = _C._gaussians(scene.means3D.to(dev), e, scene.colors.to(dev), scene.opacities.to(dev),
                                     scene.scales.to(dev), scene.rotations.to(dev), e, dev)
        c2 = colors2.to(dev).contiguous()
        outs = [torch.full((k, c.H, c.W), fill, dtype=torch.float32, device=dev) for k in (3, 3, 1)]
        radii = torch.zeros(scene.P, dtype=torch.int32, device=dev)
        _C._begin(dev)
        n = _C.lib.gsr_forward_dual_static(ctypes.byref(st), ctypes.byref(g), c2.data_ptr(), int(capacity),
                                           status.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                           outs[2].data_ptr(), radii.data_ptr(), _C._ALLOC_CB, None, _C._stream(dev))
        _C._check(n, "gsr_forward_dual_static")
        torch.cuda.synchronize()
        del keep_s, keep_g
    return outs


def _colors2(scene):
    z = scene.means3D[:, 2:3]
    return torch.cat([z, torch.ones_like(z), z * z], 1)  # SplaTAM's [z, 1, z^2]


# ------------------------------------------------------------------------------- a. sort edges --
SORT_CASES = ([("one", L, "random") for L in es.SORT_LENGTHS] +
              [("one", L, o) for L in es.SORT_ORDER_LENGTHS for o in es.ORDERS if o != "random"] +
              [("layout", lay, "random") for lay in es.SORT_LAYOUTS])


@pytest.mark.parametrize("kind,L,order", SORT_CASES, ids=[f"{k}-{L}-{o}" for k, L, o in SORT_CASES])
def test_sort_edges(cuda, kind, L, order):
    """Lists of exactly the lengths at which tile_sort_bucket changes path (1 | 256 | 512 | 1024 keys, 2-4
    chunks written back in place and merged by rank, the radix fallback past 4096), with most depths tied so
    that the id half of the key decides, and three-tile layouts whose neighbours' keys sit right behind a
    chunk that is written back in place: num_rendered, ranges and the point list bit-exact against the
    oracle with the reference's lists; with culling (the default) the same lists, since every footprint
    reaches a block of its tile (the small classes sit at least 3 px inside it): nothing may be dropped."""
    e = es.sort_scene(L, order) if kind == "one" else es.sort_layout(L)
    fr, _ = harness.run_oracle(e.scene, backward=False)
    assert [int(b - a) for a, b in fr.ranges] == e.lengths  # the scene sits on its edge
    ref = _forward(e.scene, cuda, reference=True)
    assert ref["n"] == fr.num_rendered
    np.testing.assert_array_equal(ref["ranges"], fr.ranges)
    np.testing.assert_array_equal(ref["point_list"], fr.point_list)
    cul = _forward(e.scene, cuda)
    assert cul["n"] == fr.num_rendered
    for t, (a, b) in enumerate(fr.ranges):
        a3, b3 = (int(x) for x in cul["ranges"][t])
        full, kept = fr.point_list[a:b], cul["point_list"][a3:b3]
        sel = np.isin(full, kept)
        np.testing.assert_array_equal(full[sel], kept)
        assert sel.all()  # every footprint reaches a block of its own tile: nothing is culled
    for k in ("color", "depth", "radii"):
        assert np.array_equal(ref[k], cul[k]), k


def test_sort_cap_static_forward(cuda):
    """The static-capacity forward at the sort cap: a 4096-entry list renders bitwise the dynamic forward's
    images; a 4097-entry list is reported as include/gsr.h documents (status[2] = the longest list = 4097 >
    status[3] = 4096 = the longest the per-tile sort handles, status[0] = num_rendered within the capacity),
    never silently, and every kernel after the scan skips its work: prefilled images stay as they were."""
    for L in (4096, 4097):
        e = es.sort_scene(L)
        c2 = _colors2(e.scene)
        status = torch.zeros(4, dtype=torch.int32, device=cuda)
        out = _dual(e.scene, c2, cuda, capacity=8192, status=status)
        torch.cuda.synchronize()
        st = [int(x) for x in status.cpu()]
        assert st == [L, 0, L, es.TILE_SORT_CAP], st
        if L == 4096:
            dyn = _dual(e.scene, c2, cuda)
            assert dyn[0] == L
            for i in (1, 2, 3, 7):  # color, color2, radii, depth
                assert torch.equal(out[i], dyn[i]), i
            assert float(out[1].abs().sum()) > 0
        status.zero_()
        outs = _dual_static_into(e.scene, c2, cuda, 8192, status, 7.0)
        assert [int(x) for x in status.cpu()] == st
        if L == 4096:
            assert torch.equal(outs[0], out[1]) and torch.equal(outs[1], out[2]) and torch.equal(outs[2], out[7])
        else:
            assert all(bool((o == 7.0).all()) for o in outs)  # nothing rendered, nothing written


# ------------------------------------------------------------------------ b. forward batch edges --
FWD_CASES = [("full", L) for L in es.FWD_LENGTHS] + [("stop", n) for n in es.FWD_STOPS]


@pytest.mark.parametrize("kind,L", FWD_CASES, ids=[f"{k}-{L}" for k, L in FWD_CASES])
def test_forward_batch_edges(cuda, kind, L):
    """Lists of exactly 1, 2 and 3 staging batches (RENDER_BATCH = 256) and their neighbours, every row
    walking every entry, and stopper scenes whose last contributor sits on and next to a batch boundary
    with 100 entries behind it: n_contrib exact, RGB and final T within 1e-4 max(1, |ref|) of the float64
    oracle, median depth and radii exact -- at every pixel -- and the dual forward bitwise the single one."""
    e = es.forward_scene(L) if kind == "full" else es.forward_stop_scene(L)
    s = e.scene
    fr64, _ = harness.run_oracle(s, backward=False, dtype=np.float64)
    want_n = L if kind == "full" else e.n_contrib
    assert (fr64.n_contrib == want_n).all()
    g = _forward(s, cuda)
    np.testing.assert_array_equal(g["n_contrib"], fr64.n_contrib)
    np.testing.assert_array_equal(g["radii"], fr64.radii)
    np.testing.assert_array_equal(g["depth"], fr64.depth.astype(np.float32))
    for name, got, ref in (("rgb", g["color"], fr64.color), ("final_T", g["final_T"], fr64.final_T)):
        err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        print(f"{kind} {L}: worst {name} error {err.max():.2e} (final T in [{fr64.final_T.min():.3e}, "
              f"{fr64.final_T.max():.3e}])")
        assert err.max() <= 1e-4, (name, float(err.max()))
    c2 = _colors2(s)
    g2 = _forward(s, cuda, colors=c2)
    d = _dual(s, c2, cuda)
    assert np.array_equal(d[1].cpu().numpy(), g["color"]) and np.array_equal(d[2].cpu().numpy(), g2["color"])
    assert np.array_equal(d[3].cpu().numpy(), g["radii"]) and np.array_equal(d[7].cpu().numpy(), g["depth"])


# ------------------------------------------------------------- c. backward batch and slot edges --
def _dpix(s, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(3, s.cam.H, s.cam.W) * scale).astype(np.float32)


def _refs(s, dpix, power=1, use_sh=False):
    mode = oracle.UPSTREAM if power == 1 else oracle.FUSED
    _, r32 = harness.run_oracle(s, dpix, use_sh=use_sh, power=power, mode=mode)
    _, r64 = harness.run_oracle(s, dpix, use_sh=use_sh, power=power, mode=mode, dtype=np.float64,
                                error_scale=True)
    return r32, r64


def _sum_refs(a, b):
    """The dual variants' reference: the sum of two passes (dcolors from the first, dcolors2 = the second's)."""
    out = {}
    for k in ("dmeans3D", "dmeans2D", "dopacity", "dscales", "drot"):
        out[k] = a[k] + b[k]
    out["dcolors"], out["dcolors2"] = a["dcolors"], b["dcolors"]
    if "scale" in a:
        out["scale"] = _sum_refs(a["scale"], b["scale"])
    return out


def _run_dual(s, cuda, dpix, dpix2, tracking):
    from splatam_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians_dual
    c = s.cam
    st = GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, torch.zeros(3, device=cuda), 1.0,
                                       c.viewmatrix.to(cuda), c.projmatrix.to(cuda), 0, c.campos.to(cuda), False)
    leaf = lambda t, rg: t.detach().to(cuda).clone().requires_grad_(rg)  # noqa: E731
    m3, col2 = leaf(s.means3D, True), leaf(_colors2(s), True)
    op, col, sc, ro = (leaf(t, not tracking) for t in (s.opacities, s.colors, s.scales, s.rotations))
    m2 = torch.zeros_like(m3, requires_grad=not tracking)
    im, im2, _, _ = rasterize_gaussians_dual(m3, m2, None, col, col2, op, sc, ro, None, st,
                                             grad2_channels=1 if tracking else 3, means2D_grad_sum=not tracking)
    ((im * torch.as_tensor(dpix, device=cuda)).sum() + (im2 * torch.as_tensor(dpix2, device=cuda)).sum()).backward()
    g = dict(dmeans3D=m3.grad, dcolors2=col2.grad)
    if not tracking:
        g.update(dmeans2D=m2.grad, dopacity=op.grad, dcolors=col.grad, dscales=sc.grad, drot=ro.grad)
    return {k: v.cpu().numpy() for k, v in g.items()}


def _run_variant(variant, s, cuda):
    """(gpu gradients of two identical runs, float32 reference, float64 reference, power)."""
    if variant in ("wide_dual", "tracking"):
        dpix, dpix2 = _dpix(s, 6), _dpix(s, 7)
        if variant == "tracking":
            dpix2[1:] = 0.0  # the tracking loss reads only the depth channel
        runs = [_run_dual(s, cuda, dpix, dpix2, variant == "tracking") for _ in range(2)]
        s2 = dataclasses.replace(s, colors=_colors2(s))
        (a32, a64), (b32, b64) = _refs(s, dpix), _refs(s2, dpix2)
        return runs, _sum_refs(a32, b32), _sum_refs(a64, b64), 1
    power = {"wide": 1, "mom1": 2, "mom2": 2, "fisher": 2, "power_sh0": 3, "power_sh3": 3}[variant]
    use_sh = variant in ("mom2", "power_sh3")
    dpix = _dpix(s, 5, 1.0 if power == 1 else 0.3)
    only = ("means3D", "opacities") if variant == "fisher" else None
    runs = [harness.run_gpu(s, dpix, device=cuda, use_sh=use_sh, power=power, grads_for=only)["grads"]
            for _ in range(2)]
    r32, r64 = _refs(s, dpix, power, use_sh)
    if variant == "fisher":
        full = harness.run_gpu(s, dpix, device=cuda, power=power)["grads"]
        for k in ("dmeans3D", "dopacity"):
            r = harness.rel_l2(runs[0][k], full[k])
            print(f"fisher {k}: rel L2 against the full power path {r:.2e}")
            assert r <= 2e-6, (k, r)
    return runs, r32, r64, power


def _row_check(gpu, r32, r64, tag):
    """No row of any gradient tensor differs from float64 by more than the larger of 1e-3 of the row's norm
    and 3 x the float32 oracle's own error on that row.  Returns the worst ratio error / bound."""
    worst = {}
    for k, v in gpu.items():
        P = v.shape[0]
        x = np.asarray(v, np.float64).reshape(P, -1)
        b = np.asarray(r64[k], np.float64).reshape(P, -1)
        o = np.asarray(r32[k], np.float64).reshape(P, -1)
        if not b.any():  # identically zero in float64 (drot of isotropic Gaussians): rounding noise only
            continue
        err = np.linalg.norm(x - b, axis=1)
        bound = np.maximum(1e-3 * np.linalg.norm(b, axis=1), 3 * np.linalg.norm(o - b, axis=1))
        zero = bound == 0
        assert not err[zero].any(), (tag, k, "a row that is exactly zero in both oracles", np.nonzero(err * zero)[0][:8])
        ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
        f32 = np.where(zero, 0.0, np.linalg.norm(o - b, axis=1) / np.where(zero, 1.0, bound))
        worst[k] = (float(ratio.max()), float(f32.max()))
        assert ratio.max() <= 1.0, (tag, k, int(ratio.argmax()), float(ratio.max()))
    return worst


BWD_CASES = [(v, n) for v in es.BUDGETS for n in es.backward_names(v)]


@pytest.mark.parametrize("variant,name", BWD_CASES, ids=[f"{v}-{n}" for v, n in BWD_CASES])
def test_backward_batch_and_slot_edges(cuda, variant, name):
    """One tile whose list puts the render backward of `variant` on a batch edge: entry counts around BB and
    2 BB, slot counts around BS and 2 BS, mixed lists whose running popcount lands exactly on BS, reaches
    BS - 1 before a 16-slot entry, is cut by slots in front of a full BB-entry batch (the re-fetch of the
    staged registers, then the normal pipeline) or leaves a last batch of one entry, and stopper scenes with
    BB / BB + 1 entries behind the last contributor.  The masks and n_contrib this forward wrote, put through
    the cut rule restated in Python, give exactly the designed batches; then every gradient against the
    float64 oracle per element, per tensor (<= 1e-4 against the float32 oracle) and per Gaussian,
    with no Gaussian excluded, and two runs bitwise equal."""
    e = es.backward_scene(variant, name)
    s = e.scene
    BB, BS = es.BUDGETS[variant]
    f = _forward(s, cuda, use_sh=s.shs is not None)
    np.testing.assert_array_equal(f["point_list"][:len(e.lists[0])], e.lists[0])
    bmax = int(f["n_contrib"].max())
    assert bmax == (e.n_contrib if e.n_contrib is not None else e.lengths[0])
    pc = [bin(int(m) & 0xFFFF).count("1") for m in f["block_masks"][:bmax][::-1]]
    assert pc == list(e.popcount[e.lists[0][:bmax][::-1]])
    assert es.cut_batches(pc, BB, BS) == e.batches, (es.cut_batches(pc, BB, BS), e.batches)

    runs, r32, r64, _ = _run_variant(variant, s, cuda)
    gpu = runs[0]
    for k in gpu:
        assert np.array_equal(gpu[k], runs[1][k]), ("not deterministic", k)
    assert all(np.isfinite(v).all() for v in gpu.values())
    tag = f"{variant} {name}"
    line = [tag + ":"]
    # per element, no Gaussian excluded (fused mode: the oracle's per-pair error scale)
    g, o = harness.check_grad_accuracy(gpu, r32, r64, np.ones(s.P, bool))
    line.append("worst r " + ", ".join(f"{k} {g[k]['max']:.1e} (f32 {o[k]['max']:.1e})" for k in g))
    errs = {k: harness.rel_l2(v, np.asarray(r32[k]).reshape(v.shape)) for k, v in gpu.items()}
    assert not {k: v for k, v in errs.items() if v > 1e-4}, errs
    worst = _row_check(gpu, r32, r64, tag)
    line.append("worst row ratio " + ", ".join(f"{k} {a:.1e} (f32 {b:.1e})" for k, (a, b) in worst.items()))
    print(" ".join(line))
    assert any(np.abs(v).sum() > 0 for v in gpu.values())
    if e.n_contrib is not None:  # entries behind every pixel's last contributor: exactly zero
        tail = e.lists[0][e.n_contrib:]
        assert len(tail) in (BB, BB + 1)
        for k, v in gpu.items():
            assert not v[tail].any(), k


@pytest.mark.parametrize("name", es.backward_names("tracking"))
def test_fused_tracking_render_on_edges(cuda, name, monkeypatch):
    """The tracking iteration's fused render (a tile's forward and backward in one workgroup) against the
    separate launches on the tracking variant's edge scenes: loss, radii and pose gradients bitwise."""
    from splatam_amd import glue
    from splatam_amd.slam import TrackingConfig, camera_settings, init_tracking_params
    e = es.backward_scene("tracking", name)
    s = e.scene
    params = init_tracking_params(s, num_frames=2, device=cuda, pose_noise=(0.0, 0.0))
    params = {k: v.to(cuda) for k, v in params.items()}
    cam = camera_settings(s.cam, cuda)
    rs = np.random.RandomState(3)
    curr = {"cam": cam, "w2c": torch.eye(4, device=cuda),
            "im": torch.as_tensor(rs.rand(3, s.cam.H, s.cam.W).astype(np.float32), device=cuda),
            "depth": torch.as_tensor(2.0 + rs.rand(1, s.cam.H, s.cam.W).astype(np.float32), device=cuda)}
    cfg = TrackingConfig(sil_thres=0.0)  # these tiles stay translucent: every pixel with a contributor counts
    seed = torch.ones((), device=cuda)
    outs = []
    for fused in (False, True):
        monkeypatch.setattr(glue, "_RENDER_FUSED", fused)
        p = dict(params)
        p["cam_unnorm_rots"] = params["cam_unnorm_rots"].detach().clone().requires_grad_(True)
        p["cam_trans"] = params["cam_trans"].detach().clone().requires_grad_(True)
        status = torch.zeros(4, dtype=torch.int32, device=cuda)
        loss, radii = glue.tracking_iteration(p, curr, 1, cfg, capacity=4096, status=status, seed=seed)
        assert (getattr(loss.grad_fn, "records", None) is not None) == fused
        torch.autograd.backward(loss, seed)
        assert [int(x) for x in status.cpu()][:3] == [s.P, 0, s.P]
        outs.append((loss.detach().clone(), radii.clone(), p["cam_unnorm_rots"].grad.clone(),
                     p["cam_trans"].grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[1][0]) > 0 and float(outs[1][3][..., 1].abs().sum()) > 0
