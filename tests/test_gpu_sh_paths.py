"""The SH colour paths of the HIP rasterizer at every degree, coefficient count and block edge, on the scenes
of tests/sh_scenes.py (tests/test_sh_paths_cpu.py pins the oracle on them first).

a. The per-lane path (M > (D+1)^2 stored coefficients: sh_fwd inside preprocess at stride 3 M, sh_chain_bwd from
   gauss_chain, preprocess's own clamp bits, the zero-filled dsh tails of gauss_bwd, of the power-2 moments
   kernel and of gauss_bwd_power) against the oracle, class by class, with tests/test_gpu_camera.py's criteria:
   colour within 1e-4 max(1, |ref|) at every pixel neither oracle build flags, median depth equal there, radii
   equal, the culled class exactly zero, harness.check_grad_accuracy over all Gaussians and per class (powers
   2 and 3: relative L2 <= 1e-4 against the float32 oracle).  The unused coefficients are NaN: every output
   must be finite, dsh[:, (D+1)^2:] exactly 0.0, and +-1e30 in their place must give the same bits.
b. gsr_backward called directly with every gradient output prefilled with NaN (the binding's torch.empty
   often comes back zeroed, so an unwritten tail could pass (a) by luck): no NaN remains, the tail is 0.0,
   the head is (a)'s bitwise; one staged case too.
c. The staged kernels (sh_eval: 64-Gaussian blocks, sh_bwd: 256, sh_bwd_split: 128) at sh_scenes.EDGE_P for
   degrees 0..3, and from a coefficient array that is not 16-byte aligned (the scalar staging path).
d. The fused colour Adam step at every degree and at the split kernel's block edges.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sh_scenes as ss
from oracle import harness

pytestmark = pytest.mark.gpu

POWER_CASES = ((1, 16, 2), (3, 25, 2), (0, 16, 3))
POWER_IDS = [f"D{d}_M{m}_p{p}" for d, m, p in POWER_CASES]


# ------------------------------------------------------------------------------ a. the per-lane path
@functools.lru_cache(maxsize=None)
def _gpu(D, M, power=1, poison="nan"):
    scene, _ = ss.posed(D, M, poison)
    assert scene.sh_degree == D and scene.shs.shape[1] == M
    return harness.run_gpu(scene, ss.upstream_grad(), use_sh=True, power=power)


@functools.lru_cache(maxsize=None)
def _ref(D, M, power=1):
    scene, classes = ss.posed(D, M)
    dpix = ss.upstream_grad()
    fr32, g32 = harness.run_oracle(scene, dpix, use_sh=True, power=power)
    fr64, g64 = harness.run_oracle(scene, dpix, use_sh=True, power=power, dtype=np.float64, error_scale=True)
    return scene, classes, fr32, g32, fr64, g64


def _finite_and_zero_tail(gpu, D):
    for k in ("color", "depth"):
        assert np.isfinite(gpu[k]).all(), k
    for k, v in gpu["grads"].items():
        assert np.isfinite(v).all(), k
    dsh = gpu["grads"]["dsh"]
    assert (dsh[:, ss.nsh(D):] == 0.0).all(), int((dsh[:, ss.nsh(D):] != 0.0).sum())
    assert np.abs(dsh[:, :ss.nsh(D)]).sum() > 0


@pytest.mark.parametrize("D,M", ss.PAIRS, ids=ss.PAIR_IDS)
def test_per_lane_forward(cuda, D, M):
    scene, classes, fr32, _, fr64, _ = _ref(D, M)
    gpu = _gpu(D, M)
    assert np.isfinite(gpu["color"]).all() and np.isfinite(gpu["depth"]).all()
    col, ref = np.asarray(gpu["color"], np.float64), fr32.color.astype(np.float64)
    bad = (np.abs(col - ref) > 1e-4 * np.maximum(1.0, np.abs(ref))).any(axis=0)
    settled = ~(fr32.unstable_pix | fr64.unstable_pix)
    print(f"D{D} M{M}: colour max |d| {np.abs(col - ref)[:, settled].max():.2e}, {int((~settled).sum())} unsettled pixels")
    assert not (bad & settled).any(), (int((bad & settled).sum()), np.argwhere(bad & settled)[:8])
    depth_ok = (np.asarray(gpu["depth"])[0] == fr32.depth[0]) | fr32.unstable_depth_pix | fr64.unstable_depth_pix
    assert depth_ok.all(), np.argwhere(~depth_ok)[:8]
    agree = fr32.radii == fr64.radii
    assert agree.mean() > 0.99
    diff = np.nonzero((gpu["radii"] != fr32.radii) & agree)[0]
    assert diff.size == 0, {n: int(m[diff].sum()) for n, m in classes.items()}
    m = classes["culled"]
    assert (gpu["radii"][m] == 0).all() and (gpu["radii"][classes["sh_clamp"]] > 0).all()
    for k, v in gpu["grads"].items():
        assert (v[m] == 0.0).all(), k


@pytest.mark.parametrize("D,M", ss.PAIRS, ids=ss.PAIR_IDS)
def test_per_lane_gradients_per_class(cuda, D, M):
    scene, classes, fr32, g32, fr64, g64 = _ref(D, M)
    grads = _gpu(D, M)["grads"]
    assert grads["dsh"].shape == (scene.P, M, 3)
    _finite_and_zero_tail(_gpu(D, M), D)
    stable = ~(fr32.unstable | fr64.unstable)
    failed = {}
    for n, m in [("all", stable)] + [(str(n), m & stable) for n, m in classes.items()]:
        try:
            g, o = harness.check_grad_accuracy(grads, g32, g64, m)
        except AssertionError as e:
            g, o = e.args[0]["gpu"], e.args[0]["oracle_f32"]
            # ("rel_l2" is the figure over every row, whatever the subset: it is reported under "all")
            why = {k: [w for w in v if n == "all" or w != "rel_l2"] for k, v in e.args[0]["failed"].items()}
            if any(why.values()):
                failed[n] = {k: v for k, v in why.items() if v}
        print(f"D{D} M{M} {n}: " + ", ".join(
            f"{k} L2 {g[k]['rel_l2_stable']:.1e} ({o[k]['rel_l2_stable']:.1e}) r {g[k]['max']:.1e} ({o[k]['max']:.1e})"
            for k in g))
    assert not failed, failed


@pytest.mark.parametrize("D,M,power", POWER_CASES, ids=POWER_IDS)
def test_per_lane_power(cuda, D, M, power):
    """Power 2: the moments kernel (ysq[k] for k >= nsh and its k >= 16 loop); power 3: gauss_bwd_power."""
    scene, classes, fr32, g32, fr64, _ = _ref(D, M, power)
    gpu = _gpu(D, M, power)
    _finite_and_zero_tail(gpu, D)
    stable = ~(fr32.unstable | fr64.unstable)
    failed = {}
    for n, m in [("all", np.ones(scene.P, bool))] + [(str(n), m & stable) for n, m in classes.items()]:
        errs = {k: harness.rel_l2(v[m], np.asarray(g32[k]).reshape(v.shape)[m]) for k, v in gpu["grads"].items()}
        print(f"D{D} M{M} power {power} {n}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        over = {k: e for k, e in errs.items() if not e <= 1e-4}
        if over:
            failed[n] = over
    assert not failed, failed


@pytest.mark.parametrize("D,M,power", [(d, m, 1) for d, m in ss.PAIRS] + list(POWER_CASES),
                         ids=[f"{i}_p1" for i in ss.PAIR_IDS] + POWER_IDS)
def test_per_lane_tail_is_never_read(cuda, D, M, power):
    """+-1e30 in the unused coefficients instead of NaN: the same bits in every output."""
    a, b = _gpu(D, M, power, "nan"), _gpu(D, M, power, "big")
    for k in ("color", "depth", "radii"):
        assert np.array_equal(a[k], b[k]), k
    assert set(a["grads"]) == set(b["grads"])
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k], b["grads"][k]), k


# ------------------------------------------------- b. the dsh tail is written, not inherited from the allocator
def _direct_backward(dev, scene, power):
    """gsr_forward, then gsr_backward into NaN-filled outputs, through ctypes (the direct-call form of
    tests/test_gpu_capi_paths.py)."""
    from splatam_amd import _C
    from splatam_amd._lib import GsrGrads, lib
    c = scene.cam
    t = lambda x: x.to(dev).contiguous()  # noqa: E731
    means, opac, scales, rots, shs = (t(x) for x in (scene.means3D, scene.opacities, scene.scales, scene.rotations,
                                                     scene.shs))
    cam = [torch.zeros(3, device=dev), t(c.viewmatrix), t(c.projmatrix), t(c.campos)]
    P, M = shs.shape[:2]
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = _C._stream(dev)
        s, keep_s = _C._settings(*cam, c.tanfovx, c.tanfovy, c.H, c.W, 1.0, scene.sh_degree, False, dev, stream)
        g, keep_g, _ = _C._gaussians(means, shs, None, opac, scales, rots, None, dev)
        assert g.M == M
        color, depth = torch.empty(3, c.H, c.W, **f32), torch.empty(1, c.H, c.W, **f32)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        _C._begin(dev)
        n = lib.gsr_forward(ctypes.byref(s), ctypes.byref(g), color.data_ptr(), depth.data_ptr(), radii.data_ptr(),
                            _C._ALLOC_CB, None, stream)
        assert n > 0, lib.gsr_last_error().decode()
        bufs = dict(_C._tls.buffers)
        shapes = dict(dmeans2D=(P, 3), dcolors=(P, 3), dopacity=(P, 1), dmeans3D=(P, 3), dcov3D=(P, 6),
                      dsh=(P, M, 3), dscales=(P, 3), drotations=(P, 4))
        out = {k: torch.full(v, float("nan"), **f32) for k, v in shapes.items()}
        grads = GsrGrads(**{k: v.data_ptr() for k, v in out.items()})
        dpix = torch.as_tensor(ss.upstream_grad(), device=dev).contiguous()
        _C._begin(dev)
        rc = lib.gsr_backward(ctypes.byref(s), ctypes.byref(g), radii.data_ptr(), dpix.data_ptr(), int(n),
                              bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), int(power),
                              ctypes.byref(grads), _C._ALLOC_CB, None, stream)
        assert rc == 0, lib.gsr_last_error().decode()
        torch.cuda.synchronize()
        _C._tls.buffers = {}
    del keep_s, keep_g
    return {k: v.cpu().numpy() for k, v in out.items()}, radii.cpu().numpy()


@pytest.mark.parametrize("D,M,power", [(1, 16, 1), (3, 25, 1), (1, 16, 2), (3, 25, 2), (3, 16, 1)])
def test_every_gradient_row_is_written(cuda, D, M, power):
    """(3, 16) is the staged case: dsh leaves sh_bwd_kernel through unstage_rows, and dL/dcolor -- which the staged
    chain routes to sh_bwd through a scratch array -- must still reach a caller who asked for it."""
    scene, _ = ss.posed(D, M)
    out, radii = _direct_backward(cuda, scene, power)
    assert (radii > 0).any() and (radii == 0).any()
    for k, v in out.items():
        assert not np.isnan(v).any(), (k, int(np.isnan(v).sum()), np.argwhere(np.isnan(v))[:4])
        assert np.isfinite(v).all(), k
        assert (v[radii == 0] == 0.0).all(), k
    n = ss.nsh(D)
    assert (out["dsh"][:, n:] == 0.0).all()
    a = _gpu(D, M, power)["grads"]
    assert np.array_equal(out["dsh"][:, :n], a["dsh"][:, :n])
    assert np.abs(out["dcolors"]).sum() > 0 and np.abs(out["dsh"][:, :n]).sum() > 0


# --------------------------------------------------------------- c. the staged kernels at their block edges
def _render(dev, scene, shs, power=1):
    """harness.run_gpu for SH colours with the coefficient tensor `shs` (a device leaf) used as it is."""
    from splatam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    c = scene.cam
    st = GaussianRasterizationSettings(
        image_height=c.H, image_width=c.W, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
        bg=torch.zeros(3, dtype=torch.float32, device=dev), scale_modifier=1.0, viewmatrix=c.viewmatrix.to(dev),
        projmatrix=c.projmatrix.to(dev), sh_degree=scene.sh_degree, campos=c.campos.to(dev), prefiltered=False)
    leaf = lambda t: t.detach().to(dev).clone().requires_grad_(True)  # noqa: E731
    means3D, opac, scales, rots = leaf(scene.means3D), leaf(scene.opacities), leaf(scene.scales), leaf(scene.rotations)
    means2D = torch.zeros_like(means3D, requires_grad=True)
    color, radii, depth = GaussianRasterizer(st, backward_power=power)(
        means3D=means3D, means2D=means2D, opacities=opac, shs=shs, scales=scales, rotations=rots)
    color.backward(torch.as_tensor(ss.upstream_grad(), device=dev))
    g = dict(dmeans3D=means3D.grad, dmeans2D=means2D.grad, dopacity=opac.grad, dsh=shs.grad, dscales=scales.grad,
             drot=rots.grad)
    return dict(color=color.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), radii=radii.cpu().numpy(),
                grads={k: v.detach().cpu().numpy() for k, v in g.items()})


def _offset_leaf(dev, t, nbytes=4):
    """A contiguous copy of `t` that starts `nbytes` into a larger allocation."""
    assert nbytes % 4 == 0
    buf = torch.empty(t.numel() + nbytes // 4 + 4, dtype=torch.float32, device=dev)
    v = buf[nbytes // 4: nbytes // 4 + t.numel()].view(t.shape)
    v.copy_(t.to(dev))
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0
    return v.requires_grad_(True)


def _same_bits(a, b):
    for k in ("color", "depth", "radii"):
        assert np.array_equal(a[k], b[k]), k
    assert set(a["grads"]) == set(b["grads"])
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("D", range(4))
@pytest.mark.parametrize("P", ss.EDGE_P)
def test_staged_block_edges(cuda, P, D):
    """M == (D+1)^2 at P below one block, at exact multiples and at each boundary +-1 of the 64-, 128- and
    256-Gaussian blocks: the full-block and ragged staging paths, float4 (D = 1, 3) and scalar (D = 0, 2).  No
    pixel or Gaussian of these scenes is near a threshold (tests/test_sh_paths_cpu.py), so every row counts."""
    scene = ss.edge_scene(P, D)
    dpix = ss.upstream_grad()
    gpu = harness.run_gpu(scene, dpix, use_sh=True)
    fr32, g32 = harness.run_oracle(scene, dpix, use_sh=True)
    _, g64 = harness.run_oracle(scene, dpix, use_sh=True, dtype=np.float64, error_scale=True)
    fwd = harness.compare_forward(gpu, fr32)
    print(f"P{P} D{D}: {fwd}")
    assert fwd["frac_bad"] <= 1e-3, fwd
    assert fwd["radii_match"] >= 0.999, fwd
    assert fwd["depth_match"] >= 0.995, fwd
    assert all(np.isfinite(v).all() for v in gpu["grads"].values())
    g, o = harness.check_grad_accuracy(gpu["grads"], g32, g64, np.ones(P, bool))
    print(f"P{P} D{D}: " + ", ".join(f"{k} L2 {g[k]['rel_l2']:.1e} ({o[k]['rel_l2']:.1e}) r {g[k]['max']:.1e}" for k in g))
    culled = gpu["radii"] == 0
    assert np.array_equal(culled, ss.culled_rows(P)) and (~culled).any()
    for k, v in gpu["grads"].items():
        assert (v[culled] == 0.0).all(), k
        if k not in ("drot", "dscales"):
            assert np.abs(v[~culled]).sum() > 0, k
    _same_bits(gpu, harness.run_gpu(scene, dpix, use_sh=True))


@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("P", (64, 129, 257))
def test_staged_misaligned_coefficients(cuda, P, D):
    """ROW % 4 == 0 but shs 4 bytes off a 16-byte boundary: stage_rows / unstage_rows take their scalar loops.
    The same values through the same sh_fwd / sh_chain_bwd, so every output equals the aligned call's bit for
    bit, dsh included."""
    scene = ss.edge_scene(P, D)
    aligned = scene.shs.to(cuda).clone().requires_grad_(True)
    assert aligned.data_ptr() % 16 == 0
    a = _render(cuda, scene, aligned)
    b = _render(cuda, scene, _offset_leaf(cuda, scene.shs))
    assert np.abs(a["grads"]["dsh"]).sum() > 0
    _same_bits(a, b)
    _same_bits(a, harness.run_gpu(scene, ss.upstream_grad(), use_sh=True))  # (_render is run_gpu)


# ------------------------------------------------------------------- d. the fused colour Adam step
ADAM_CASES = [(0, 300, False), (2, 300, False)] + [(d, p, False) for d in (1, 3) for p in (127, 128, 129, 300)] + \
    [(1, 300, True), (3, 300, True)]


@pytest.mark.parametrize("D,P,misaligned", ADAM_CASES,
                         ids=[f"D{d}_P{p}" + ("_misaligned" if m else "") for d, p, m in ADAM_CASES])
def test_sh_colour_adam_fused_bitwise_every_degree(cuda, monkeypatch, D, P, misaligned):
    """tests/test_gpu_mapping.py::test_sh_colour_adam_fused_bitwise (degree 3, P = 3000, aligned) at every
    degree: three iterations with the colour step inside the SH backward (gsr_backward_dual_sh_adam) against
    the step in gsr_map_transform_bwd_adam; parameters and both moments bitwise equal, and moved.

    Which kernel and loops a case reaches (SH_SPLIT_BLOCK = 128 lanes, ROW = 3 (D+1)^2 floats per row, U = 4
    float4 per lane in adam_rows_lds' deep loop, which a lane enters while lane + 3 * 128 < n ROW / 4, n rows
    in the block):
      D = 0, 2 (ROW = 3, 27: not float4) and the misaligned D = 1, 3: sh_bwd_kernel (256-row blocks, 300 = 256
        + 44) with adam_rows' scalar loop;
      D = 1 (ROW / 4 = 3): a full block has 384 float4, so the deep loop never runs: the tail loop only, in
        every case (P = 127: 381 float4; 129: a 1-row block, 3 float4; 300: a 44-row block, 132 float4);
      D = 3 (ROW / 4 = 12): a full block (1536 float4) runs the deep loop three times and no tail (P = 128);
        P = 127 (1524): lanes >= 116 leave the deep loop after two rounds and finish in the tail loop;
        P = 129: the 1-row block (12 float4) is tail only; P = 300: the 44-row block (528 float4) runs the
        deep loop once in every lane and the tail loop in lanes < 16.
    adam_rows' own float4 branch needs ROW % 4 == 0 and aligned pointers -- the condition under which
    launch_sh_bwd_t picks sh_bwd_split_kernel -- so no case reaches it."""
    from splatam_amd import slam
    from splatam_amd.glue import MapAdam
    from splatam_amd.scenes import make_scene
    from test_gpu_mapping import GAUSS_KEYS, _scene_targets
    scene = make_scene(P, 150, 110, seed=3, anisotropic=True, sh_degree=D)
    if D == 0:
        scene = ss.degree0(scene)
    params = slam.init_mapping_params(scene, num_frames=3, device=cuda)
    assert params["shs"].shape == (P, ss.nsh(D), 3)
    cam = slam.camera_settings(scene.cam, cuda, sh_degree=D)
    curr = _scene_targets(params, cam, cuda)
    cfg = slam.MappingConfig()
    key = slam.color_key(params)
    assert key == "shs"
    keys = GAUSS_KEYS + (key,)
    out = []
    for fused in (False, True):
        monkeypatch.setattr(slam, "_SH_ADAM_FUSED", fused)
        p = {k: v.clone() for k, v in params.items()}
        for k in keys:
            p[k].requires_grad_(True)
        if misaligned:
            p[key] = _offset_leaf(cuda, params[key])
        assert (p[key].data_ptr() % 16 != 0) == misaligned
        adam = MapAdam(p, cfg.lrs, color_key=key)
        assert all(t.data_ptr() % 16 == 0 for t in adam.exp_avg + adam.exp_avg_sq)
        for _ in range(3):
            loss, _, _ = slam.get_loss_mapping(p, curr, 1, cfg, fused=True, adam=adam)
            loss.backward()
        assert adam.step == 3
        out.append(({k: p[k].detach().clone() for k in keys}, [t.clone() for t in adam.exp_avg + adam.exp_avg_sq]))
    (p0, s0), (p1, s1) = out
    for k in keys:
        assert torch.equal(p0[k], p1[k]), k
        assert bool(torch.isfinite(p1[k]).all()), k
        assert float((p1[k] - params[k]).abs().max()) > 0.0, k
    moved = (p1[key] != params[key]).reshape(P, -1).any(1)
    assert int(moved.sum()) >= P // 2, int(moved.sum())  # (Adam moves every row whose gradient is not zero)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)
