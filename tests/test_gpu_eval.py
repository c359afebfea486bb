"""The evaluation kernels (gsr_eval_frame through splatam_amd.evaluate.frame_metrics) against the float64 numpy
restatement of tests/eval_ref.py on seeded images, their workspace contract, determinism, graph capture and
error paths; evaluate_sequence on a capacity-padded map against evaluate_literal fed by plain renders; and
SlamSequence.evaluate.

Tolerances (relative to the float64 restatement).  MEASURED is the largest distance of the float32 torch literal
(evaluate_literal on CPU tensors: the same precision as the reference's eval(), another summation order) from the
float64 restatement over this module's seeded cases -- 161x163, 163x161, 176x200, 240x320 with MS-SSIM and 1x1,
5x7, 61x4101, 4101x61 without, both mask modes (tests/test_eval_cpu.py prints the distances):
    psnr 1.09e-7, ms_ssim 7.8e-8, depth_rmse / depth_l1 1.33e-7, mse_c 1.21e-7
-- about two units of float32 roundoff (2^-24 = 6.0e-8): the literal is correct to the rounding of its float32
result.  The device is allowed 4 x MEASURED (BOUND).  n_valid, the NaN / inf cases and everything stated as
"bits" are exact.  Against evaluate_literal (the padded-map test) the allowance is BOUND plus the literal's own
distance from the restatement on those very images."""
import contextlib

import numpy as np
import pytest
import torch

import eval_ref as er
from splatam_amd import evaluate as ev

pytestmark = pytest.mark.gpu

MEASURED = {"psnr": 1.09e-7, "ms_ssim": 7.8e-8, "depth_rmse": 1.33e-7, "depth_l1": 1.33e-7, "n_valid": 0.0,
            "mse_r": 1.21e-7, "mse_g": 1.21e-7, "mse_b": 1.21e-7}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
KEYS = ("im", "depth_sil", "gt_im", "gt_depth")


def _dev(c, dev):
    return [torch.from_numpy(np.array(c[k])).to(dev) for k in KEYS]


def _row(c, dev, use_sil, ms, ws=None, thres=None):
    a = _dev(c, dev)
    H, W = a[0].shape[1:]
    ws = ev.make_workspace(H, W, dev, ms) if ws is None else ws
    table = torch.full((3, 8), float("nan"), device=dev)
    ev.frame_metrics(*a, c["sil_thres"] if thres is None else thres, table[1], ws, use_sil_mask=use_sil, ms_ssim=ms)
    torch.cuda.synchronize()
    assert torch.isnan(table[0]).all() and torch.isnan(table[2]).all()  # the neighbouring rows are untouched
    assert int(ws[:16].abs().sum()) == 0  # the counter words are back to zero
    return table[1].clone()


def _check(row, ref, tag, bound=BOUND, extra=None):
    got = row.detach().cpu().numpy().astype(np.float64)
    bad = []
    for i, name in enumerate(er.COLS):
        if np.isnan(ref[i]) or np.isinf(ref[i]) or ref[i] == 0:
            ok, rel = (np.isnan(got[i]) if np.isnan(ref[i]) else got[i] == ref[i]), float("nan")
        else:
            rel = abs(got[i] - ref[i]) / abs(ref[i])
            ok = rel <= bound[name] + (0.0 if extra is None else extra[i])
        print(f"{tag} {name}: device {got[i]!r} ref {ref[i]!r} rel {rel:.3e} (bound {bound[name]:.2e})")
        if not ok:
            bad.append(name)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("use_sil", [False, True])
@pytest.mark.parametrize("H,W", [(161, 163), (163, 161), (176, 200), (240, 320)])
def test_pyramid_matches_restatement(cuda, H, W, use_sil):
    c = er.make_case(H, W)
    _check(_row(c, cuda, use_sil, True), er.reference(H, W, use_sil), f"{H}x{W} sil={use_sil}")


@pytest.mark.parametrize("use_sil", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (61, 4101), (4101, 61)])
def test_pixel_metrics_match_restatement(cuda, H, W, use_sil):
    depth = "valid" if H == 1 else "mixed"
    c = er.make_case(H, W, depth=depth)
    row = _row(c, cuda, use_sil, False)
    ref = er.reference(H, W, use_sil, False, depth=depth)
    assert np.isnan(ref[1]) and float(row[4]) == ref[4]
    _check(row, ref, f"{H}x{W} sil={use_sil}")


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0, posinf=1e30), torch.nan_to_num(b, nan=-7.0, posinf=1e30)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))


def test_invalid_valid_and_threshold_edges(cuda):
    # all-invalid depth: NaN depth columns, PSNR of two zero images = inf; what evaluate_literal gives
    c = er.make_case(5, 7, depth="invalid")
    row = _row(c, cuda, False, False).cpu()
    lit = ev.evaluate_literal(*_dev(c, "cpu"), 0.5, ms_ssim=False)
    assert torch.isinf(row[0]) and row[0] > 0 and torch.isnan(row[2]) and torch.isnan(row[3]) and row[4] == 0
    assert _same(row, lit)
    # all-valid depth: the count is the image
    c = er.make_case(61, 4101, depth="valid")
    assert float(_row(c, cuda, True, False)[4]) == 61 * 4101
    # a silhouette exactly at sil_thres is NOT present (strict >); just below the threshold all of it is
    c = dict(er.make_case(5, 7, depth="valid"))
    ds = np.array(c["depth_sil"])
    ds[1] = np.float32(0.5)
    c["depth_sil"] = ds
    at = _row(c, cuda, True, False, thres=0.5).cpu()
    assert torch.isinf(at[0]) and float(at[2]) == 0.0 and float(at[3]) == 0.0 and float(at[4]) == 35
    below = _row(c, cuda, True, False, thres=float(np.nextafter(np.float32(0.5), np.float32(0)))).cpu()
    unmasked = _row(c, cuda, False, False).cpu()
    assert torch.isfinite(below).sum() == 7 and _same(below, unmasked)


def test_deterministic_bits(cuda):
    c = er.make_case(176, 200)
    ws = ev.make_workspace(176, 200, cuda)
    rows = [_row(c, cuda, True, True, ws=ws) for _ in range(2)] + [_row(c, cuda, True, True)]
    assert torch.isfinite(rows[0]).all()
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


def test_workspace_reuse_across_sizes(cuda):
    """One workspace of the largest size, used alternately for two image sizes (and a pixel-only call), gives
    the bits of fresh workspaces."""
    big, small = er.make_case(240, 320), er.make_case(161, 163)
    ws = ev.make_workspace(240, 320, cuda)
    assert ws.numel() * 4 >= ev.workspace_bytes(161, 163)
    fresh = {id(c): _row(c, cuda, False, True) for c in (big, small)}
    fresh_pix = _row(small, cuda, True, False)
    for c in (big, small, big, small):
        assert torch.equal(_row(c, cuda, False, True, ws=ws), fresh[id(c)])
        assert _same(_row(small, cuda, True, False, ws=ws), fresh_pix)


def test_graph_replay(cuda):
    """frame_metrics captured as a linear chain, replayed after the four inputs changed in place: the eager
    call's bits on the new values."""
    ca, cb = er.make_case(176, 200), er.make_case(176, 200, seed=4242)
    args = _dev(ca, cuda)
    ws = ev.make_workspace(176, 200, cuda)
    table = torch.full((2, 8), float("nan"), device=cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        ev.frame_metrics(*args, 0.5, table[0], ws, use_sil_mask=True)  # (warm-up)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    first = table[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ev.frame_metrics(*args, 0.5, table[0], ws, use_sil_mask=True)
    for a, b in zip(args, _dev(cb, cuda)):
        a.copy_(b)
    table.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    eager = _row(cb, cuda, True, True)
    assert torch.equal(table[0], eager) and not torch.equal(eager, first)
    assert torch.isnan(table[1]).all() and int(ws[:16].abs().sum()) == 0


def test_error_paths(cuda):
    from splatam_amd._lib import lib
    c = er.make_case(160, 200)
    a = _dev(c, cuda)
    row = torch.full((8,), -7777.0, device=cuda)
    ws = ev.make_workspace(240, 320, cuda)
    rc = lib.gsr_eval_frame(160, 200, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), 0.5, 0, 1,
                            ws.data_ptr(), row.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
    assert rc < 0 and b"160" in lib.gsr_last_error()
    with pytest.raises(RuntimeError, match="160"):
        ev.frame_metrics(*a, 0.5, row, ws, ms_ssim=True)
    torch.cuda.synchronize()
    assert bool((row == -7777.0).all()) and int(ws.abs().sum()) == 0  # nothing was written
    ev.frame_metrics(*a, 0.5, row, ws, ms_ssim=False)  # the pixel metrics of the same image are fine
    torch.cuda.synchronize()
    assert torch.isnan(row[1]) and torch.isfinite(row[0])
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        ev.frame_metrics(*_dev(c, "cpu"), 0.5, torch.zeros(8), torch.zeros(64, dtype=torch.int32), ms_ssim=False)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ev.frame_metrics(*_dev(er.make_case(176, 200), cuda), 0.5, row, torch.zeros(64, dtype=torch.int32, device=cuda))


# ------------------------------------------------------------------ renders / sequence

@contextlib.contextmanager
def no_host_read():
    """Raises on any Python-level read of a device tensor (item, cpu, tolist, numpy, bool / int / float)."""
    names = ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__")
    saved = {n: getattr(torch.Tensor, n) for n in names}

    def guard(name, fn):
        def wrapped(self, *a, **k):
            if self.is_cuda:
                raise AssertionError(f"host read of a device tensor: Tensor.{name}")
            return fn(self, *a, **k)
        return wrapped

    for n, fn in saved.items():
        setattr(torch.Tensor, n, guard(n, fn))
    try:
        yield
    finally:
        for n, fn in saved.items():
            setattr(torch.Tensor, n, fn)


@pytest.fixture(scope="module")
def capture(cuda):
    from splatam_amd.scenes import make_scene
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    cap = sequence_workload(make_scene(20_000, 320, 240, seed=7), 3, torch.device(cuda))
    params, frames, cam, w2c = cap[:4]
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
    return cap, 4 * n + 400_000


def test_padded_map_against_literal(cuda, capture):
    from splatam_amd.rasterizer import GaussianRasterizer
    from splatam_amd.sequence import pad_map
    from splatam_amd.slam import transform_to_frame, transformed_params2depthplussilhouette, \
        transformed_params2rendervar
    (params, frames, cam, w2c, _, _), bin_cap = capture
    P = params["means3D"].shape[0]
    padded, alive, _ = pad_map(params, P + 1000)
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    with no_host_read():
        table, times = ev.evaluate_sequence(padded, frames, cam, w2c, sil_thres=0.5, alive=alive,
                                            bin_capacity=bin_cap, status=status)
    torch.cuda.synchronize()
    assert times == [0, 1, 2] and table.shape == (3, 8)
    st = status.cpu()
    assert int(st[0]) <= bin_cap and int(st[1]) == 0
    for i, t in enumerate(times):
        with torch.no_grad():
            tg = transform_to_frame(params, t, False, False)
            im, _, _ = GaussianRasterizer(cam)(**transformed_params2rendervar(params, tg))
            ds, _, _ = GaussianRasterizer(cam)(**transformed_params2depthplussilhouette(params, w2c, tg))
        a = (im, ds, frames[t]["im"], frames[t]["depth"])
        lit = ev.evaluate_literal(*(x.cpu() for x in a), 0.5).numpy().astype(np.float64)  # (CPU tensors)
        ref = er.frame_metrics(*(x.cpu().numpy() for x in a), 0.5, False)
        own = np.abs(lit - ref) / np.abs(ref)  # the literal's own distance from the restatement
        print(f"frame {t}: literal's own distance {own}")
        _check(table[i], ref, f"frame {t} vs restatement")
        _check(table[i], lit, f"frame {t} vs literal", extra=np.nan_to_num(own))
        assert float(table[i, 4]) == lit[4]
    assert float(table[1, 0]) != float(table[0, 0])


def test_slam_sequence_evaluate(cuda, capture):
    from splatam_amd.sequence import SlamSequence
    (params, frames, cam, w2c, intr, (q_gt, t_gt)), bin_cap = capture
    seq = SlamSequence(params, frames, cam, w2c, intr, capacity=params["means3D"].shape[0] + 2 * 320 * 240,
                       bin_capacity=bin_cap, seed=0, tracking_iters=20, mapping_iters=10, window=3, keyframe_every=1)
    seq.frame(0)
    with no_host_read():
        seq.frame(1)
    seq.check()
    gt_w2c = ev.poses_w2c(q_gt, t_gt)
    before = {k: v.detach().clone() for k, v in seq.params.items() if torch.is_tensor(v)}
    out = seq.evaluate(gt_w2c=gt_w2c)
    assert all(torch.equal(v, seq.params[k]) for k, v in before.items())  # evaluation only reads the map
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    table, times = ev.evaluate_sequence(seq.params, frames, cam, w2c, sil_thres=seq.sil_thres, alive=seq.alive,
                                        bin_capacity=bin_cap, status=status)
    torch.cuda.synchronize()
    assert out["times"] == times == [0, 1, 2] and torch.equal(out["table"], table)
    t = table.cpu().numpy()
    for k, col in (("psnr", 0), ("ssim", 1), ("rmse", 2), ("l1", 3)):
        assert np.array_equal(out[k], t[:, col]) and out["avg_" + k] == float(t[:, col].mean())
    print({k: out[k] for k in ("avg_psnr", "avg_ssim", "avg_rmse", "avg_l1", "ate_rmse")})
    assert all(np.isfinite(out["avg_" + k]) for k in ("psnr", "ssim", "rmse", "l1")) and 0 < out["avg_ssim"] <= 1
    est = [w2c.cpu().numpy()] + [ev.pose_w2c(seq.params, i).cpu().numpy() for i in range(1, 3)]
    want = er.ate(gt_w2c.cpu().numpy(), est)
    assert abs(out["ate_rmse"] - want) <= 1e-9 + 1e-9 * want
    with no_host_read():
        seq.frame(2)  # the sequence goes on as before
    seq.check()
