"""gsr_resize_frame and the tracking resolution without a GPU: the numpy restatements (tests/resize_ref.py)
against torch's own interpolation, resize.resize_literal against the restatements, the scaled intrinsics and
cameras, the entry's refusals (nothing is launched: small host buffers stand in for device memory, as in
tests/test_capi_refusals_cpu.py) and the two loops' argument checks.

The colour bound of resize_literal (and of the kernel, tests/test_gpu_resize.py) is four times the float32
restatement's own largest distance from the float64 one, measured per size pair and printed: the factor leaves
room for a fused multiply-add where numpy rounds twice."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as rr
from splatam_amd import densify as dn
from splatam_amd import resize as rz

PAIRS = rr.SIZE_PAIRS
IDS = [f"{H}x{W}-{h}x{w}" for (H, W), (h, w) in PAIRS]


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_restatement_against_torch(src, dst):
    """Pins the helper, not the product: restate64 is torch's CPU float64 bilinear (align_corners=False) to
    1e-15, the integer nearest rule is torch's mode="nearest" exactly."""
    im, depth = rr.make_frame(*src, seed=1)
    got, d = rr.restate64(im, depth, dst)
    want = F.interpolate(torch.from_numpy(im).double()[None], size=dst, mode="bilinear", align_corners=False)[0].numpy()
    dist = rr.max_distance(got, want)
    print(f"{src} -> {dst}: restate64 against torch float64 {dist:.2e}")
    assert got.dtype == np.float64 and dist <= 1e-15
    want_d = F.interpolate(torch.from_numpy(depth)[None], size=dst, mode="nearest")[0].numpy()
    assert d.shape == want_d.shape and np.array_equal(rr.bits(d), rr.bits(want_d))
    for n_out, n_in in ((dst[0], src[0]), (dst[1], src[1])):
        idx = F.interpolate(torch.arange(n_in, dtype=torch.float64)[None, None], size=n_out, mode="nearest")[0, 0]
        assert np.array_equal(rr.nearest_index(n_out, n_in), idx.numpy().astype(np.int64))


@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_resize_literal(src, dst):
    im, depth = rr.make_frame(*src, seed=2)
    ref64, _ = rr.restate64(im, depth, dst)
    ref32, ref_d = rr.restate32(im, depth, dst)
    out = rz.resize_literal({"im": torch.from_numpy(im), "depth": torch.from_numpy(depth)}, dst)
    assert out["im"].shape == (3, *dst) and out["depth"].shape == (1, *dst)
    assert out["im"].dtype == out["depth"].dtype == torch.float32
    assert out["im"].is_contiguous() and out["depth"].is_contiguous()
    assert np.array_equal(rr.bits(out["depth"].numpy()), rr.bits(ref_d))
    own, dist = rr.max_distance(ref32, ref64), rr.max_distance(out["im"].numpy(), ref64)
    print(f"{src} -> {dst}: float32 restatement {own:.3e} from float64, resize_literal {dist:.3e} (bound {4 * own:.3e})")
    assert dist <= 4 * own
    if src == dst:
        assert np.array_equal(rr.bits(out["im"].numpy()), rr.bits(im))


def test_literal_nan_and_zero_depth():
    """A NaN colour poisons exactly the outputs it enters with a non-zero weight; depths are copied, 0 and NaN
    alike; nothing is masked."""
    (H, W), (h, w) = (48, 64), (30, 40)
    im, depth = rr.make_frame(H, W, seed=3)
    im[1, 20, 33] = np.nan
    depth[0, 10, 12], depth[0, 11, 12] = 0.0, np.nan
    out = rz.resize_literal({"im": torch.from_numpy(im), "depth": torch.from_numpy(depth)}, (h, w))
    x0, x1, rx, _ = rr.taps(w, W)
    y0, y1, ry, _ = rr.taps(h, H)
    hit_x = (x0 == 33) | ((x1 == 33) & (rx != 0))
    hit_y = (y0 == 20) | ((y1 == 20) & (ry != 0))
    want = np.zeros((3, h, w), dtype=bool)
    want[1] = hit_y[:, None] & hit_x[None, :]
    assert want.sum() >= 1 and np.array_equal(np.isnan(out["im"].numpy()), want)
    _, ref_d = rr.restate32(im, depth, (h, w))
    assert np.array_equal(rr.bits(out["depth"].numpy()), rr.bits(ref_d))


def test_scale_intrinsics_and_camera():
    intr = (600.0, 600.0, 599.5, 339.5)
    assert rz.scale_intrinsics(intr, 680, 1200, 340, 600) == (300.0, 300.0, 299.75, 169.75)
    # x by 400 / 1200, y by 170 / 680: the ratio is formed first (datautils.scale_intrinsics)
    fx, fy, cx, cy = rz.scale_intrinsics(intr, 680, 1200, 170, 400)
    assert (fx, cx) == (600.0 * (400 / 1200), 599.5 * (400 / 1200))
    assert (fy, cy) == (600.0 * 0.25, 339.5 * 0.25) == (150.0, 84.875)
    cam = rz.resized_camera(1200, 680, intr, 170, 400, "cpu")
    assert (cam.image_height, cam.image_width) == (170, 400)
    assert cam.tanfovx == 400 / (2 * fx) and cam.tanfovy == 170 / (2 * 150.0)
    proj = torch.tensor([[2 * fx / 400, 0.0, -(400 - 2 * cx) / 400, 0.0], [0.0, 2 * 150.0 / 170, -(170 - 2 * cy) / 170, 0.0],
                         [0.0, 0.0, 100.0 / (100.0 - 0.01), -(100.0 * 0.01) / (100.0 - 0.01)],
                         [0.0, 0.0, 1.0, 0.0]]).float().T
    assert torch.equal(cam.projmatrix[0], proj) and torch.equal(cam.viewmatrix[0], torch.eye(4))
    # at a power-of-two factor the ratio and the product with it are exact: densify.downscale_camera's bits,
    # whatever the intrinsics; at another integer factor (w / W is rounded) the two agree to a double's ulp
    odd = (517.3061, 516.4689, 318.6431, 255.3139)
    for factor in (1, 2, 4):
        a = rz.resized_camera(640, 480, odd, 480 // factor, 640 // factor, "cpu")
        b = dn.downscale_camera(640, 480, odd, factor, "cpu")
        assert (a.image_height, a.image_width, a.tanfovx, a.tanfovy) == (b.image_height, b.image_width, b.tanfovx, b.tanfovy)
        for k in ("viewmatrix", "projmatrix", "campos", "bg"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (factor, k)
    for factor in (3, 5):
        got = rz.scale_intrinsics(odd, 480, 630, 480 // factor, 630 // factor)
        for g, v in zip(got, odd):
            assert abs(g - v / factor) <= 2.0 ** -52 * (v / factor)
    with pytest.raises(ValueError):
        rz.resized_camera(640, 480, odd, 0, 320, "cpu")


# ------------------------------------------------------------------ gsr_resize_frame's refusals

_BUF = (ctypes.c_float * 64)()
D = ctypes.addressof(_BUF)  # a non-null pointer nobody dereferences: a refused call launches nothing
GOOD = dict(H=4, W=6, im=D, depth=D, h0=2, w0=3, im_out0=D, depth_out0=D, h1=3, w1=2, im_out1=D, depth_out1=D,
            stream=None)
REFUSALS = [
    ("H zero", dict(H=0), "bad image size"), ("W negative", dict(W=-2), "bad image size"),
    ("image beyond an int", dict(H=65536, W=65536), "bad image size"),
    ("null im", dict(im=None), "null input"), ("null depth", dict(depth=None), "null input"),
    ("output 0 without its depth", dict(depth_out0=None), "both its colour and its depth"),
    ("output 0 without its colour", dict(im_out0=None), "both its colour and its depth"),
    ("output 1 without its colour", dict(im_out1=None), "both its colour and its depth"),
    ("output 1 without its depth, output 0 absent", dict(im_out0=None, depth_out0=None, depth_out1=None),
     "both its colour and its depth"),
    ("h0 zero", dict(h0=0), "bad output size"), ("w0 negative", dict(w0=-1), "bad output size"),
    ("h1 zero", dict(h1=0), "bad output size"), ("w1 zero", dict(w1=0), "bad output size"),
    ("numerator beyond an int", dict(W=40000, w0=40000), "sizes too large"),
    ("both outputs absent", dict(im_out0=None, depth_out0=None, im_out1=None, depth_out1=None), "no output"),
    # two defects at once: the image's size is checked first, then the inputs, then the outputs in order
    ("bad size and null input", dict(H=0, im=None), "bad image size"),
    ("null input and half an output", dict(im=None, depth_out0=None), "null input"),
]


def test_resize_signature():
    from splatam_amd import _lib, build
    assert "gsr_resize.hip" in build.SOURCES and hasattr(_lib.lib, "gsr_resize_frame")
    assert len(_lib.SIGNATURES["gsr_resize_frame"][1]) == len(GOOD) == 13
    assert _lib.lib.gsr_abi_version() == 8


@pytest.mark.parametrize("name,over,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_resize_refusals(name, over, message):
    from splatam_amd._lib import lib
    rc = lib.gsr_resize_frame(*{**GOOD, **over}.values())
    text = lib.gsr_last_error().decode()
    assert rc == -1 and text.startswith("resize_frame: ") and message in text, (rc, text)


def test_absent_outputs_sizes_are_not_read():
    """An absent output's sizes may be anything: the call with a bad size there is refused for another reason
    only (here: the other output's missing pointer), never for the size."""
    from splatam_amd._lib import lib
    rc = lib.gsr_resize_frame(*{**GOOD, **dict(h1=0, w1=-7, im_out1=None, depth_out1=None, depth_out0=None)}.values())
    assert rc == -1 and "both its colour and its depth" in lib.gsr_last_error().decode()


def test_resize_device_refuses_host_tensors():
    f = {"im": torch.zeros(3, 4, 6), "depth": torch.zeros(1, 4, 6)}
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        rz.resize_device(f, (2, 3))
    with pytest.raises(ValueError):
        rz.resize_literal(f, (0, 3))
    with pytest.raises(ValueError):
        rz.resize_literal({"im": torch.zeros(3, 4, 5), "depth": torch.zeros(1, 4, 6)}, (2, 3))


# ------------------------------------------------------------------ the loops' arguments

def _loops(frames, **kw):
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    params = {"means3D": torch.zeros(5, 3), "rgb_colors": torch.zeros(5, 3), "log_scales": torch.zeros(5, 1)}
    intr = (5.0, 5.0, 3.0, 2.0)
    return (lambda: SlamSequence(params, frames, None, None, intr, capacity=16, bin_capacity=16, **kw),
            lambda: PerFrameSlam(params, frames, None, None, intr, **kw))


def test_loops_take_the_tracking_arguments():
    from splatam_amd.sequence import PerFrameSlam, SlamSequence, _SequenceBase
    for cls in (SlamSequence, PerFrameSlam):
        sig = inspect.signature(cls.__init__).parameters
        assert all(sig[k].default is None for k in ("track_frames", "track_cam", "track_size", "densify_size"))
    assert {"track_frames", "track_cam", "track_size", "densify_size"} <= set(_SequenceBase.OPTIONS)
    assert list(inspect.signature(SlamSequence.push_frames).parameters) == \
        ["self", "im", "depth", "w2c", "densify_frame", "track_frame"]


def test_value_errors():
    frames = [{"im": torch.zeros(3, 4, 6), "depth": torch.ones(1, 4, 6)}] * 2
    small = [rz.resize_literal(f, (2, 3)) for f in frames]
    cam = rz.resized_camera(6, 4, (5.0, 5.0, 3.0, 2.0), 2, 3, "cpu")
    bad = [dict(track_frames=small), dict(track_cam=cam), dict(track_size=(2, 3), track_frames=small, track_cam=cam),
           dict(track_frames=small[:1], track_cam=cam), dict(track_frames=small + small, track_cam=cam),
           dict(densify_size=(2, 3), densify_frames=small, densify_cam=cam, densify_intrinsics=(2.5, 2.5, 1.5, 1.0))]
    for kw in bad:
        for make in _loops(frames, **kw):
            with pytest.raises(ValueError):
                make()


def test_append_frame_takes_the_tracking_frame():
    from splatam_amd.sequence import PerFrameSlam
    f = {"im": torch.zeros(3, 4, 6), "depth": torch.ones(1, 4, 6)}
    s = rz.resize_literal(f, (2, 3))
    cam = rz.resized_camera(6, 4, (5.0, 5.0, 3.0, 2.0), 2, 3, "cpu")
    params = {"means3D": torch.zeros(5, 3), "rgb_colors": torch.zeros(5, 3), "log_scales": torch.zeros(5, 1)}
    loop = PerFrameSlam(params, [f], None, None, (5.0, 5.0, 3.0, 2.0), num_frames=3, track_frames=[s], track_cam=cam)
    assert loop._append_frame(f["im"], f["depth"], track_frame=s) == 1 and len(loop.track_frames) == 2
    with pytest.raises(ValueError):
        loop._append_frame(f["im"], f["depth"])  # a capture with track_frames: one per frame
    assert len(loop.frames) == 2
    curr = loop._track_curr(1)
    assert curr["cam"] is cam and curr["im"] is s["im"] and loop._kf(1)["im"] is f["im"] and loop._kf(1)["cam"] is None
    plain = PerFrameSlam(params, [f], None, None, (5.0, 5.0, 3.0, 2.0), num_frames=3)
    with pytest.raises(ValueError):
        plain._append_frame(f["im"], f["depth"], track_frame=s)  # a capture without track_frames
    assert plain._track_curr(0)["im"] is f["im"]
