"""The raw-frame intake without a GPU: ingest_literal against the numpy restatement (tests/ingest_ref.py) on every
byte and every uint16 reading, the depth rule's double rounding, odometry_w2c, gsr_ingest_frame's refusals (which
are turned away before the library's first HIP call) and the loops' push_raw argument checks."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import ingest_ref as ir
from splatam_amd import ingest as ig


def _t16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16)


# ------------------------------------------------------------------ the literal form

def test_colour_table_and_every_byte():
    rgb = ir.all_bytes_image()
    assert all(sorted(rgb[..., c].reshape(-1).tolist()) == list(range(256)) for c in range(3))
    assert np.array_equal(ir.bits(ig.COLOUR_TABLE), ir.bits(ir.TABLE))
    # the table is the correctly rounded quotient: the float64 quotient of two small integers, rounded once
    assert np.array_equal(ir.bits(ir.TABLE), ir.bits((np.arange(256) / 255.0).astype(np.float32)))
    out = ig.ingest_literal(torch.from_numpy(rgb), _t16(np.zeros((16, 16), np.uint16)), 1000.0)
    assert out["im"].shape == (3, 16, 16) and out["im"].dtype == torch.float32 and out["im"].is_contiguous()
    assert np.array_equal(ir.bits(out["im"].numpy()), ir.bits(ir.colour(rgb)))
    # torch's CPU `/ 255` is a true division: the same bits (its device form is not pinned to them)
    cpu_form = torch.from_numpy(rgb).float().permute(2, 0, 1) / 255
    assert np.array_equal(ir.bits(cpu_form.contiguous().numpy()), ir.bits(ir.colour(rgb)))
    # ... and a multiply by the rounded reciprocal is NOT the contract for some bytes
    recip = (np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))).astype(np.float32)
    differ = int((ir.bits(recip) != ir.bits(ir.TABLE)).sum())
    print(f"bytes whose reciprocal-multiply differs from the division: {differ}")
    assert differ > 0


@pytest.mark.parametrize("max_depth", [None, ir.MAX_DEPTH])
@pytest.mark.parametrize("scale", ir.SCALES)
def test_every_u16_reading(scale, max_depth):
    d16 = ir.all_u16_image()
    rgb = np.zeros((256, 256, 3), np.uint8)
    for carrier in (_t16(d16), torch.from_numpy(d16.view(np.int16))):  # uint16, or an int16 view of the same bytes
        out = ig.ingest_literal(torch.from_numpy(rgb), carrier, scale, max_depth)
        assert out["depth"].shape == (1, 256, 256) and out["depth"].dtype == torch.float32
        assert np.array_equal(ir.bits(out["depth"].numpy()), ir.bits(ir.depth(d16, scale, max_depth)))
    ref = ir.depth(d16, scale, max_depth).reshape(-1)
    assert ref[0] == 0.0 and not np.signbit(ref[0])  # a zero reading stays +0
    if max_depth is None:
        assert (ref >= 0).all()
        return
    # the threshold: every reading whose ROUNDED quotient is >= 9.5f is -1, the others are untouched
    plain = ir.depth(d16, scale).reshape(-1)
    far = plain >= np.float32(max_depth)
    assert 0 < far.sum() < 65536 and (ref[far] == -1).all()
    assert np.array_equal(ir.bits(ref[~far]), ir.bits(plain[~far]))
    first = int(np.argmax(far))
    assert far[first:].all() and not far[:first].any()  # (monotone: one cut)
    exact = np.arange(65536)[plain == np.float32(max_depth)]
    print(f"scale {scale}: first far reading {first} ({plain[first]!r}); readings rounding exactly to 9.5: {exact.tolist()}")
    if scale in (1000.0, 5000.0):  # 9500 / 1000 and 47500 / 5000 are 9.5 exactly: at the threshold, so -1
        assert exact.tolist() == [int(9.5 * scale)] and ref[int(9.5 * scale)] == -1


def test_a_quotient_that_only_rounds_to_the_threshold():
    """A float64 quotient just below 9.5 whose float32 rounding IS 9.5f: the comparison is on the rounded float32,
    so the reading is far.  (A scale chosen so that such a reading exists.)"""
    scale = 1000.0 * (1 + 2.0 ** -30)
    d16 = np.array([[9500, 9499]], dtype=np.uint16)
    q = d16.astype(np.float64) / scale
    assert q[0, 0] < 9.5 and np.float32(q[0, 0]) == np.float32(9.5)
    out = ig.ingest_literal(torch.zeros(1, 2, 3, dtype=torch.uint8), _t16(d16), scale, 9.5)["depth"].numpy()
    assert np.array_equal(ir.bits(out), ir.bits(ir.depth(d16, scale, 9.5)))
    assert out[0, 0, 0] == -1 and out[0, 0, 1] == np.float32(q[0, 1]) > 0


def test_depth_is_the_float64_quotient_rounded_once():
    """The contract is the float64 quotient rounded to float32 once.  Measured here over all 65,536 readings:
    a correctly rounded float32 division differs from it for 0 readings at 6553.5, 1000 and 5000 (all float32
    values; the second rounding of a division is innocuous at 53 >= 2 * 24 + 2 bits) -- NOT for the 10,752 this
    test was first specified with, a figure no float32 rule tried reproduces.  The float32 rule that does differ
    is the multiply by the reciprocal, torch's device-side `/ scale`: 249 readings at 6553.5, 38,850 at 1000,
    19,860 at 5000.  The contract follows the float64 rule, which is what is asserted."""
    d16 = ir.all_u16_image()
    zeros = torch.zeros(256, 256, 3, dtype=torch.uint8)
    counts = {}
    for scale in ir.SCALES:
        contract = ir.depth(d16, scale)
        div, mul = ir.depth_f32_division(d16, scale), ir.depth_f32_reciprocal(d16, scale)
        counts[scale] = (int((ir.bits(contract) != ir.bits(div)).sum()), int((ir.bits(contract) != ir.bits(mul)).sum()))
        print(f"scale {scale}: float32 division differs for {counts[scale][0]}, reciprocal multiply for "
              f"{counts[scale][1]} of 65536 readings")
        out = ig.ingest_literal(zeros, _t16(d16), scale)["depth"].numpy()
        assert np.array_equal(ir.bits(out), ir.bits(contract)) and not np.array_equal(ir.bits(out), ir.bits(mul))
    assert counts == {1000.0: (0, 38850), 6553.5: (0, 249), 5000.0: (0, 19860)}
    # a scale that is no float32 value: the float32 division (by the rounded scale) is another rule too
    contract, div = ir.depth(d16, 6553.7), ir.depth_f32_division(d16, 6553.7)
    assert int((ir.bits(contract) != ir.bits(div)).sum()) > 0
    out = ig.ingest_literal(zeros, _t16(d16), 6553.7)["depth"].numpy()
    assert np.array_equal(ir.bits(out), ir.bits(contract))


def test_literal_small_frames_and_argument_errors():
    rgb, d16 = ir.raw_frame(37, 53, seed=3)
    full, a, b = ig.ingest_literal(torch.from_numpy(rgb), _t16(d16), 5000.0, 9.5, size=(17, 29), size2=(74, 106))
    for got, size in ((a, (17, 29)), (b, (74, 106))):
        im, d = ir.small(rgb, d16, 5000.0, 9.5, size)
        assert np.array_equal(ir.bits(got["im"].numpy()), ir.bits(im))
        assert np.array_equal(ir.bits(got["depth"].numpy()), ir.bits(d))
    assert (full["depth"] == -1).any() and (full["depth"] == 0).any()
    z8, z16 = torch.zeros(4, 6, 3, dtype=torch.uint8), _t16(np.zeros((4, 6), np.uint16))
    for bad in (lambda: ig.ingest_literal(z8[..., :2], z16, 1000.0), lambda: ig.ingest_literal(z8, z16[:3], 1000.0),
                lambda: ig.ingest_literal(z8, z16, 0.0), lambda: ig.ingest_literal(z8, z16, float("nan")),
                lambda: ig.ingest_literal(z8, z16, 1000.0, size2=(2, 3))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ig.ingest_literal(z8.float(), z16, 1000.0), lambda: ig.ingest_literal(z8, z16.to(torch.int32), 1000.0)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        ig.ingest_device(z8, z16, 1000.0)


# ------------------------------------------------------------------ odometry_w2c

def _pose(xyz, axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return np.array([*xyz, *(np.sin(angle / 2) * axis), np.cos(angle / 2)])


IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def test_odometry_identity_initial_pose_is_the_inverse_pose():
    p = _pose((0.3, -1.2, 2.0), (1, 2, -0.5), 0.7)
    w2c = ig.odometry_w2c(IDENTITY, p)
    assert w2c.shape == (4, 4) and w2c.dtype == torch.float32 and w2c.device.type == "cpu"
    want = np.linalg.inv(ir.pose_matrix(p))
    assert np.abs(w2c.numpy().astype(np.float64) - want).max() <= 1e-6
    assert np.abs(ig.pose_matrix(p) - ir.pose_matrix(p)).max() <= 1e-15


def test_odometry_same_pose_is_the_identity():
    for p in (_pose((0.3, -1.2, 2.0), (1, 2, -0.5), 0.7), _pose((5, 6, 7), (0, 0, 1), 3.0), IDENTITY):
        assert np.abs(ig.odometry_w2c(p, p).numpy() - np.eye(4)).max() <= 1e-6


def test_odometry_yaw_by_hand():
    """The camera starts at (1, 0, 0) unrotated and moves to (1, 2, 0) turned 90 degrees about z.  Its pose
    relative to the start is c2w = [Rz(90) | (0, 2, 0)]; the inverse is [Rz(-90) | -Rz(-90) (0, 2, 0)] with
    Rz(-90) = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], so the translation is -(2, 0, 0)."""
    s = np.sqrt(0.5)
    first = np.array([1, 0, 0, 0, 0, 0, 1.0])
    second = np.array([1, 2, 0, 0, 0, s, s])
    want = np.array([[0, 1, 0, -2], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    assert np.abs(ig.odometry_w2c(first, second).numpy() - want).max() <= 1e-6
    # relative to a start that is itself turned 90 degrees about z at the origin: the second pose in the first's
    # frame is c2w = Rz(-90) [Rz(90) | (1, 2, 0)] = [I | (2, -1, 0)], and w2c = [I | (-2, 1, 0)]
    turned = np.array([0, 0, 0, 0, 0, s, s])
    want = np.eye(4)
    want[:3, 3] = (-2, 1, 0)
    assert np.abs(ig.odometry_w2c(turned, second).numpy() - want).max() <= 1e-6


def test_odometry_normalises_the_quaternion():
    p = _pose((0.3, -1.2, 2.0), (1, 2, -0.5), 0.7)
    scaled = p.copy()
    scaled[3:] *= 3.7
    assert np.array_equal(ig.odometry_w2c(IDENTITY, scaled).numpy(), ig.odometry_w2c(IDENTITY, p).numpy())
    r = ig.pose_matrix(scaled)[:3, :3]
    assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(r) - 1) <= 1e-15
    for bad in (np.zeros(7), np.zeros(6), [0, 0, 0, np.nan, 0, 0, 1]):
        with pytest.raises(ValueError):
            ig.pose_matrix(bad)


# ------------------------------------------------------------------ the C entry's refusals

_BUF = (ctypes.c_float * 64)()
D = ctypes.addressof(_BUF)  # a non-null pointer nobody dereferences: a refused call launches nothing
GOOD = dict(H=4, W=6, rgb_hwc=D, depth_u16=D, png_depth_scale=1000.0, use_max_depth=1, max_depth=9.5, im=D, depth=D,
            h0=2, w0=3, im_out0=D, depth_out0=D, h1=8, w1=12, im_out1=D, depth_out1=D, stream=None)
NO_SMALL = dict(im_out0=None, depth_out0=None, im_out1=None, depth_out1=None)
REFUSALS = [
    ("H_zero", dict(H=0), "bad image size"),
    ("W_negative", dict(W=-3), "bad image size"),
    ("H_W_beyond_an_int", dict(H=65536, W=32768), "bad image size"),
    ("rgb_null", dict(rgb_hwc=None), "null input"),
    ("depth_u16_null", dict(depth_u16=None), "null input"),
    ("scale_zero", dict(png_depth_scale=0.0), "png_depth_scale"),
    ("scale_negative", dict(png_depth_scale=-1000.0), "png_depth_scale"),
    ("scale_inf", dict(png_depth_scale=float("inf")), "png_depth_scale"),
    ("scale_nan", dict(png_depth_scale=float("nan")), "png_depth_scale"),
    ("max_depth_nan", dict(max_depth=float("nan")), "max_depth is NaN"),
    ("im_only", dict(depth=None), "the full frame needs both"),
    ("depth_only", dict(im=None), "the full frame needs both"),
    ("out0_im_only", dict(depth_out0=None), "an output needs both its colour and its depth"),
    ("out1_depth_only", dict(im_out1=None), "an output needs both its colour and its depth"),
    ("out_h_zero", dict(h0=0), "bad output size"),
    ("out_w_negative", dict(w1=-1), "bad output size"),
    ("out_beyond_an_int", dict(h1=65536, w1=32768), "bad output size"),
    ("tap_numerator_x", dict(H=1, W=40000, h0=1, w0=30000), "sizes too large"),
    ("tap_numerator_y", dict(H=40000, W=1, h1=30000, w1=1), "sizes too large"),
    ("nothing_to_write", dict(im=None, depth=None, **NO_SMALL), "no output"),
]


def test_ingest_signature():
    from splatam_amd import _lib, build
    assert "gsr_ingest.hip" in build.SOURCES and hasattr(_lib.lib, "gsr_ingest_frame")
    assert len(_lib.SIGNATURES["gsr_ingest_frame"][1]) == len(GOOD) == 18
    assert _lib.SIGNATURES["gsr_ingest_frame"][1][4] is ctypes.c_double


@pytest.mark.parametrize("name,over,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_ingest_refusals(name, over, message):
    from splatam_amd._lib import lib
    rc = lib.gsr_ingest_frame(*{**GOOD, **over}.values())
    text = lib.gsr_last_error().decode()
    assert rc == -1 and text.startswith("ingest_frame: ") and message in text, (rc, text)


def test_unused_arguments_are_not_read():
    """A NaN max_depth without use_max_depth, and an absent output's sizes, are not what a call is refused for."""
    from splatam_amd._lib import lib
    over = dict(use_max_depth=0, max_depth=float("nan"), h1=0, w1=-7, im_out1=None, depth_out1=None, depth_out0=None)
    rc = lib.gsr_ingest_frame(*{**GOOD, **over}.values())
    assert rc == -1 and "both its colour and its depth" in lib.gsr_last_error().decode()


# ------------------------------------------------------------------ the loops' arguments

def _loop(**kw):
    from splatam_amd.sequence import PerFrameSlam
    f = {"im": torch.zeros(3, 4, 6), "depth": torch.ones(1, 4, 6)}
    params = {"means3D": torch.zeros(5, 3), "rgb_colors": torch.zeros(5, 3), "log_scales": torch.zeros(5, 1)}
    return PerFrameSlam(params, [f], None, None, (5.0, 5.0, 3.0, 2.0), num_frames=3, **kw)


def test_loops_take_the_raw_arguments():
    from splatam_amd.sequence import PerFrameSlam, SlamSequence, _SequenceBase
    for cls in (SlamSequence, PerFrameSlam):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["png_depth_scale"].default is None and sig["max_depth"].default is None
        assert sig["arrival_report"].default is False
        assert {"rgb_u8", "depth_u16", "pose", "w2c"} <= set(inspect.signature(cls.push_raw).parameters)
    assert {"png_depth_scale", "max_depth", "arrival_report"} <= set(_SequenceBase.OPTIONS)
    assert list(inspect.signature(SlamSequence.push_raw).parameters) == ["self", "rgb_u8", "depth_u16", "pose", "w2c"]


def test_push_raw_value_errors():
    from splatam_amd import resize as rz
    z8, z16 = torch.zeros(4, 6, 3, dtype=torch.uint8), _t16(np.zeros((4, 6), np.uint16))
    with pytest.raises(ValueError, match="png_depth_scale"):
        _loop().push_raw(z8, z16)
    with pytest.raises(ValueError, match="not both"):
        _loop(png_depth_scale=1000.0).push_raw(z8, z16, pose=IDENTITY, w2c=torch.eye(4))
    f = {"im": torch.zeros(3, 4, 6), "depth": torch.ones(1, 4, 6)}
    small, cam = rz.resize_literal(f, (2, 3)), rz.resized_camera(6, 4, (5.0, 5.0, 3.0, 2.0), 2, 3, "cpu")
    owner = _loop(png_depth_scale=1000.0, track_frames=[small], track_cam=cam)
    with pytest.raises(ValueError, match="owns its small frames"):
        owner.push_raw(z8, z16)
    assert len(owner.frames) == 1 and owner.initial_pose is None  # nothing was appended
    with pytest.raises(ValueError, match="png_depth_scale"):  # raw frames at construction need the scale too
        from splatam_amd.sequence import PerFrameSlam
        PerFrameSlam({}, [{"rgb_u8": z8, "depth_u16": z16}], None, None, (5.0, 5.0, 3.0, 2.0))
