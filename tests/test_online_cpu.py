"""CPU checks of the realtime loop's pieces: densify_literal with median_thr / median_scale against the numpy
restatement of gsr_densify_frame_capped's threshold (tests/online_ref.py), the unchanged defaults, the two new
entries' signatures, exports and refusals, matrix_to_quaternion against the reference's recorded outputs
(tests/golden/matrix_to_quaternion.npz, written by tests/golden/make_matrix_to_quaternion.py), init_map_literal,
and the keyframe / map_every / growing-list bookkeeping of the two loops."""
import inspect
import os

import numpy as np
import pytest
import torch

import densify_ref as dr
import online_ref as orf
from splatam_amd import densify as dn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix_to_quaternion.npz")
# the generator's figure: the reference's float32 output against its own float64 evaluation on the fixture's
# matrices (9.029e-08) plus one float32 ulp at 1 (2^-23)
QUAT_TOL = 2.095013782454913e-07

CASES = orf.threshold_cases()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def literal(case: dict, **kw):
    curr = {"im": _t(case["im"]), "depth": _t(case["gt"])}
    return dn.densify_literal(curr, _t(case["w2c"]).reshape(4, 4), case["intrinsics"], case["sil_thres"],
                              _t(case["depth_sil"]), **kw)


@pytest.fixture(scope="module")
def restated():
    return {name: orf.restate_capped(case, thr, scale) for name, case, thr, scale in CASES}


@pytest.mark.parametrize("name,case,median_thr,median_scale", CASES, ids=[c[0] for c in CASES])
def test_literal_equals_capped_restatement(restated, name, case, median_thr, median_scale):
    ref = restated[name]
    rows, mask, count = literal(case, median_thr=median_thr, median_scale=median_scale)
    print(f"{name}: med {ref['med']!r}, thr {ref['thr']!r}, {ref['count']} selected")
    assert count == ref["count"] and np.array_equal(mask.numpy(), ref["mask"])
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities"):
        assert np.array_equal(dr.bits(rows[k].numpy()), dr.bits(ref["rows"][k])), k
    assert dr.rel_distance(rows["log_scales"].numpy(), ref["rows"]["log_scales"]) <= 2.0 ** -23
    got = dn.depth_threshold(torch.tensor(ref["med"]), median_thr, median_scale).numpy()
    assert got.dtype == np.float32 and got.tobytes() == np.float32(ref["thr"]).tobytes()


def test_threshold_rows(restated):
    """The table of include/gsr_glue.h, row by row, and the reset to 50."""
    F = np.float32
    by = {name: (case, thr, scale) for name, case, thr, scale in CASES}
    med = restated["equal"]["med"]
    down = F(by["just_above"][1])
    assert down < med and restated["just_above"]["thr"] == F(3.0 * float(down))  # capped
    assert restated["equal"]["thr"] == F(50.0) * med  # `>`: an equal median is not capped
    assert restated["just_below"]["thr"] == F(50.0) * med
    assert restated["thr0_med_positive"]["thr"] == 0 and restated["thr0_med_zero"]["thr"] == 0
    assert restated["thr0_med_zero"]["med"] == 0
    nan = restated["nan_med"]
    case = by["nan_med"][0]
    assert np.isnan(nan["med"]) and np.isnan(nan["thr"])
    assert np.array_equal(nan["mask"], (case["depth_sil"][1].reshape(-1) < 0.5) & (case["gt"].reshape(-1) > 0))
    assert restated["scale1"]["thr"] == med and restated["scale50"]["thr"] == F(50.0) * med
    assert restated["scale1_capped"]["thr"] == F(float(med) / 2) and restated["scale50_capped"]["thr"] == F(25.0) * med
    # not capped with median_thr given: 50 x the median whatever median_scale is
    for name in ("scale1_uncapped", "scale50_uncapped", "scale50"):
        assert restated[name]["thr"] == F(50.0) * med
        assert np.array_equal(restated[name]["mask"], dr.restate(by[name][0])["mask"])
    assert restated["scale1"]["count"] > restated["scale1_uncapped"]["count"] > 0
    # a capped product that float32 and double round differently: the contract is the double product
    assert orf.threshold(F(1.0), 0.1, 0.7) == F(float(F(0.7)) * float(F(0.1)))


@pytest.mark.parametrize("content", ["random", "zeros90", "nan_depth", "all_selected"])
def test_defaults_are_todays_bits(content):
    from splatam_amd.sequence import non_presence_mask
    case = dr.make_case(61, 67, content, seed=1)
    ref = dr.restate(case)
    rows, mask, count = literal(case)
    rows2, mask2, count2 = literal(case, median_thr=None, median_scale=50.0)
    assert count == count2 == ref["count"] and torch.equal(mask, mask2) and np.array_equal(mask.numpy(), ref["mask"])
    for k in dr.ROW_KEYS:
        assert torch.equal(rows[k], rows2[k]), k
        if k != "log_scales":
            assert np.array_equal(dr.bits(rows[k].numpy()), dr.bits(ref["rows"][k])), k
    ds, gt = _t(case["depth_sil"]), _t(case["gt"])
    assert torch.equal(non_presence_mask(ds, gt, 0.5), mask)
    assert torch.equal(non_presence_mask(ds, gt, 0.5, None, 50.0), mask)
    for name, fn in (("densify_device", dn.densify_device), ("densify_literal", dn.densify_literal)):
        sig = inspect.signature(fn).parameters
        assert sig["median_thr"].default is None and sig["median_scale"].default == 50.0, name


def test_torch_forms_take_the_threshold():
    """non_presence_mask (densify_static's and add_new_gaussians_literal's selection) with the two keywords."""
    from splatam_amd import sequence as sq
    for name, case, thr, scale in CASES:
        got = sq.non_presence_mask(_t(case["depth_sil"]), _t(case["gt"]), case["sil_thres"], thr, scale)
        assert np.array_equal(got.numpy(), orf.restate_capped(case, thr, scale)["mask"]), name
    for fn in (sq.non_presence_mask, sq.densify_static, sq.add_new_gaussians_literal, sq.add_new_gaussians_device):
        sig = inspect.signature(fn).parameters
        assert sig["median_thr"].default is None and sig["median_scale"].default == 50.0, fn.__name__


def test_signatures_exports_and_refusals():
    from splatam_amd import _lib
    for name in ("gsr_densify_frame_capped", "gsr_init_frame"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["gsr_densify_frame_capped"][1]) == 24 + 3
    assert _lib.SIGNATURES["gsr_densify_frame_capped"][1][:24] == _lib.SIGNATURES["gsr_densify_frame"][1]
    assert len(_lib.SIGNATURES["gsr_init_frame"][1]) == 22
    assert len(_lib.SIGNATURES["gsr_densify_frame"][1]) == 24
    assert _lib.lib.gsr_abi_version() == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsr_glue.h")).read()
    assert "gsr_densify_frame_capped(" in hdr and "gsr_init_frame(" in hdr and "resets" in hdr
    for bad in ((0, 7), (5, 0), (-3, 7), (46341, 46341)):  # refused before anything is enqueued: no device is touched
        assert _lib.lib.gsr_densify_frame_capped(*bad, *([None] * 3), 1.0, 1.0, 0.0, 0.0, None, 0.5, 4,
                                                 *([None] * 12), 1, 0.1, 3.0) != 0
        assert b"densify_frame_capped: bad image size" in _lib.lib.gsr_last_error()
        assert _lib.lib.gsr_init_frame(*bad, None, None, 1.0, 1.0, 0.0, 0.0, None, 4, *([None] * 12)) != 0
        assert b"init_frame: bad image size" in _lib.lib.gsr_last_error()
    assert _lib.lib.gsr_init_frame(5, 7, None, None, 1.0, 1.0, 0.0, 0.0, None, -1, *([None] * 12)) != 0
    assert b"init_frame: negative capacity" in _lib.lib.gsr_last_error()
    assert _lib.lib.gsr_init_frame(5, 7, None, None, 1.0, 1.0, 0.0, 0.0, None, 4, *([None] * 12)) != 0
    assert b"init_frame: null pointer" in _lib.lib.gsr_last_error()
    assert _lib.lib.gsr_densify_frame_capped(5, 7, *([None] * 3), 1.0, 1.0, 0.0, 0.0, None, 0.5, -1, *([None] * 12),
                                             0, 0.0, 50.0) != 0
    assert b"densify_frame_capped: negative capacity" in _lib.lib.gsr_last_error()


def test_matrix_to_quaternion_equals_the_reference():
    from splatam_amd.slam import build_rotation, matrix_to_quaternion
    g = np.load(GOLDEN)
    assert float(g["tol"]) == QUAT_TOL
    m = _t(g["matrices"])
    assert set(g["branch"].tolist()) == {0, 1, 2, 3}  # every branch of the best-conditioned choice
    assert abs(float(np.trace(g["matrices"][2])) + 1.0) < 1e-6  # a 180 degree rotation
    q = matrix_to_quaternion(m)
    d = float((q - _t(g["quaternions"])).abs().max())
    print(f"matrix_to_quaternion: largest distance from the reference's output {d:.3e} (tol {QUAT_TOL:.3e})")
    assert q.dtype == torch.float32 and q.shape == (m.shape[0], 4) and d <= QUAT_TOL
    one = matrix_to_quaternion(m[5])  # no batch dimension; and [1,3,3] as the loop passes it
    assert one.shape == (4,) and torch.equal(one, q[5]) and torch.equal(matrix_to_quaternion(m[5:6])[0], q[5])
    # a quaternion of the rotation it came from (up to the matrices' own float32 rounding, 9 entries of 2^-24)
    assert float((build_rotation(q) - m).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        matrix_to_quaternion(torch.zeros(3, 4))


def test_init_map_literal():
    from splatam_amd.sequence import init_map_literal
    case = dr.make_case(5, 7, "random", seed=3)
    case["gt"].reshape(-1)[::3] = 0.0
    ref = orf.restate_init(case)
    p = init_map_literal({"im": _t(case["im"]), "depth": _t(case["gt"])}, _t(case["w2c"]).reshape(4, 4),
                         case["intrinsics"], 6)
    want = ref
    assert p["means3D"].shape[0] == ref["count"] == int((case["gt"] > 0).sum()) < 35
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities"):
        assert np.array_equal(dr.bits(p[k].numpy()), dr.bits(want["rows"][k])), k
    assert dr.rel_distance(p["log_scales"].numpy(), want["rows"]["log_scales"]) <= 2.0 ** -23
    assert p["cam_unnorm_rots"].shape == (1, 4, 6) and p["cam_trans"].shape == (1, 3, 6)
    assert torch.equal(p["cam_unnorm_rots"][0, :, 4], torch.tensor([1.0, 0.0, 0.0, 0.0])) and not p["cam_trans"].any()


def _loop(frames, **kw):
    from splatam_amd.sequence import PerFrameSlam
    params = {"means3D": torch.zeros(5, 3), "rgb_colors": torch.zeros(5, 3), "log_scales": torch.zeros(5, 1)}
    return PerFrameSlam(params, frames, None, None, (5.0, 5.0, 3.0, 2.0), **kw)


def test_bookkeeping_with_a_growing_list():
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    f = {"im": torch.zeros(3, 4, 6), "depth": torch.ones(1, 4, 6)}
    frames = [f]
    loop = _loop(frames, num_frames=6, keyframe_every=2, keyframe_policy="overlap", window=3, map_every=3)
    # overlap: frame 0, every 2nd frame, frame num_frames - 2 = 4 -- although one frame is there yet
    assert [loop._is_keyframe(t) for t in range(6)] == [True, True, False, True, True, True]
    assert [loop._maps(t) for t in range(6)] == [True, False, True, False, False, True]
    assert [_loop([f], num_frames=6, keyframe_every=2)._is_keyframe(t) for t in range(6)] == \
        [False, True, False, True, False, True]
    whole = _loop([f] * 6, keyframe_every=2, keyframe_policy="overlap", window=3)  # today's form: the list's length
    assert [whole._is_keyframe(t) for t in range(6)] == [loop._is_keyframe(t) for t in range(6)]
    assert all(whole._maps(t) for t in range(6)) and whole._n_frames() == 6 == loop._n_frames()
    for t in range(1, 6):
        assert loop._append_frame(f["im"], f["depth"]) == t and len(frames) == t + 1
    with pytest.raises(ValueError):
        loop._append_frame(f["im"], f["depth"])  # beyond num_frames
    assert len(frames) == 6
    with pytest.raises(ValueError):
        whole._append_frame(f["im"], f["depth"])  # no num_frames: the pose columns are the list's
    with pytest.raises(ValueError):
        _loop([f], num_frames=6)._append_frame(f["im"], f["depth"], densify_frame=f)  # a capture without densify_frames
    for kw in (dict(num_frames=1), dict(num_frames=0), dict(map_every=0)):
        with pytest.raises(ValueError):
            _loop([f, f], **kw)
        with pytest.raises(ValueError):
            SlamSequence(None, [f, f], None, None, (5.0, 5.0, 3.0, 2.0), capacity=16, bin_capacity=16, **kw)
    for cls in (SlamSequence, PerFrameSlam):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["median_thr"].default is None and sig["median_scale"].default == 50.0
        assert sig["num_frames"].default is None and sig["map_every"].default == 1
        assert "w2c" in inspect.signature(cls.frame).parameters
    assert list(inspect.signature(SlamSequence.push).parameters) == ["self", "im", "depth", "w2c", "densify_frame"]
