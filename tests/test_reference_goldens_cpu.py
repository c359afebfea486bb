"""The float32 and float64 oracle against results recorded from the reference's own kernels on the GPU
(tests/golden/ref_raster/*.npz, written by tools/record_reference_goldens.py from oracle/reference.py: the
reference's forward.cu / backward.cu / rasterizer_impl.cu compiled by hipcc for gfx950).  Same assertions as
tests/test_gpu_reference.py (tests/reference_cases.py), on machines with neither the library nor a GPU; plus
the input check of every case of that test and the build recipe's behaviour without a reference checkout.

The reference's distance to float64 that a raised bound would rest on is taken here from the recorded run
plus the recorded two-run spread.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import reference_cases as rc
from oracle import harness

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_raster")
ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")


@functools.lru_cache(maxsize=None)
def _golden(name):
    """(file, scene rebuilt from its recorded inputs, float32 frame, float64 frame)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    scene, kw = rc.recorded_scene(z)
    return (z, scene) + rc.frames_of(scene, kw)


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_inputs_sit_within_the_cap(name):
    """The float32 oracle against the float64 oracle alone on every case of the comparison: rows and pixels
    whose discrete state differs stay within the 0.1 % cap, no pixel differs away from a flagged decision,
    and the lists agree at least as per-tile sets."""
    r = rc.input_check(*rc.oracle_frames(name)[1:])
    assert r["rows"] <= rc.CAP and r["pixels"] <= rc.CAP and r["unflagged_pixels"] == 0 and r["lists_as_sets"], r


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_recorded_inputs_are_the_case(name):
    """The scene the files were recorded from is the scene the case builds today, to the last place or two
    (torch's CPU transcendentals differ between hosts; the comparisons below run on the recorded inputs), and
    it too sits within the cap."""
    z, _, fr32, fr64 = _golden(name)
    case = rc.BY_NAME[name]
    for k, v in rc.scene_inputs(case.scene(), case.kwargs()).items():
        np.testing.assert_allclose(z[k], v, rtol=1e-6, atol=1e-7, err_msg=k)
    r = rc.input_check(fr32, fr64)
    assert r["rows"] <= rc.CAP and r["pixels"] <= rc.CAP and r["unflagged_pixels"] == 0 and r["lists_as_sets"], r


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_forward_state(name):
    z, _, fr32, fr64 = _golden(name)
    ref = {k: z[k] for k in rc.FRAME_KEYS}
    ref["num_rendered"] = int(z["num_rendered"])
    assert ref["num_rendered"] > 0
    fails = []
    for tag, fr, lists in (("oracle32", fr32, "exact"), ("oracle64", fr64, "sets")):
        rep, f = rc.compare_frame(f"{name} {tag}", ref, rc.frame_dict(fr), fr32, fr64, lists=lists)
        print(rep)
        fails += f
    assert not fails, fails


@pytest.mark.parametrize("name,power,seed", rc.GOLDEN_RUNS, ids=[f"{n}-p{p}" for n, p, _ in rc.GOLDEN_RUNS])
def test_gradients(name, power, seed):
    z, scene, fr32, fr64 = _golden(name)
    d = z[f"dpix_p{power}"]
    np.testing.assert_array_equal(d, rc.dpix(scene, seed))
    ref = {k: z[f"g_p{power}_{k}"] for k in harness.GRAD_KEYS}
    v32, _, v64 = rc.grads_of(fr32, fr64, d, power)
    dist = {k: v + float(z[f"spread_p{power}_{k}"]) for k, v in rc.reference_distance([ref], v64).items()}
    stable = ~(fr32.unstable | fr64.unstable)
    fails = []
    for who, cand in (("oracle32", v32), ("oracle64", v64)):
        rep, f = rc.compare_grads(f"{name} p{power} {who}", ref, dist, cand, v32, v64, stable, int(fr64.n_contrib.max()))
        print(rep)
        fails += f
    assert not fails, fails


def test_ref_target_without_a_checkout_is_a_no_op(tmp_path):
    """`make -C oracle ref` with GSR_REFERENCE pointing nowhere succeeds, prints nothing, compiles nothing
    and leaves an existing library as it is: the case of a machine without the reference checkout, where
    oracle.build() must not fail the build."""
    lib = os.path.join(ORACLE_DIR, "_ref", "libref_raster.so")
    before = os.stat(lib).st_mtime_ns if os.path.exists(lib) else None
    env = dict(os.environ, GSR_REFERENCE=str(tmp_path / "absent"))
    r = subprocess.run(["make", "-s", "-C", ORACLE_DIR, "ref"], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (r.returncode, r.stdout, r.stderr)
    after = os.stat(lib).st_mtime_ns if os.path.exists(lib) else None
    assert after == before
    r = subprocess.run(["make", "-n", "-C", ORACLE_DIR, "ref"], env=env, capture_output=True, text=True)
    assert "hipcc" not in r.stdout
