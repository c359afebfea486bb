"""Numpy restatements for the realtime loop's entries (include/gsr_glue.h: gsr_densify_frame_capped,
gsr_init_frame), written from the contract on top of tests/densify_ref.py: the capped threshold of step 3 and
the selection it gives, the first frame's selection (gt > 0), and the seeded cases tests/test_online_cpu.py and
tests/test_gpu_online.py share.  Steps 4-6 are densify_ref.restate's: a selection is handed to it as a case whose
silhouette is 0 on the selected pixels and 1 elsewhere and whose rendered depth equals the measured one (the
depth term is then false everywhere), so the row arithmetic exists once."""
import numpy as np

import densify_ref as dr

F32 = np.float32


def threshold(med, median_thr, median_scale) -> np.float32:
    """Step 3's thr.  median_thr None: use_median_thr clear."""
    med = F32(med)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if median_thr is None:
            return F32(median_scale) * med
        if med > F32(median_thr):  # (false for a NaN med)
            return F32(float(F32(median_scale)) * float(F32(median_thr)))  # the double product, rounded once
        return F32(50.0) * med  # median_scale is not used here: the reference's reset to 50


def _rows_of(case: dict, mask: np.ndarray) -> dict:
    H, W = case["H"], case["W"]
    gt = case["gt"].reshape(-1)
    assert not (mask & ~(gt > 0)).any()
    sil = np.where(mask, F32(0.0), F32(1.0)).astype(F32)
    ds = np.stack((gt, sil, (gt * gt).astype(F32))).reshape(3, H, W).astype(F32)
    ref = dr.restate(dict(case, depth_sil=ds, sil_thres=0.5))
    assert np.array_equal(ref["mask"], mask)
    return ref


def restate_capped(case: dict, median_thr=None, median_scale=50.0) -> dict:
    """densify_ref.restate's dict for gsr_densify_frame_capped(..., median_thr is not None, median_thr, median_scale)."""
    rd, sil = case["depth_sil"][0].reshape(-1), case["depth_sil"][1].reshape(-1)
    gt = case["gt"].reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        valid = gt > 0
        err = (np.abs(gt - rd) * valid.astype(F32)).astype(F32)
        med = dr.lower_median(err)
        thr = threshold(med, median_thr, median_scale)
        assert err.dtype == F32 and thr.dtype == F32
        mask = ((sil < F32(case["sil_thres"])) | ((rd > gt) & (err > thr))) & valid
    ref = _rows_of(case, mask)
    ref.update(med=med, thr=thr)
    return ref


def restate_init(case: dict) -> dict:
    """densify_ref.restate's dict for gsr_init_frame: every pixel with gt > 0."""
    return _rows_of(case, case["gt"].reshape(-1) > 0)


def threshold_cases() -> list:
    """(name, case, median_thr, median_scale) at 48 x 64: a median a float32 step above, equal to and a step below
    median_thr; median_thr = 0 with a positive and with a zero median; a NaN median; median_scale 1 and 50 with
    and without median_thr, capped and not (the uncapped ones with median_thr show the reset to 50)."""
    rnd = dr.make_case(48, 64, "random", seed=2)
    med = F32(dr.restate(rnd)["med"])
    assert med > 0
    up, down = np.nextafter(med, F32(np.inf)), np.nextafter(med, F32(0.0))
    zeros, nan = dr.make_case(48, 64, "zeros90", seed=2), dr.make_case(48, 64, "nan_depth", seed=2)
    assert dr.restate(zeros)["med"] == 0 and np.isnan(dr.restate(nan)["med"])
    return [("just_above", rnd, float(down), 3.0), ("equal", rnd, float(med), 3.0), ("just_below", rnd, float(up), 3.0),
            ("thr0_med_positive", rnd, 0.0, 3.0), ("thr0_med_zero", zeros, 0.0, 3.0), ("nan_med", nan, 0.01, 1.0),
            ("scale1", rnd, None, 1.0), ("scale50", rnd, None, 50.0),
            ("scale1_capped", rnd, float(med) / 2, 1.0), ("scale50_capped", rnd, float(med) / 2, 50.0),
            ("scale1_uncapped", rnd, float(med) * 2, 1.0), ("scale50_uncapped", rnd, float(med) * 2, 50.0)]
