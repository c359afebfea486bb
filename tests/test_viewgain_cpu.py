"""CPU checks of the view-gain additions (splatam_amd.fisher mode "gains", gsr_silhouette_count): the entry point
is declared, mirrored and built, its argument checks answer before anything is launched, the float64 gain
combination restates send_gains (scripts/ros_handler.py:299-322), and gains mode refuses an anisotropic map."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsr_silhouette_count"


def test_entry_point_is_declared_mirrored_and_built():
    from splatam_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gsr_glue.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % NAME, hdr, re.M | re.S)
    assert m, "not declared in include/gsr_glue.h"
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == 9
    assert "gsr_viewgain.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "splatam_amd", "csrc", "gsr_viewgain.hip"))
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)


def _settings(W=64, H=48, bg=1):
    from splatam_amd._lib import GsrSettings
    return GsrSettings(image_height=H, image_width=W, tan_fovx=1.0, tan_fovy=1.0, bg=bg or None, scale_modifier=1.0,
                       viewmatrix=None, projmatrix=None, sh_degree=0, campos=None, prefiltered=0, binning=0)


def test_argument_errors_name_the_function():
    """Every refusal is decided on the host before a launch (the pointers below are never dereferenced)."""
    from splatam_amd._lib import lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ok = _settings()
    cases = {
        "null settings": (None, 4, 10, p, p, p, p),
        "null count": (ctypes.byref(ok), 4, 10, p, p, p, None),
        "zero width": (ctypes.byref(_settings(W=0)), 4, 10, p, p, p, p),
        "negative height": (ctypes.byref(_settings(H=-3)), 4, 10, p, p, p, p),
        "too many pixels": (ctypes.byref(_settings(W=70000, H=70000)), 4, 10, p, p, p, p),
        "negative P": (ctypes.byref(ok), -1, 10, p, p, p, p),
        "negative num_rendered": (ctypes.byref(ok), 4, -1, p, p, p, p),
        "no geometry buffer": (ctypes.byref(ok), 4, 10, None, p, p, p),
        "no image buffer": (ctypes.byref(ok), 4, 10, p, p, None, p),
        "no binning buffer": (ctypes.byref(ok), 4, 10, p, None, p, p),
        "no background": (ctypes.byref(_settings(bg=0)), 4, 10, p, p, p, p),
    }
    for what, (st, P, n, geom, binning, img, count) in cases.items():
        rc = lib.gsr_silhouette_count(st, P, n, geom, binning, img, 0.5, count, None)
        assert rc != 0, what
        assert "silhouette_count" in lib.gsr_last_error().decode(), what


def _restated(count, eig, npix, k_sil, k_eig, k_sum, nl_sil, nl_eig):
    """scripts/ros_handler.py:299-322 for one pose, in Python floats."""
    g_sil = float(count)
    g_sil /= npix
    g_eig = eig if k_eig != 0 else 0
    g_sil *= k_sil
    g_eig *= k_eig
    if nl_sil:
        g_sil = (3400 / (1 + math.exp(-0.002 * g_sil))) - 1700
    if nl_eig:
        g_eig = (3400 / (1 + math.exp(-0.002 * g_eig))) - 1700
    return g_sil, g_eig, k_sum * (g_eig + g_sil)


@pytest.mark.parametrize("nl_sil", [False, True])
@pytest.mark.parametrize("nl_eig", [False, True])
@pytest.mark.parametrize("w", [(1.0, 1.0, 1.0), (250.0, 0.3, 2.5), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (3.0, 2.0, 0.0)])
def test_gain_combination_restates_send_gains(nl_sil, nl_eig, w):
    from splatam_amd.fisher import combine_gains
    npix = 640 * 480
    counts = torch.tensor([0, 1, 2690, 153600, npix], dtype=torch.int32)
    eig = torch.tensor([0.0, 3.25, 812.5, 41234.125, 1.5e6], dtype=torch.float64)
    got = combine_gains(counts, eig, npix, k_sil=w[0], k_eig=w[1], k_sum=w[2], nl_sil=nl_sil, nl_eig=nl_eig)
    assert got.dtype == torch.float64 and got.shape == (5, 3)
    for i in range(5):
        want = _restated(int(counts[i]), float(eig[i]), npix, w[0], w[1], w[2], nl_sil, nl_eig)
        # the linear path is the same float64 operations in the same order: equal.  The non-linear map subtracts
        # 1700 from a value near 1700 (one ulp of it is 2.3e-13) and torch's exp may differ from libm's in
        # the last place, which 3400 / (1 + e)^2 ~ 850 scales: a few 1e-13 absolute; the sum carries k_sum times it.
        tol = 0.0 if not (nl_sil or nl_eig) else 2e-12 * max(1.0, abs(w[2]))
        for c in range(3):
            assert abs(float(got[i, c]) - want[c]) <= tol * max(1.0, abs(want[c])), (i, c, float(got[i, c]), want[c])


def test_gains_mode_refuses_an_anisotropic_map():
    from splatam_amd.fisher import BatchedFisher, FisherScorer
    from splatam_amd.scenes import make_scene
    from splatam_amd.slam import camera_settings, init_tracking_params
    scene = make_scene(50, 32, 32, seed=1, anisotropic=True)
    params = init_tracking_params(scene, num_frames=1, device="cpu")
    params["log_scales"] = torch.log(scene.scales)
    sc = FisherScorer(params, camera_settings(scene.cam, "cpu"))
    with pytest.raises(ValueError, match="isotropic"):
        BatchedFisher(sc, 2, mode="gains")
    with pytest.raises(ValueError, match="mode is"):
        BatchedFisher(sc, 2, mode="nonsense")
