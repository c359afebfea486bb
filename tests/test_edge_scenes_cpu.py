"""The constructed edge scenes (tests/edge_scenes.py) do what they claim, on the CPU oracle: exact list
lengths and orders, exact block-mask popcounts, no (pixel, entry) pair and no transmittance near a
threshold -- so the GPU tests (tests/test_gpu_edges.py) may compare every pixel and every Gaussian."""
import os
import re

import numpy as np
import pytest

import edge_scenes as es
from oracle import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = dict(es.all_scenes())


def _walk(fr64, t):
    """float64 restatement of the forward walk of tile t (forward.cu:330-360): per list entry the alpha of
    every pixel (0 where the pair does not blend), its power and test_T; per pixel n_contrib."""
    X, Y, _ = es.block_of_pixel()
    a, b = fr64.ranges[t]
    ids = fr64.point_list[a:b]
    m2, co = fr64.means2D, fr64.conic_opacity
    dx = m2[ids, 0][:, None] - (16 * t + X)[None]
    dy = m2[ids, 1][:, None] - Y[None]
    power = -0.5 * (co[ids, 0, None] * dx * dx + co[ids, 2, None] * dy * dy) - co[ids, 1, None] * dx * dy
    alpha = co[ids, 3, None] * np.exp(power)
    T = np.ones(256)
    done = np.zeros(256, bool)
    ncon = np.zeros(256, np.int64)
    test_T = np.full(alpha.shape, np.nan)
    for k in range(len(ids)):
        blend = (power[k] <= 0) & (alpha[k] >= 1 / 255) & ~done
        tt = T * (1 - np.minimum(0.99, alpha[k]))
        test_T[k] = np.where(blend, tt, np.nan)
        stop = blend & (tt < 1e-4)
        done |= stop
        go = blend & ~stop
        T = np.where(go, tt, T)
        ncon[go] = k + 1
    return alpha, power, test_T, ncon


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_meets_its_design(name):
    e = SCENES[name]
    s = e.scene
    W = s.cam.W
    use_sh = s.shs is not None
    fr, _ = harness.run_oracle(s, backward=False, use_sh=use_sh)
    fr64, _ = harness.run_oracle(s, backward=False, use_sh=use_sh, dtype=np.float64)
    for f in (fr, fr64):
        # the oracle's per-tile lists are the designed ones, entry for entry
        assert [int(b - a) for a, b in f.ranges] == e.lengths
        for t, (a, b) in enumerate(f.ranges):
            np.testing.assert_array_equal(f.point_list[a:b], e.lists[t])
    assert not fr.clamped.any() and not fr64.clamped.any()
    for t, ids in enumerate(e.lists):
        masks = es.exact_masks(fr64.means2D[ids], fr64.conic_opacity[ids], W, 16, t, 0)
        pc = np.array([bin(int(m)).count("1") for m in masks])
        np.testing.assert_array_equal(pc, e.popcount[ids])
    if not e.render:
        return
    assert not fr.unstable.any() and not fr64.unstable.any()  # every Gaussian is stable: no exclusions
    assert not fr.unstable_pix.any() and not fr64.unstable_pix.any()
    # T steps by about 1 % per entry, so some pixel's T passes close to 0.5; the median depth it picks is one of
    # eight tied values, and the same one in both precisions
    np.testing.assert_array_equal(fr.depth, fr64.depth.astype(np.float32))
    X, Y, _ = es.block_of_pixel()
    for t in range(len(e.lists)):
        alpha, power, test_T, ncon = _walk(fr64, t)
        np.testing.assert_array_equal(ncon, fr64.n_contrib[Y, 16 * t + X])
        np.testing.assert_array_equal(ncon, fr.n_contrib[Y, 16 * t + X])
        assert (power <= 0).all()
        assert (((alpha >= 2 / 255) & (alpha <= 0.97)) | (alpha < 0.5 / 255)).all()
        if e.n_contrib is None:
            assert not (test_T < 2e-4).any()  # no pixel runs out of transmittance
            assert ncon.max() == len(e.lists[t])
        else:
            assert (ncon == e.n_contrib).all()
            assert (test_T[:e.n_contrib] >= 2e-4).all()
            assert (test_T[e.n_contrib] <= 5e-5).all()
            assert np.isnan(test_T[e.n_contrib + 1:]).all()  # the tail behind the blocker blends nowhere
            assert len(e.lists[t]) > e.n_contrib + 1
        if t == 0 and e.batches:
            back = e.popcount[e.lists[0][:ncon.max()][::-1]]
            variant = name[len("bwd_"):]
            variant = next(v for v in sorted(es.BUDGETS, key=len, reverse=True) if variant.startswith(v + "_"))
            assert es.cut_batches(list(back), *es.BUDGETS[variant]) == e.batches


def _define(text, name):
    m = re.search(r"#define\s+" + name + r"\s+(.+?)\s*(?://.*)?$", text, re.M)
    assert m, name
    return m.group(1)


def test_budget_table_matches_sources():
    """edge_scenes.BUDGETS restates the kernels' batch sizes and slot budgets: read the defaults out of the
    sources, so that a retuned budget cannot leave the edge scenes beside their edges unnoticed."""
    csrc = os.path.join(ROOT, "splatam_amd", "csrc")
    bwd = open(os.path.join(csrc, "gsr_render_bwd.h")).read()
    pw = open(os.path.join(csrc, "gsr_backward_power.hip")).read()
    common = open(os.path.join(csrc, "gsr_layout.h")).read()
    BB = int(_define(bwd, "GSR_BWD_BB"))
    WBB = int(_define(bwd, "GSR_BWD_WBB"))
    WBS = int(_define(bwd, "GSR_BWD_WBS"))
    bs = _define(bwd, "GSR_BWD_BS")
    assert bs == "(4 * GSR_BWD_BB)", bs
    BS = 4 * BB
    m = re.search(r"constexpr int bwd_batch\(\) \{ return MOM \? (\d+) : \(NV <= 6 \? GSR_BWD_BB : GSR_BWD_WBB\); \}", bwd)
    assert m
    MBB = int(m.group(1))
    m = re.search(r"constexpr int bwd_slots\(\) \{ return MOM == 1 \? (\d+) : \(MOM == 2 \? (\d+) : "
                  r"\(NV <= 6 \? GSR_BWD_BS : GSR_BWD_WBS\)\); \}", bwd)
    assert m
    M1, M2 = int(m.group(1)), int(m.group(2))
    m = re.search(r"static constexpr int BATCH = NSH >= 9 \? (\d+) : (\d+);", pw)
    assert m
    P9, P0 = int(m.group(1)), int(m.group(2))
    m = re.search(r"constexpr int NV = 4, BB = (\d+), BS = (\d+) \* BB,", pw)
    assert m
    FBB, FBS = int(m.group(1)), int(m.group(1)) * int(m.group(2))
    got = {"wide": (WBB, WBS), "wide_dual": (WBB, WBS), "tracking": (BB, BS), "mom1": (MBB, M1), "mom2": (MBB, M2),
           "power_sh0": (P0, None), "power_sh3": (P9, None), "fisher": (FBB, FBS)}
    assert got == es.BUDGETS
    assert int(re.search(r"constexpr int RENDER_BATCH = (\d+);", common).group(1)) == es.RENDER_BATCH
    assert int(re.search(r"constexpr int TILE_SORT_CAP = (\d+);", common).group(1)) == es.TILE_SORT_CAP
    # every sort branch edge and both sides of the cap are among the sort lengths
    for edge in (1, 256, 512, 1024, 2048, 3072, es.TILE_SORT_CAP):
        assert edge in es.SORT_LENGTHS and edge + 1 in es.SORT_LENGTHS
