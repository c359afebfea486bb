"""splatam_amd.keyframes.select_literal (the overlap keyframe selection in plain torch ops, the comparison
form of the device kernels) on CPU tensors against the float64 numpy restatement of tests/keyframe_ref.py:
sampled pixels, n_points, the window and the draws exactly, every overlap count within the restatement's
[sure, sure + borderline] band."""
import numpy as np
import pytest
import torch

import keyframe_ref as kr
from splatam_amd import keyframes as kfm


def _run(c, ref=None):
    ref = kr.restate(c) if ref is None else ref
    assert ref["borderline"].max(initial=0) <= 0.01 * ref["S"]
    out = kfm.select_literal(*kr.to_torch(c, "cpu"))
    kr.check(out, ref)
    return out, ref


def _word_for_rank(rank, n_valid):
    u = ((rank << 32) + n_valid - 1) // n_valid
    assert (u * n_valid) >> 32 == rank and u < 1 << 32
    return u


@pytest.mark.parametrize("n_kf", [0, 1, 2, 9])
@pytest.mark.parametrize("S", [1, 65, 400])
def test_literal_matches_restatement(n_kf, S):
    out, ref = _run(*kr.make_valid_case(100, 75, S, n_kf, seed=100 * n_kf + S, zero_rows=(0, 30, -1)))
    assert ref["n_window"] == min(ref["n_eligible"], 3) + (n_kf > 0) + 1
    assert out["overlap"].dtype == torch.int32 and out["draw_rows"].dtype == torch.int64


def test_more_and_fewer_eligible_than_k_select():
    c, ref = kr.make_valid_case(96, 64, 300, 13, seed=3, k_select=2)
    _run(c, ref)
    assert ref["n_eligible"] > 2 and ref["n_window"] == 4
    c, ref = kr.make_valid_case(96, 64, 300, 13, seed=3, k_select=11)
    _run(c, ref)
    assert 0 < ref["n_eligible"] < 11 and ref["n_window"] == ref["n_eligible"] + 2


def test_keyframe_facing_away_is_excluded():
    c, ref = kr.make_valid_case(96, 64, 300, 9, seed=4, k_select=8)
    out, ref = _run(c, ref)
    assert ref["n_eligible"] > 0
    for i in (3, 7):  # make_case turns every fourth keyframe by 180 degrees
        assert int(out["overlap"][i]) == 0 and i not in out["window"][:-2].tolist()


def test_duplicate_ranks_drop_every_copy():
    c, _ = kr.make_valid_case(96, 64, 40, 3, seed=5)
    c["u_pix"][7] = c["u_pix"][3]          # the same word
    c["u_pix"][9] = c["u_pix"][3] + 1      # another word, the same rank
    c["u_pix"][20] = c["u_pix"][21]
    out, ref = _run(c)
    n_valid = int((c["depth"] > 0).sum())
    r = (c["u_pix"].astype(np.uint64) * np.uint64(n_valid)) >> np.uint64(32)
    assert r[9] == r[3]
    assert ref["n_points"] == 40 - 5 == int(out["n_points"])


def test_point_at_the_origin_is_dropped():
    W, H = 96, 64
    c, _ = kr.make_valid_case(W, H, 30, 3, seed=6)
    c["intr"] = (80.0, 80.0, 48.0, 32.0)
    c["depth"][32, 48] = 2.0
    c["w2c"] = np.eye(4, dtype=np.float32)
    c["w2c"][2, 3] = 2.0                   # the camera centre at (0, 0, -2): pixel (48, 32) at depth 2 is the origin
    flat = c["depth"].reshape(-1) > 0
    c["u_pix"][11] = _word_for_rank(int(flat[:32 * W + 48].sum()), int(flat.sum()))
    out, ref = _run(c)
    assert int(out["pixels"][11]) == 32 * W + 48
    assert ref["n_points"] == 29 == int(out["n_points"])


@pytest.mark.parametrize("n_kf", [0, 1, 4])
def test_no_valid_depth(n_kf):
    c, _ = kr.make_valid_case(96, 64, 50, n_kf, seed=7)
    c["depth"][:] = 0.0
    out, ref = _run(c)
    assert int(out["n_points"]) == 0 and int(out["overlap"].sum()) == 0
    assert out["window"][:int(out["n_window"])].tolist() == ([n_kf - 1] if n_kf else []) + [c["cur_row"]]
    assert (out["pixels"] == -1).all()


def test_draw_index_ends():
    c, _ = kr.make_valid_case(96, 64, 200, 9, seed=8)
    c["u_draw"][:] = 0
    c["u_draw"][1::2] = 0xFFFFFFFF
    out, ref = _run(c)
    nw = int(out["n_window"])
    assert nw >= 3
    assert out["draw_index"].tolist() == [0, nw - 1] * 6
    assert out["draw_rows"][1].item() == c["cur_row"] and out["draw_times"][1].item() == c["time_idx"]
    first = int(out["window"][0])
    assert out["draw_rows"][0].item() == first and out["draw_times"][0].item() == int(c["kf_time"][first])


def test_header_functions_in_ctypes_table():
    from splatam_amd import _lib
    for name in ("gsr_keyframe_select", "gsr_keyframe_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["gsr_keyframe_select"][1]) == 28
    small, big = _lib.lib.gsr_keyframe_workspace_bytes(64, 1), _lib.lib.gsr_keyframe_workspace_bytes(480, 1600)
    assert 0 < small < big and big >= 16 * 1600 + 4 * (2 * 480 + 1)


def test_policy_argument_is_checked():
    from splatam_amd.sequence import _check_policy
    _check_policy("window", 1)
    _check_policy("overlap", 2)
    with pytest.raises(ValueError):
        _check_policy("overlap", 1)
    with pytest.raises(ValueError):
        _check_policy("nearest", 8)
