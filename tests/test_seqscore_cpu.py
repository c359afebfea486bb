"""The view scorer of a running sequence, the part that needs no device: the refusals of the two new C entry
points (gsr_fisher_score, gsr_forward_static_alive: return code and gsr_last_error text, before any HIP call;
small host buffers stand in for device memory, these checks never dereference them), the numpy restatement
tests/test_gpu_seqscore.py compares the kernel with, and the Python layer's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from splatam_amd._lib import ALLOC_FN, SIGNATURES, GsrGaussians, GsrSettings, lib

INVALID = -1
_BUF = (ctypes.c_double * 64)()
D = (ctypes.addressof(_BUF) + 15) // 16 * 16  # non-null, 16-byte aligned, never dereferenced


def restate_score(dmeans, dopac, hinv, alive=None):
    """gsr_fisher_score's contract in numpy: the float32 products of [dmeans, dopac] and hinv over the selected
    rows (alive != 0; every row for None), summed in float64."""
    H = np.concatenate([np.asarray(dmeans, np.float32).reshape(-1, 3), np.asarray(dopac, np.float32).reshape(-1, 1)], 1)
    sel = np.ones(H.shape[0], bool) if alive is None else np.asarray(alive).reshape(-1) != 0
    prod = (H[sel] * np.asarray(hinv, np.float32).reshape(-1, 4)[sel]).astype(np.float32)
    return float(prod.astype(np.float64).sum())


def _score(P=4, dm=D, dop=D, hinv=D, alive=None, ws=D, out=D):
    rc = lib.gsr_fisher_score(P, dm, dop, hinv, alive, ws, out, None)
    return rc, lib.gsr_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(P=-1), "fisher_score: P must be >= 0"),
    (dict(out=None), "fisher_score: null out pointer"),
    (dict(P=0, out=None), "fisher_score: null out pointer"),
    (dict(P=-1, out=None), "fisher_score: P must be >= 0"),           # the size is checked first
    (dict(out=D + 4), "fisher_score: out must be 8-byte aligned"),
    (dict(dm=None), "fisher_score: null pointer"),
    (dict(dop=None), "fisher_score: null pointer"),
    (dict(hinv=None), "fisher_score: null pointer"),
    (dict(ws=None), "fisher_score: null pointer"),
    (dict(hinv=D + 8), "fisher_score: H_inv and workspace must be 16-byte aligned"),
    (dict(ws=D + 8), "fisher_score: H_inv and workspace must be 16-byte aligned"),
])
def test_fisher_score_refusals(kw, msg):
    rc, err = _score(**kw)
    assert rc == INVALID and err == msg


def test_fisher_score_workspace_is_a_constant_that_holds_the_grid():
    n = lib.gsr_fisher_score_workspace_bytes()
    assert n == 128 + 8 * 256  # the counter's head, one float64 partial per workgroup of the bounded grid
    assert len(SIGNATURES["gsr_fisher_score"][1]) == 8


@ALLOC_FN
def _no_memory(ctx, kind, nbytes):  # (never reached by a refused call)
    return None


def _static_alive(P=4, capacity=64, status=D, alive=D):
    s = GsrSettings(image_height=32, image_width=48, tan_fovx=1.0, tan_fovy=1.0, bg=D, scale_modifier=1.0, viewmatrix=D,
                    projmatrix=D, sh_degree=0, campos=D, prefiltered=0, binning=0)
    g = GsrGaussians(P=P, M=0, means3D=D, shs=None, colors_precomp=D, opacities=D, scales=D, rotations=D,
                     cov3D_precomp=None)
    rc = lib.gsr_forward_static_alive(ctypes.byref(s), ctypes.byref(g), capacity, status, D, D, D, alive, _no_memory,
                                      None, None)
    return rc, lib.gsr_last_error().decode()


def test_forward_static_alive_refusals():
    """The dual form's refusals (tests/test_capi_refusals_cpu.py), in its order: static mode, then the mask."""
    assert _static_alive(alive=None) == (INVALID, "alive mask required")
    assert _static_alive(capacity=0) == (INVALID, "static mode needs capacity > 0 and status")
    assert _static_alive(status=None) == (INVALID, "static mode needs capacity > 0 and status")
    assert _static_alive(capacity=0, alive=None) == (INVALID, "static mode needs capacity > 0 and status")
    assert _static_alive(P=-1) == (INVALID, "P must be >= 0")
    sig, dual = SIGNATURES["gsr_forward_static_alive"][1], SIGNATURES["gsr_forward_dual_static_alive"][1]
    assert len(sig) == len(SIGNATURES["gsr_forward_static"][1]) + 1 == len(dual) - 2


def test_binding_refuses_the_mask_without_the_static_forward():
    from splatam_amd import _C
    z, e = torch.zeros(4, 3), torch.Tensor([])
    with pytest.raises(RuntimeError, match="need the static"):  # the dual form's error
        _C.rasterize_gaussians(torch.zeros(3), z, z, torch.zeros(4, 1), z, torch.zeros(4, 4), 1.0, e, torch.eye(4)[None],
                               torch.eye(4)[None], 1.0, 1.0, 8, 8, e, 0, torch.zeros(3), False,
                               alive=torch.ones(4, dtype=torch.uint8))


def test_restatement():
    """Float32 products, float64 sum, dead rows selected out (their NaN does not reach the sum)."""
    dm = np.array([[1, 2, 3], [4, 5, 6], [np.nan, np.nan, np.nan]], np.float32)
    dop = np.array([[0.5], [0.25], [np.nan]], np.float32)
    hinv = np.array([[1, 1, 1, 2], [0.1, 0, 1, 4], [np.nan] * 4], np.float32)
    alive = np.array([1, 1, 0], np.uint8)
    want = 1 + 2 + 3 + 1 + float(np.float32(4) * np.float32(0.1)) + 0 + 6 + 1
    assert restate_score(dm, dop, hinv, alive) == want
    assert np.isnan(restate_score(dm, dop, hinv))
    assert restate_score(dm[:0], dop[:0], hinv[:0]) == 0.0
    assert restate_score(dm, dop, hinv, np.zeros(3, np.uint8)) == 0.0
    # the product is rounded to float32 before it is widened: 0.1f * 3f is not the double product
    a, b = np.float32(0.1), np.float32(3.0)
    assert restate_score([[a, 0, 0]], [[0]], [[b, 0, 0, 0]]) == float(np.float32(a * b)) != float(a) * float(b)


def _params(P, scale_cols=1):
    return {"means3D": torch.zeros(P, 3), "rgb_colors": torch.zeros(P, 3), "unnorm_rotations": torch.zeros(P, 4),
            "logit_opacities": torch.zeros(P, 1), "log_scales": torch.zeros(P, scale_cols)}


def test_sequence_fisher_argument_checks():
    from splatam_amd.fisher import SequenceFisher
    alive = torch.ones(5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="mode is"):
        SequenceFisher(_params(5), alive, None, 4, "mean", 1000)
    with pytest.raises(ValueError, match="isotropic"):  # BatchedFisher's rule
        SequenceFisher(_params(5, 3), alive, None, 4, "gains", 1000)
    with pytest.raises(ValueError, match="bin_capacity > 0"):
        SequenceFisher(_params(5), alive, None, 4, "sum", 0)
    with pytest.raises(RuntimeError, match="ROCm devices only"):  # no CPU fallback
        SequenceFisher(_params(5), alive, None, 4, "sum", 1000)


def test_view_scorer_stream_is_its_own():
    """ViewScorer draws from RandomState(seed) of its own: the same seed repeats the choice, and no global or
    sequence stream is consumed."""
    from splatam_amd.sequence import ViewScorer
    state = np.random.get_state()[1].copy()
    a, b = ViewScorer(4, 2, seed=5), ViewScorer(4, 2, seed=5)
    ia = [int(i) for i in a.rng.choice(3, size=2, replace=False)]
    ib = [int(i) for i in b.rng.choice(3, size=2, replace=False)]
    assert ia == ib and len(set(ia)) == 2
    assert np.array_equal(np.random.get_state()[1], state)
    assert (a.n_monte, a.K, a.fitted, a.stale, a.used) == (2, 4, False, False, [])
