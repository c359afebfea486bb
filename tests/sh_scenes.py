"""Scenes for the spherical-harmonics colour paths (tests/test_sh_paths_cpu.py pins the oracle on them,
tests/test_gpu_sh_paths.py compares the rasterizer with it).

The rasterizer has two SH implementations.  With M == (D+1)^2 stored coefficients per Gaussian the
staged kernels of csrc/gsr_sh.hip run (64-, 256- and 128-Gaussian blocks moved through LDS); with
M > (D+1)^2 -- the way 3DGS callers ramp active_sh_degree over 16 stored coefficients -- every lane
reads its own row at stride 3 M inside preprocess and gauss_chain, and the backward has to zero the
3 (M - (D+1)^2) unused gradient entries itself.

  padded(scene, M, poison)   the same scene with its coefficient rows widened to M; the extra
                             coefficients are NaN or +-1e30, so anything that reads them shows;
  degree0(scene)             active degree 0 (DC term only, M = 1) of a Scene or of a
                             camera_scenes.build (scene, classes) pair;
  PAIRS                      the (D, M) table of the per-lane path;
  posed(D, M, poison)        camera_scenes.build("posed", True, max(D, 1), 1.0) at degree D, padded to M;
  EDGE_P, edge_scene(P, D)   make_scene at the staged kernels' block edges.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import camera_scenes as cs
from dense_ref import SH_C0
from splatam_amd.scenes import Scene, make_scene

W, H = cs.W, cs.H

# (active degree D, stored coefficients M > (D+1)^2)
PAIRS = ((0, 4), (0, 16), (1, 9), (1, 16), (2, 16), (3, 25))
PAIR_IDS = [f"D{d}_M{m}" for d, m in PAIRS]

# sh_eval_kernel works in 64-Gaussian blocks, sh_bwd_kernel in 256, sh_bwd_split_kernel in 128: below one block,
# exact multiples (no ragged block), each boundary +-1, and two full blocks plus one row (513)
EDGE_P = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)


def nsh(D):
    return (D + 1) ** 2


def padded(scene, M, poison="nan"):
    """`scene` with shs widened from [P, (D+1)^2, 3] to [P, M, 3]; sh_degree unchanged.  The extra
    coefficients are NaN (poison="nan") or +-1e30 with alternating signs (poison="big")."""
    n = nsh(scene.sh_degree)
    assert scene.shs is not None and scene.shs.shape[1] == n and M >= n, (scene.shs.shape, M)
    P = scene.P
    if poison == "nan":
        tail = torch.full((P, M - n, 3), float("nan"))
    elif poison == "big":
        sign = 1.0 - 2.0 * (torch.arange(P * (M - n) * 3) % 2).float()
        tail = (1e30 * sign).reshape(P, M - n, 3)
    else:
        raise ValueError(poison)
    return dataclasses.replace(scene, shs=torch.cat([scene.shs, tail], 1).contiguous())


def degree0(scene_or_layout):
    """The SH scene of active degree 0: shs[:, 0] = (colour - 0.5) / SH_C0, M = 1.

    A Scene gives a Scene.  A (scene, classes) pair of camera_scenes.build at degree 1 (camera_scenes.layout
    creates the sh_clamp class only for sh_degree > 0) gives the pair back with the higher coefficients
    dropped; the sh_clamp members' DC terms are then set directly so that the channels of
    camera_scenes.SH_CLAMP_BITS evaluate to -0.05 - U(0, 0.3) and the others to 0.05 + U(0.05, 0.5): the
    targets of camera_scenes.build, reached with the DC term alone."""
    if isinstance(scene_or_layout, Scene):
        scene, classes = scene_or_layout, None
    else:
        scene, classes = scene_or_layout
    dc = (scene.colors.double().numpy() - 0.5) / SH_C0
    if classes is not None and "sh_clamp" in classes:
        rs = np.random.RandomState(3000 + cs.SEED)
        bits = cs.sh_clamp_bits(classes)
        target = np.where(bits, -0.05 - rs.uniform(0.0, 0.3, bits.shape), 0.05 + rs.uniform(0.05, 0.5, bits.shape))
        dc[np.nonzero(classes["sh_clamp"])[0]] = (target - 0.5) / SH_C0
    out = dataclasses.replace(scene, shs=torch.tensor(dc[:, None, :], dtype=torch.float32).contiguous(), sh_degree=0)
    return out if classes is None else (out, classes)


@functools.lru_cache(maxsize=None)
def posed(D, M=None, poison="nan"):
    """(scene, classes) of the posed anisotropic camera scene at active degree D with M stored coefficients
    (None or (D+1)^2: unpadded).  Padding changes no colour, so the construction and the near-threshold caps
    that tests/test_camera_scenes_cpu.py checks on the unpadded scenes carry over."""
    scene, classes = cs.build("posed", True, max(D, 1), 1.0)
    if D == 0:
        scene, classes = degree0((scene, classes))
    if M is not None and M != nsh(D):
        scene = padded(scene, M, poison)
    return scene, classes


# edge_scene seeds.  make_scene draws every centre inside the image, at z in [0.5, 5] with a radius of at
# least 2 px, so every Gaussian it draws is visible; the culled rows (radius 0: their gradient rows must be
# exactly zero and sh_bwd zero-fills their LDS rows) are made by mirroring the Gaussians i % 5 == 2 behind
# the camera.  Per P, the seed is the first of 0..19 at which, for every degree 0..3, the float32 oracle finds
# at least one Gaussian with radii > 0 and -- for P >= 63 -- one with radii == 0, renders at least one pixel,
# agrees with the float64 build on every radius, and neither build flags a near-threshold pixel or Gaussian
# (tests/test_sh_paths_cpu.py::test_edge_scenes_have_visible_and_culled_rows checks all of this again), so
# that the forward and gradient criteria apply to every pixel and every row.
EDGE_SEEDS = {1: 0, 63: 0, 64: 0, 65: 0, 127: 1, 128: 0, 129: 1, 255: 3, 256: 4, 257: 0, 513: 2}


def culled_rows(P):
    """The rows edge_scene puts behind the camera."""
    return np.arange(P) % 5 == 2


@functools.lru_cache(maxsize=None)
def edge_scene(P, D, seed=None):
    """make_scene(P, 64, 48, anisotropic=True, sh_degree=D) at the seed of EDGE_SEEDS (degree0 of it for
    D == 0), with the rows of culled_rows(P) mirrored behind the camera; M = (D+1)^2."""
    s = EDGE_SEEDS[P] if seed is None else seed
    scene = make_scene(P, W, H, seed=s, anisotropic=True, sh_degree=D)
    if D == 0:
        scene = degree0(scene)
    means = scene.means3D.clone()
    means[torch.as_tensor(culled_rows(P)), 2] *= -1.0
    return dataclasses.replace(scene, means3D=means)


@functools.lru_cache(maxsize=None)
def upstream_grad():
    return cs.upstream_grad()
