"""Generates tests/golden/matrix_to_quaternion.npz by importing the REFERENCE's own matrix_to_quaternion
(utils/slam_helpers.py:43-103) on the CPU.  Never run by a test.  Run:
    python tests/golden/make_matrix_to_quaternion.py <path of the reference checkout>

What is captured:
  * matrices [K,3,3] float32: the identity, a small rotation, 180 degree rotations about x, y, z and about a
    general axis, rotations a hair short of 180 degrees about axes led by x, by y and by z (one per branch
    of the best-conditioned choice: r, i, j, k largest), 120 degrees about (1,1,1) (all four candidates tie:
    argmax takes the first) and seeded random rotations;
  * quaternions [K,4] float32: the reference's output on them, float32 on the CPU;
  * branch [K]: the reference's q_abs.argmax, recomputed here (every value 0..3 must occur);
  * tol: the largest |float32 output - the reference's own float64 evaluation of the same float32 matrices|
    plus one float32 ulp at 1 (2^-23; |q| <= 1): the float32 rounding of this formula on these inputs.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "matrix_to_quaternion.npz")


def axis_angle(axis, deg: float) -> np.ndarray:
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def matrices() -> np.ndarray:
    rng = np.random.RandomState(20)
    ms = [np.eye(3), axis_angle((0.3, -0.5, 0.8), 0.3),
          axis_angle((1, 0, 0), 180.0), axis_angle((0, 1, 0), 180.0), axis_angle((0, 0, 1), 180.0),
          axis_angle((1, 2, 3), 180.0),
          axis_angle((5, 1, 2), 179.9), axis_angle((1, 5, 2), 179.9), axis_angle((1, 2, 5), 179.9),
          axis_angle((1, 1, 1), 120.0)]
    for _ in range(22):
        ms.append(axis_angle(rng.standard_normal(3), rng.uniform(0.0, 180.0)))
    return np.stack(ms).astype(np.float32)


def main(ref_root: str):
    sys.path.insert(0, ref_root)
    from utils.slam_helpers import matrix_to_quaternion
    m = torch.from_numpy(matrices())
    q32 = matrix_to_quaternion(m)
    q64 = matrix_to_quaternion(m.double())
    assert q32.dtype == torch.float32 and q64.dtype == torch.float64
    own = float((q32.double() - q64).abs().max())
    tol = own + 2.0 ** -23
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    branch = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                          1.0 - m00 - m11 + m22], dim=-1).clamp_min(0).sqrt().argmax(dim=-1)
    assert set(branch.tolist()) == {0, 1, 2, 3}, branch
    np.savez(OUT, matrices=m.numpy(), quaternions=q32.numpy(), branch=branch.numpy().astype(np.int64),
             tol=np.float64(tol))
    print(f"{OUT}: {m.shape[0]} rotations, branches {np.bincount(branch.numpy()).tolist()}, "
          f"float32 against float64 {own:.3e}, tol {tol!r}")


if __name__ == "__main__":
    main(sys.argv[1])
