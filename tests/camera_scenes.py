"""Constructed scenes whose Gaussians are placed in named camera branches, not drawn into them
(tests/test_camera_scenes_cpu.py checks the construction and pins the references on it,
tests/test_gpu_camera.py compares the rasterizer with the oracle class by class).

The image is 64x48 with the Replica intrinsics (fx = 32, tanfovx = 1).  Every Gaussian is laid out in
the camera frame and moved to the world frame with p_w = R^T (p_c - t); the camera is
setup_camera(..., w2c=[R|t]); the quaternions are world-frame values and are used as they are.  Two poses:

  posed     R = Rx(20) Ry(-35) Rz(50) (degrees), t = (0.3, -0.2, 0.5): nine distinct non-zero rotation
            entries, campos != 0;
  identity  the control that separates a camera bug from a branch bug (same camera-frame layout).

Classes (`classes[name]` is a bool mask over the P Gaussians):

  body      200 Gaussians as make_scene draws them: occlusion and ordinary gradients;
  clamp_x / clamp_y / clamp_xy
            t.x/t.z and / or t.y/t.z at +-1.5 tanfov (the reference clamps at +-1.3: forward.cu:82-87,
            backward.cu:175-176), both signs, the other axis inside the image; 2D sigma about 8 px, so
            each reaches image pixels with alpha >= 1/255 from 12-16 px outside;
  edge_in   the same three placements at +-1.25 tanfov: off screen, not clamped;
  near      z in [0.05, 0.15] (the reference culls at z <= 0.001, upstream 3DGS at 0.2), scale 3 z / fx;
  culled    z = 0.0005, z = -1, and centres at +-3 tanfov with 2D sigma about 1 px (the rect covers no tile);
  opaque    opacity cycling through 0.99, 0.995, 1.0, 2D sigma about 4 px, centred on a pixel centre: the
            members above 0.99 have o G > 0.99 there (alpha = min(0.99, o G) is clamped), the 0.99 members
            sit on the clamp's edge (o G <= 0.99 everywhere: the clamp must not change them);
  sh_clamp  (SH scenes) DC coefficients solved so that channels `SH_CLAMP_BITS[k % 7]` evaluate to
            -0.05 - U(0, 0.3) and the other channels to 0.05 + U(0.05, 0.5).

SH rest coefficients are 0.1 randn for degrees 1 to 3.  The placements above are footprints, so a scene
built for scale_modifier m stores the placed classes' scales divided by m (the body's are left to grow and
shrink with m); dL/dscale is still taken through m * scale in every class.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from dense_ref import SH_C0, eval_sh
from splatam_amd.scenes import Scene, make_scene, replica_intrinsics, setup_camera

W, H = 64, 48
N_BODY = 200
N_CLASS = 12     # members of every placed class
N_OPAQUE = 15    # five of each opacity
OPAQUE_CYCLE = (0.99, 0.995, 1.0)
SH_CLAMP_BITS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
CLAMP_AT, EDGE_AT, CULL_AT, LIMIT = 1.5, 1.25, 3.0, 1.3
# One near-threshold pixel under a 16 px footprint marks every large Gaussian over it unstable, so the caps of
# test_camera_scenes_cpu.py::test_stability_caps hold only where no such pixel falls under the placed classes:
# the first seed of 0..39 at which every case meets them (about one seed in three does for a single case).
SEED = 2


def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose_matrix(pose):
    """[4,4] float64 world-to-camera matrix of a named pose."""
    w2c = np.eye(4)
    if pose == "posed":
        w2c[:3, :3] = _rot(0, 20.0) @ _rot(1, -35.0) @ _rot(2, 50.0)
        w2c[:3, 3] = (0.3, -0.2, 0.5)
    elif pose != "identity":
        raise ValueError(pose)
    return w2c


def camera_arrays(w2c):
    """view, proj, campos in float64 (setup_camera restated without its float32 cast: the pose-equivariance
    test needs a rotation that is orthogonal to 1e-16), and tanfovx, tanfovy."""
    fx, fy, cx, cy = replica_intrinsics(W, H)
    near, far = 0.01, 100.0
    gl = np.array([[2 * fx / W, 0.0, -(W - 2 * cx) / W, 0.0],
                   [0.0, 2 * fy / H, -(H - 2 * cy) / H, 0.0],
                   [0.0, 0.0, far / (far - near), -(far * near) / (far - near)],
                   [0.0, 0.0, 1.0, 0.0]])
    view = w2c.T
    return dict(view=view, proj=view @ gl.T, campos=np.linalg.inv(w2c)[:3, 3], tanfovx=W / (2 * fx),
                tanfovy=H / (2 * fy))


def _off_axis(rs, n, at, tanx, tany, which):
    """t.x/t.z, t.y/t.z of n members: the axes of `which` ("x", "y", "xy") at +-at tanfov (signs alternate, the
    xy members go through all four corners), the other axis inside 0.8 tanfov."""
    k = np.arange(n)
    sx, sy = np.where(k % 2 == 0, 1.0, -1.0), np.where((k // 2) % 2 == 0, 1.0, -1.0)
    ax = sx * at * tanx if "x" in which else rs.uniform(-0.8, 0.8, n) * tanx
    ay = (sy if which == "xy" else sx) * at * tany if "y" in which else rs.uniform(-0.8, 0.8, n) * tany
    return ax, ay


@functools.lru_cache(maxsize=None)
def layout(aniso=True, sh_degree=0, seed=SEED):
    """The camera-frame layout (float64 numpy): means, scales, rotations, opacities, colors, and the classes."""
    fx, fy, cx, cy = replica_intrinsics(W, H)
    tanx, tany = W / (2 * fx), H / (2 * fy)
    rs = np.random.RandomState(1000 + seed)
    body = make_scene(N_BODY, W, H, seed=seed, anisotropic=aniso)
    parts, names = [], []

    def add(name, ax, ay, z, sigma_px, opac):
        n = len(z)
        m = np.stack([ax * z, ay * z, z], 1)
        s = np.repeat((sigma_px * np.abs(z) / fx)[:, None], 3, 1)
        parts.append((m, s, np.broadcast_to(np.asarray(opac, np.float64), (n,)).copy()))
        names.extend([name] * n)

    for which in ("x", "y", "xy"):
        ax, ay = _off_axis(rs, N_CLASS, CLAMP_AT, tanx, tany, which)
        add("clamp_" + which, ax, ay, rs.uniform(2.0, 4.0, N_CLASS), np.full(N_CLASS, 8.0), rs.uniform(0.3, 0.6, N_CLASS))
    ax, ay = zip(*(_off_axis(rs, N_CLASS // 3, EDGE_AT, tanx, tany, w) for w in ("x", "y", "xy")))
    add("edge_in", np.concatenate(ax), np.concatenate(ay), rs.uniform(2.0, 4.0, N_CLASS), np.full(N_CLASS, 8.0),
        rs.uniform(0.3, 0.6, N_CLASS))
    # pixel (u, v) <-> t.x/t.z = (u - cx + 0.5) / fx (the projection of setup_camera with ndc2pix)
    pix = lambda u, v: ((u - cx + 0.5) / fx, (v - cy + 0.5) / fy)  # noqa: E731
    ax, ay = pix(rs.uniform(4, W - 4, N_CLASS), rs.uniform(4, H - 4, N_CLASS))
    add("near", ax, ay, np.linspace(0.05, 0.15, N_CLASS), np.full(N_CLASS, 3.0), rs.uniform(0.3, 0.6, N_CLASS))
    n3 = N_CLASS // 3
    ax, ay = pix(rs.uniform(4, W - 4, 2 * n3), rs.uniform(4, H - 4, 2 * n3))
    add("culled", ax, ay, np.array([0.0005] * n3 + [-1.0] * n3), np.full(2 * n3, 3.0), rs.uniform(0.3, 0.9, 2 * n3))
    ax, ay = _off_axis(rs, N_CLASS - 2 * n3, CULL_AT, tanx, tany, "x")
    ax2, ay2 = _off_axis(rs, N_CLASS - 2 * n3, CULL_AT, tanx, tany, "y")
    k = np.arange(N_CLASS - 2 * n3) < (N_CLASS - 2 * n3) // 2
    add("culled", np.where(k, ax, ax2), np.where(k, ay, ay2), rs.uniform(1.0, 3.0, len(k)), np.full(len(k), 1.0),
        rs.uniform(0.3, 0.9, len(k)))
    ax, ay = pix(rs.randint(4, W - 4, N_OPAQUE).astype(np.float64), rs.randint(4, H - 4, N_OPAQUE).astype(np.float64))
    add("opaque", ax, ay, rs.uniform(0.6, 1.0, N_OPAQUE), np.full(N_OPAQUE, 4.0),
        [OPAQUE_CYCLE[i % 3] for i in range(N_OPAQUE)])
    if sh_degree > 0:
        ax, ay = pix(rs.uniform(4, W - 4, N_CLASS), rs.uniform(4, H - 4, N_CLASS))
        add("sh_clamp", ax, ay, rs.uniform(0.6, 1.5, N_CLASS), np.full(N_CLASS, 2.0), rs.uniform(0.4, 0.8, N_CLASS))

    means = np.concatenate([body.means3D.double().numpy()] + [p[0] for p in parts])
    scales = np.concatenate([body.scales.double().numpy()] + [p[1] for p in parts])
    opac = np.concatenate([body.opacities.double().numpy()[:, 0]] + [p[2] for p in parts])
    P, n_new = len(means), len(names)
    rot = np.zeros((P, 4))
    rot[:, 0] = 1.0
    rot[:N_BODY] = body.rotations.double().numpy()
    if aniso:
        scales[N_BODY:] *= np.exp(0.25 * rs.randn(n_new, 3))
        q = rs.randn(n_new, 4)
        rot[N_BODY:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    colors = np.concatenate([body.colors.double().numpy(), rs.uniform(0.2, 0.8, (n_new, 3))])
    cls = np.array(["body"] * N_BODY + names)
    classes = {n: cls == n for n in dict.fromkeys(cls)}
    return dict(means=means, scales=scales, rotations=rot, opacities=opac, colors=colors, classes=classes)


def to_world(means_c, w2c):
    """p_w = R^T (p_c - t), solved (not transposed) so that a rounded R gives the camera-frame point back."""
    return np.linalg.solve(w2c[:3, :3], (means_c - w2c[:3, 3]).T).T


@functools.lru_cache(maxsize=None)
def build(pose="posed", aniso=True, sh_degree=0, mod=1.0, seed=SEED):
    """The Scene (float32, world frame) of a pose and the classes dict (name -> bool mask [P]).
    mod: the scale_modifier the scene will be rendered with; the placed classes' scales are divided by it,
    so that their footprints (which the placements are stated in) are those of the layout under every
    modifier, while the body's grow and shrink with it.
    sh_clamp members: `sh_clamp_bits(classes)` gives their designed clamped bits."""
    L = layout(aniso, sh_degree, seed)
    fx, fy, cx, cy = replica_intrinsics(W, H)
    w2c = pose_matrix(pose)
    cam = setup_camera(W, H, fx, fy, cx, cy, w2c=torch.tensor(w2c, dtype=torch.float32))
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32)  # noqa: E731
    means = f32(to_world(L["means"], w2c))
    classes = L["classes"]
    shs = None
    if sh_degree > 0:
        rs = np.random.RandomState(2000 + seed)
        P, M = len(means), (sh_degree + 1) ** 2
        sh = 0.1 * rs.randn(P, M, 3)
        sh[:, 0] = (L["colors"] - 0.5) / SH_C0
        ids = np.nonzero(classes["sh_clamp"])[0]
        bits = sh_clamp_bits(classes)
        target = np.where(bits, -0.05 - rs.uniform(0.0, 0.3, bits.shape), 0.05 + rs.uniform(0.05, 0.5, bits.shape))
        # the colour of the float32 inputs without the DC term, as the rasterizer will evaluate it
        d = means[ids].double() - cam.campos.double()[None]
        d = d / d.norm(dim=1, keepdim=True)
        rest = torch.tensor(sh[ids]).float().double()
        rest[:, 0] = 0.0
        sh[ids, 0] = (target - eval_sh(sh_degree, rest, d).numpy()) / SH_C0
        shs = f32(sh)
    scales = L["scales"].copy()
    scales[N_BODY:] /= mod
    scene = Scene(means3D=means, scales=f32(scales), rotations=f32(L["rotations"]),
                  opacities=f32(L["opacities"][:, None]), colors=f32(L["colors"]), shs=shs, sh_degree=sh_degree, cam=cam)
    return scene, classes


def sh_clamp_bits(classes):
    """[n,3] designed clamped bits of the sh_clamp members, in id order."""
    n = int(classes["sh_clamp"].sum())
    return np.array([SH_CLAMP_BITS[k % len(SH_CLAMP_BITS)] for k in range(n)], bool)


# The cases of tests/test_gpu_camera.py; the power-1 ones are also the cases on which
# tests/test_camera_scenes_cpu.py pins the oracle against autograd.
CASES = [
    dict(name="posed_aniso", pose="posed", aniso=True, sh=0, mod=1.0),
    dict(name="posed_aniso_mod1.7", pose="posed", aniso=True, sh=0, mod=1.7),
    dict(name="posed_aniso_mod0.5", pose="posed", aniso=True, sh=0, mod=0.5),
    dict(name="posed_cov3D_bg", pose="posed", aniso=True, sh=0, mod=1.0, cov=True, bg=(0.2, 0.5, 0.9)),
    dict(name="posed_sh1", pose="posed", aniso=True, sh=1, mod=1.0),
    dict(name="posed_sh2_mod1.7", pose="posed", aniso=True, sh=2, mod=1.7),
    dict(name="posed_sh3", pose="posed", aniso=True, sh=3, mod=1.0),
    dict(name="posed_iso", pose="posed", aniso=False, sh=0, mod=1.0),
    dict(name="identity_aniso_mod1.7", pose="identity", aniso=True, sh=0, mod=1.7),
    dict(name="posed_aniso_power2", pose="posed", aniso=True, sh=0, mod=1.0, power=2),
    dict(name="posed_sh3_power2", pose="posed", aniso=True, sh=3, mod=1.0, power=2),
]
POWER1_CASES = [c for c in CASES if c.get("power", 1) == 1]


def case_scene(case):
    return build(case["pose"], case["aniso"], case["sh"], 1.0 if case.get("cov") else case["mod"])


def run_kwargs(case):
    """The arguments harness.run_oracle / harness.run_gpu take for a case."""
    return dict(bg=case.get("bg", (0.0, 0.0, 0.0)), use_sh=case["sh"] > 0, use_cov=case.get("cov", False),
                power=case.get("power", 1), scale_modifier=case["mod"])


@functools.lru_cache(maxsize=None)
def upstream_grad():
    """dL/dcolor of every case ([3,H,W] float32)."""
    return np.random.RandomState(7).randn(3, H, W).astype(np.float32)
