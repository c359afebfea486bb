"""A float64 numpy restatement of the overlap keyframe selection (include/gsr_glue.h: gsr_keyframe_select,
steps 1-6) with an error bound for the float32 forms under test, and the synthetic cases the CPU and GPU
keyframe tests share.

The bound.  eps = 2^-24 is float32's unit roundoff; a sum of n rounded terms carries at most n eps of the sum
of their magnitudes (first order; the final factor 2 covers the higher orders).  With C a bound in metres
on |x| + |y| + |z| + |t_0| + |t_1| + |t_2| over the sample and every pose used (rotation entries are <= 1):
  x = (col - cx) / fx * z: 3 roundings -> |dx| <= 3 eps |x|;
  world point w_a = R x + R y + R z + t'_a, t'_a itself 5 roundings: |dw| <= (3 + 4 + 1) eps C = 8 eps C;
  camera point p = m . (w, 1): |dp| <= 3 * 8 eps C + 4 eps C = 28 eps C;
  N = fx p.x + cx p.z: |dN| <= (fx + cx) |dp| + 3 eps (fx + cx) C = 31 eps (fx + cx) C;
  zz = p.z + 1e-5: |dzz| <= 28 eps C + eps |zz| <= 29 eps C;
  u = N / zz: |du| <= |dN| / |zz| + |u| |dzz| / |zz| + eps |u|.
So delta_u = 2 [(31 (fx + cx) + 29 |u|) eps C / |zz| + eps |u|] (v likewise with fy, cy), delta_z = 2 * 29 eps C,
and for the origin test on rint(1e4 w): delta_o = 2 * 1e4 * 8 eps C.  A sample is `sure` inside a keyframe when
every comparison holds by more than its delta, sure outside when one fails by more than its delta, borderline
otherwise."""
import numpy as np

EPS = 2.0 ** -24
EDGE = 20


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _pose(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.astype(np.float32)


def words(rng, n):
    return rng.randint(0, 1 << 32, size=int(n), dtype=np.uint64).astype(np.uint32)


def make_case(W, H, S, n_kf, seed, k_select=3, n_draws=12, zero_rows=(), hole=0.15, spread_deg=70.0):
    """A synthetic frame: depth 1.5-4 m with random zero holes and whole zero rows, a current pose, n_kf
    keyframe poses spread about the y axis (every fourth one turned by 180 degrees: faces away), words."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = 2.5 + np.sin(xx / 17.0 + seed) + 0.5 * np.cos(yy / 11.0) + 0.05 * rng.rand(H, W)
    depth[rng.rand(H, W) < hole] = 0.0
    for r in zero_rows:
        depth[r % H] = 0.0
    w2c = _pose(_rot_y(np.deg2rad(3.0)) @ _rot_x(np.deg2rad(-2.0)), [0.05, -0.02, 0.1])
    kf = np.zeros((max(n_kf, 1), 16), np.float32)
    for i in range(n_kf):
        a = np.deg2rad(rng.uniform(-spread_deg, spread_deg) + (180.0 if i % 4 == 3 else 0.0))
        kf[i] = _pose(_rot_y(a) @ _rot_x(np.deg2rad(rng.uniform(-5, 5))), rng.uniform(-0.3, 0.3, 3)).reshape(16)
    return {"W": W, "H": H, "depth": depth.astype(np.float32), "intr": (0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5),
            "w2c": w2c, "kf_w2c": kf[:n_kf], "n_kf": n_kf, "k_select": k_select, "u_pix": words(rng, S),
            "perm_key": words(rng, max(n_kf - 1, 0)), "u_draw": words(rng, n_draws),
            "kf_time": (np.arange(n_kf, dtype=np.int64) * 5), "time_idx": 5 * n_kf + 2, "cur_row": n_kf + 3}


def restate(c):
    """Steps 1-6 in float64 on the case's float32 values.  Returns the exact outputs (pixels, n_points,
    window, n_window, draw_rows, draw_times) and, per candidate keyframe, `sure` and `borderline` counts.
    Raises when an exact output would rest on a borderline comparison (such a case is not a valid input)."""
    W, H = c["W"], c["H"]
    fx, fy, cx, cy = (float(np.float32(v)) for v in c["intr"])
    d = c["depth"].astype(np.float64).reshape(-1)
    S, n_kf = len(c["u_pix"]), c["n_kf"]
    n_cand = max(n_kf - 1, 0)
    valid = np.flatnonzero(d > 0)
    n_valid = len(valid)
    sure, border = np.zeros(n_cand, np.int64), np.zeros(n_cand, np.int64)
    if n_valid == 0 or S == 0:
        pix = np.full(S, -1, np.int64)
        keep = np.zeros(S, bool)
    else:
        r = ((c["u_pix"].astype(np.uint64) * np.uint64(n_valid)) >> np.uint64(32)).astype(np.int64)
        pix = valid[r]
        row, col = pix // W, pix % W
        z = d[pix]
        p = np.stack(((col - cx) / fx * z, (row - cy) / fy * z, z))          # [3, S]
        m = c["w2c"].astype(np.float64).reshape(4, 4)
        R, t = m[:3, :3], m[:3, 3]
        w = R.T @ p + (-(R.T @ t))[:, None]
        C = float(np.abs(p).sum(0).max() + np.abs(t).sum())
        _, inv, counts = np.unique(r, return_inverse=True, return_counts=True)
        twice = counts[inv] > 1
        q = np.abs(w * 1e4)
        d_o = 2 * 1e4 * 8 * EPS * C
        origin = (q < 0.5 - d_o).all(0)
        if ((q < 0.5 + d_o).all(0) != origin).any():
            raise ValueError("a sample's origin test is borderline")
        keep = ~twice & ~origin
        if n_cand:
            k = c["kf_w2c"][:n_cand].astype(np.float64).reshape(n_cand, 4, 4)
            C = max(C, float(np.abs(w).sum(0).max() + np.abs(k[:, :3, 3]).sum(1).max()))
            pc = k[:, :3, :3] @ w[None] + k[:, :3, 3:4]                        # [n_cand, 3, S]
            zz = pc[:, 2] + float(np.float32(1e-5))
            with np.errstate(divide="ignore", invalid="ignore"):
                u, v = (fx * pc[:, 0] + cx * pc[:, 2]) / zz, (fy * pc[:, 1] + cy * pc[:, 2]) / zz
                az = np.abs(zz)
                du = 2 * ((31 * (fx + cx) + 29 * np.abs(u)) * EPS * C / az + EPS * np.abs(u))
                dv = 2 * ((31 * (fy + cy) + 29 * np.abs(v)) * EPS * C / az + EPS * np.abs(v))
            dz = 2 * 29 * EPS * C
            du, dv = np.nan_to_num(du, nan=np.inf), np.nan_to_num(dv, nan=np.inf)
            u, v = np.nan_to_num(u, nan=0.0), np.nan_to_num(v, nan=0.0)
            yes = (u > EDGE + du) & (u < W - EDGE - du) & (v > EDGE + dv) & (v < H - EDGE - dv) & (zz > dz)
            no = (u < EDGE - du) | (u > W - EDGE + du) | (v < EDGE - dv) | (v > H - EDGE + dv) | (zz < -dz)
            sure = (yes & keep[None]).sum(1)
            border = (~yes & ~no & keep[None]).sum(1)
    if ((sure == 0) & (border > 0)).any():
        raise ValueError("a keyframe's eligibility rests on a borderline sample")
    keys = c["perm_key"].astype(np.uint64)
    elig = sorted((int(keys[i]), i) for i in range(n_cand) if sure[i] > 0)
    win = [i for _, i in elig[:c["k_select"]]]
    if n_kf > 0:
        win.append(n_kf - 1)
    win.append(c["cur_row"])
    n_window = len(win)
    window = np.array(win + [-1] * (c["k_select"] + 2 - n_window), np.int64)
    idx = ((c["u_draw"].astype(np.uint64) * np.uint64(n_window)) >> np.uint64(32)).astype(np.int64)
    rows = window[idx]
    kt = np.append(c["kf_time"][:n_kf], c["time_idx"])
    times = np.where(rows == c["cur_row"], c["time_idx"], kt[np.minimum(rows, n_kf)])
    return {"pixels": pix, "n_points": int(keep.sum()), "n_eligible": len(elig), "window": window,
            "n_window": n_window, "draw_rows": rows, "draw_times": times, "sure": sure, "borderline": border,
            "S": S}


def make_valid_case(W, H, S, n_kf, seed, **kw):
    """make_case at the first seed >= `seed` whose restatement -- alone, before any code under test runs --
    shows a valid input: no exact output rests on a borderline comparison and at most 1 % of the samples are
    borderline for any keyframe.  Returns (case, restatement)."""
    for s in range(seed, seed + 50):
        c = make_case(W, H, S, n_kf, s, **kw)
        try:
            ref = restate(c)
        except ValueError:
            continue
        if ref["borderline"].max(initial=0) <= 0.01 * S:
            return c, ref
    raise RuntimeError("no valid case in 50 seeds")


def check(out, ref, pixels=True):
    """`out`: a selection's outputs as numpy arrays / ints (the keys of select_device's dict)."""
    g = {k: (np.asarray(v.cpu()) if hasattr(v, "cpu") else v) for k, v in out.items() if v is not None}
    if pixels:
        assert np.array_equal(g["pixels"], ref["pixels"])
    assert int(g["n_points"][0]) == ref["n_points"]
    ov = g["overlap"].astype(np.int64)
    assert ov.shape == ref["sure"].shape
    assert ((ov >= ref["sure"]) & (ov <= ref["sure"] + ref["borderline"])).all(), (ov, ref["sure"], ref["borderline"])
    assert int(g["n_window"][0]) == ref["n_window"]
    assert np.array_equal(g["window"], ref["window"])
    assert np.array_equal(g["draw_rows"], ref["draw_rows"])
    assert np.array_equal(g["draw_times"], ref["draw_times"])


def to_torch(c, device):
    """The case as select_literal / select_device arguments (a tuple, in their order)."""
    import torch

    from splatam_amd.keyframes import words_tensor
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return (t(c["depth"]), c["intr"], t(c["w2c"]), t(c["kf_w2c"]).reshape(-1, 16), c["n_kf"], c["k_select"],
            words_tensor(c["u_pix"], device), words_tensor(c["perm_key"], device), words_tensor(c["u_draw"], device),
            t(c["kf_time"]), c["time_idx"], c["cur_row"])
