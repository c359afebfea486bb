"""A numpy restatement of gsr_densify_frame's contract (include/gsr_glue.h), written from the contract: float32
elementwise operations (each rounded on its own), np.partition for the lower median, np.cumsum for the ranks;
log_scales' logarithm in float64 (of the float32 sqrt(q * q) the contract states).  Shared by tests/test_densify_cpu.py and tests/test_gpu_densify.py, with the seeded
synthetic cases both use (a depth / silhouette image, a frame and a pose; no render)."""
import numpy as np

F32 = np.float32
ROW_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
COLS = {"means3D": 3, "rgb_colors": 3, "unnorm_rotations": 4, "logit_opacities": 1, "log_scales": 1}
SHAPES = ((1, 1), (5, 7), (61, 67), (96, 130), (97, 131))
CONTENTS = ("random", "quantised", "zeros90", "denormal", "gt_zero", "all_selected", "nan_depth", "nan_sil")
NAN_PIXEL = 11  # the flat pixel index the two NaN cases poison


def _pose(rng) -> np.ndarray:
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, rng.uniform(-1.0, 1.0, 3)
    return m.astype(F32).reshape(16)


def make_case(H: int, W: int, content: str = "random", seed: int = 0) -> dict:
    """depth_sil [3,H,W], im [3,H,W], gt [1,H,W], w2c [16], intrinsics, sil_thres (numpy, float32)."""
    rng = np.random.RandomState(1000 * seed + 17 * H + W)
    N = H * W
    gt = rng.uniform(0.5, 6.0, N).astype(F32)
    gt[rng.uniform(size=N) < 0.05] = 0.0  # no measurement
    rd = (gt + rng.standard_normal(N).astype(F32) * F32(0.05)).astype(F32)
    rd[rng.uniform(size=N) < 0.02] += F32(3.0)  # far behind the surface: the depth term
    u = rng.uniform(size=N)
    sil = np.where(u < 0.1, rng.uniform(0.0, 0.5, N), rng.uniform(0.6, 1.0, N)).astype(F32)
    if content == "quantised":  # err takes four values exactly: whole radix bins tie
        gt = (rng.randint(32, 384, N) / 64.0).astype(F32)
        step = np.array([0.0, 0.125, 0.25, 0.5], dtype=F32)[rng.randint(0, 4, N)]
        rd = (gt + step * np.where(rng.uniform(size=N) < 0.5, F32(-1), F32(1)).astype(F32)).astype(F32)
        rd[rng.uniform(size=N) < 0.01] += F32(40.0)
    elif content == "zeros90":  # med = 0 and thr = 0
        same = rng.uniform(size=N) < 0.9
        rd = np.where(same, gt, rd).astype(F32)
    elif content == "denormal":  # every err a denormal (or 0): depths of a few 2^-126
        tiny = np.ldexp(1.0, -149)
        gt = ((1 << 23) * tiny + rng.randint(0, 1 << 20, N) * tiny).astype(F32)
        rd = (gt.astype(np.float64) + rng.randint(-(1 << 12), 1 << 12, N) * tiny).astype(F32)
    elif content == "gt_zero":
        gt[:] = 0.0
    elif content == "all_selected":
        gt = rng.uniform(0.5, 6.0, N).astype(F32)
        sil[:] = 0.0
    elif content in ("nan_depth", "nan_sil") and N > NAN_PIXEL:
        gt[NAN_PIXEL] = F32(2.0)
        if content == "nan_depth":
            rd[NAN_PIXEL] = np.nan
        else:  # the depth term is false there (rd == gt): a NaN silhouette selects nothing
            rd[NAN_PIXEL], sil[NAN_PIXEL] = gt[NAN_PIXEL], np.nan
    depth_sil = np.stack((rd, sil, (rd * rd).astype(F32))).reshape(3, H, W).astype(F32)
    fx, fy = float(F32(0.9 * W + 100.0)), float(F32(0.95 * W + 100.0))
    return {"H": H, "W": W, "depth_sil": depth_sil, "im": rng.uniform(size=(3, H, W)).astype(F32),
            "gt": gt.reshape(1, H, W), "w2c": _pose(rng), "intrinsics": (fx, fy, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5),
            "sil_thres": 0.5}


def lower_median(v: np.ndarray):
    """torch.median's value: element (n - 1) // 2 of the ascending order; NaN if any element is NaN."""
    v = np.asarray(v).reshape(-1)
    if np.isnan(v).any():
        return v.dtype.type(np.nan)
    k = (v.size - 1) // 2
    return np.partition(v, k)[k]


def restate(case: dict) -> dict:
    """The selection and the appended rows, in row-major pixel order: mask [N] bool, rank [N] int64 (-1: not
    selected), count, rows {key: [count, cols]} (float32 bits to compare; log_scales float64), med."""
    H, W = case["H"], case["W"]
    rd, sil = case["depth_sil"][0].reshape(-1), case["depth_sil"][1].reshape(-1)
    gt = case["gt"].reshape(-1)
    fx, fy, cx, cy = (F32(v) for v in case["intrinsics"])
    f = F32((float(fx) + float(fy)) / 2.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        valid = gt > 0
        err = (np.abs(gt - rd) * valid.astype(F32)).astype(F32)
        med = lower_median(err)
        thr = F32(50.0) * med
        mask = ((sil < F32(case["sil_thres"])) | ((rd > gt) & (err > thr))) & valid
        rank = np.where(mask, np.cumsum(mask.astype(np.int64)) - 1, -1)
        pix = np.nonzero(mask)[0]
        row, col = (pix // W).astype(F32), (pix % W).astype(F32)
        z = gt[pix]
        x = (col - cx) / fx * z
        y = (row - cy) / fy * z
        m = case["w2c"].astype(F32)
        means = np.zeros((pix.size, 3), dtype=F32)
        for a in range(3):
            ra, rb, rc = m[a], m[4 + a], m[8 + a]
            ta = -(ra * m[3] + rb * m[7] + rc * m[11])
            means[:, a] = ra * x + rb * y + rc * z + ta
        # q, q * q and the square root are float32 steps of the contract (correctly rounded, so reproducible:
        # a tiny depth's q * q underflows to 0 here as it does there); the logarithm alone is taken in float64
        q = z / f
        s = np.sqrt(q * q)
        assert s.dtype == F32
        rot = np.zeros((pix.size, 4), dtype=F32)
        rot[:, 0] = 1.0
        rows = {"means3D": means, "rgb_colors": case["im"].reshape(3, -1)[:, pix].T.copy(),
                "unnorm_rotations": rot, "logit_opacities": np.zeros((pix.size, 1), dtype=F32),
                "log_scales": np.log(s.astype(np.float64)).reshape(-1, 1)}
    assert means.dtype == F32 and x.dtype == F32 and err.dtype == F32
    return {"mask": mask, "rank": rank, "count": int(pix.size), "rows": rows, "med": med}


def expected_call(ref: dict, n_live: int, capacity: int, overflow: int) -> dict:
    """What one call leaves: dest [N] int32, n_added, n_live, overflow, written (the rows [n_live, n_live +
    written) hold ref["rows"][:written])."""
    total = n_live + ref["count"]
    dest = np.where(ref["mask"], n_live + ref["rank"], -1)
    dest = np.where(dest < capacity, dest, -1).astype(np.int32)
    return {"dest": dest, "n_added": ref["count"], "n_live": min(total, capacity),
            "overflow": int(bool(overflow) or total > capacity), "written": max(0, min(total, capacity) - n_live)}


def rel_distance(got: np.ndarray, ref64: np.ndarray) -> float:
    """The largest |got - ref| / |ref| over the finite, non-zero reference values; the others (log 0 = -inf)
    must be equal."""
    got, ref64 = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref64, dtype=np.float64).reshape(-1)
    ok = np.isfinite(ref64) & (ref64 != 0)
    assert np.array_equal(got[~ok], ref64[~ok])
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref64[ok]) / np.abs(ref64[ok])))


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)
