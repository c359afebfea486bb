"""A float64 numpy restatement of the evaluation metrics (include/gsr_glue.h: gsr_eval_frame; SplaTAM's
utils/eval_helpers.py:23-77,466-512), written from the header's statement alone and independently of
splatam_amd/evaluate.py: masks and sums by numpy, the MS-SSIM window by np.convolve row by row, the pooling by an
explicit zero-padded array, the trajectory alignment by an explicit loop of outer products.  Shared by
tests/test_eval_cpu.py and tests/test_gpu_eval.py (cases are cached: computed once, never modified)."""
import numpy as np

COLS = ("psnr", "ms_ssim", "depth_rmse", "depth_l1", "n_valid", "mse_r", "mse_g", "mse_b")
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window():
    g = np.array([np.exp(-((k - 5) ** 2) / (2.0 * 1.5 ** 2)) for k in range(11)], dtype=np.float64)
    return g / g.sum()


def filt(a, g):
    """Valid correlation of a 2-D array with g along axis 0 (H), then along axis 1 (W)."""
    h, w = a.shape
    v = np.empty((h - 10, w), dtype=np.float64)
    for c in range(w):
        v[:, c] = np.convolve(a[:, c], g[::-1], mode="valid")
    out = np.empty((h - 10, w - 10), dtype=np.float64)
    for r in range(h - 10):
        out[r] = np.convolve(v[r], g[::-1], mode="valid")
    return out


def pool(a):
    """avg_pool2d(2, 2, padding = extent % 2, the zero pad counted): windows [-1,0], [1,2], ... on an odd axis."""
    h, w = a.shape
    ph, pw = h % 2, w % 2
    z = np.zeros((h + 2 * ph, w + 2 * pw), dtype=np.float64)
    z[ph:ph + h, pw:pw + w] = a
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = np.empty((oh, ow), dtype=np.float64)
    for i in range(oh):
        for j in range(ow):
            out[i, j] = (z[2 * i, 2 * j] + z[2 * i, 2 * j + 1] + z[2 * i + 1, 2 * j] + z[2 * i + 1, 2 * j + 1]) / 4.0
    return out


def ms_ssim(X, Y):
    """X, Y [C, H, W] float64 -> the scalar; ValueError for min(H, W) <= 160."""
    if min(X.shape[1:]) <= 160:
        raise ValueError("smaller side must exceed 160")
    g = window()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    per_channel = []
    for c in range(X.shape[0]):
        x, y = X[c].astype(np.float64), Y[c].astype(np.float64)
        prod = 1.0
        for level in range(5):
            mu1, mu2 = filt(x, g), filt(y, g)
            s1 = filt(x * x, g) - mu1 * mu1
            s2 = filt(y * y, g) - mu2 * mu2
            s12 = filt(x * y, g) - mu1 * mu2
            cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
            ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
            v = cs_map.mean() if level < 4 else ssim_map.mean()
            prod *= max(v, 0.0) ** WEIGHTS[level]
            if level < 4:
                x, y = pool(x), pool(y)
        per_channel.append(prod)
    return float(np.mean(per_channel))


def frame_metrics(im, depth_sil, gt_im, gt_depth, sil_thres, use_sil_mask, with_ms_ssim=True):
    """The row of COLS in float64 (inputs: float32 arrays, [3,H,W], [3,H,W], [3,H,W], [1,H,W]; sil_thres is
    compared as the float32 value the kernel receives)."""
    im, gt_im = im.astype(np.float64), gt_im.astype(np.float64)
    gd = gt_depth.reshape(gt_depth.shape[-2:]).astype(np.float64)
    valid = (gd > 0).astype(np.float64)
    presence = (depth_sil[1] > np.float32(sil_thres)).astype(np.float64)
    m = valid * presence if use_sil_mask else valid
    with np.errstate(all="ignore"):
        wi, wg = im * m, gt_im * m
        mse = ((wi - wg) ** 2).reshape(3, -1).sum(1) / float(gd.size)
        psnr = float(np.mean(20.0 * np.log10(1.0 / np.sqrt(mse))))
        e = depth_sil[0].astype(np.float64) * valid - gd
        if use_sil_mask:
            e = e * presence
        n_valid = valid.sum()
        l1 = (np.abs(e) * valid).sum() / n_valid
        rmse = (np.sqrt(e * e) * valid).sum() / n_valid
    ms = ms_ssim(wi, wg) if with_ms_ssim else float("nan")
    return np.array([psnr, ms, rmse, l1, n_valid, mse[0], mse[1], mse[2]], dtype=np.float64)


def ate(gt_w2c, est_w2c):
    """Mean translational error after Horn's alignment of the gt translations onto the estimated ones; gt poses
    holding a NaN are skipped (never the first)."""
    gt = [np.asarray(m, dtype=np.float64) for m in gt_w2c]
    est = [np.asarray(m, dtype=np.float64) for m in est_w2c]
    idx = [i for i in range(len(gt)) if i == 0 or not np.isnan(gt[i]).any()]
    model = np.array([gt[i][:3, 3] for i in idx]).T
    data = np.array([est[i][:3, 3] for i in idx]).T
    mc, dc = model.mean(axis=1).reshape(3, 1), data.mean(axis=1).reshape(3, 1)
    Wm = np.zeros((3, 3))
    for k in range(model.shape[1]):
        Wm += np.outer(model[:, k] - mc[:, 0], data[:, k] - dc[:, 0])
    U, _, Vh = np.linalg.svd(Wm.transpose())
    S = np.identity(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    R = U.dot(S).dot(Vh)
    t = dc - R.dot(mc)
    err = R.dot(model) + t - data
    return float(np.sqrt((err * err).sum(axis=0)).mean())


# ------------------------------------------------------------------ seeded cases

_CASES = {}


def make_case(H, W, seed=None, depth="mixed"):
    """Seeded float32 images: gt_im uniform, im = gt_im + noise (clipped to [0, 1]); depth_sil channel 0 a depth
    around 2 m, channel 1 a silhouette in [0.6, 1] with a low (0.1 .. 0.4) block and a few pixels EXACTLY at
    0.5; gt_depth = depth with 1 % noise and a zeroed block (depth="mixed"), all zero ("invalid") or all
    positive ("valid")."""
    key = (H, W, seed, depth)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.RandomState(1000 * H + W if seed is None else seed)
    f32 = np.float32
    gt_im = rng.rand(3, H, W).astype(f32)
    im = np.clip(gt_im + 0.1 * rng.randn(3, H, W), 0.0, 1.0).astype(f32)
    d = (2.0 + rng.rand(H, W)).astype(f32)
    sil = (0.6 + 0.4 * rng.rand(H, W)).astype(f32)
    h0, h1, w0, w1 = H // 5, max(H // 5 + 1, H // 2), W // 2, max(W // 2 + 1, (4 * W) // 5)
    sil[h0:h1, w0:w1] = (0.1 + 0.3 * rng.rand(h1 - h0, w1 - w0)).astype(f32)
    sil[::7, ::5] = f32(0.5)
    gt_depth = (d * (1.0 + 0.01 * rng.randn(H, W))).astype(f32)
    if depth == "mixed":
        gt_depth[(2 * H) // 5:max((2 * H) // 5 + 1, (7 * H) // 10), W // 8:max(W // 8 + 1, (5 * W) // 8)] = 0
        gt_depth[-1, :] = 0
    elif depth == "invalid":
        gt_depth[:] = 0
    depth_sil = np.stack([d, sil, d * d]).astype(f32)
    case = {"im": im, "depth_sil": depth_sil, "gt_im": gt_im, "gt_depth": gt_depth[None], "sil_thres": 0.5}
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = case
    return case


_REFS = {}


def reference(H, W, use_sil_mask, with_ms_ssim=True, seed=None, depth="mixed"):
    key = (H, W, bool(use_sil_mask), bool(with_ms_ssim), seed, depth)
    if key not in _REFS:
        c = make_case(H, W, seed, depth)
        _REFS[key] = frame_metrics(c["im"], c["depth_sil"], c["gt_im"], c["gt_depth"], c["sil_thres"], use_sil_mask,
                                   with_ms_ssim)
        _REFS[key].setflags(write=False)
    return _REFS[key]
