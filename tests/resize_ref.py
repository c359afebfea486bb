"""numpy restatements of gsr_resize_frame's contract (include/gsr_glue.h) for tests/test_resize_cpu.py and
tests/test_gpu_resize.py: the formula in float64 (restate64), the same with the header's float32 operation
order (restate32) and the integer nearest-neighbour rule (nearest_index)."""
import numpy as np

# (H, W) -> (h, w): an integer ratio; a non-integer one; x and y ratios that differ, odd sizes; a 12-pixel
# output; the identity; an odd output at factor 2
# (as (rows, columns): 64x48 -> 32x24 is ((48, 64), (24, 32)))
SIZE_PAIRS = (((48, 64), (24, 32)), ((48, 64), (30, 40)), ((37, 61), (13, 29)), ((5, 7), (3, 4)),
              ((48, 64), (48, 64)), ((34, 60), (17, 30)))


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """floor(i * n_in / n_out) in integers."""
    return (np.arange(n_out, dtype=np.int64) * n_in) // n_out


def taps(n_out: int, n_in: int):
    """(i0, i1, remainder, denominator): s = max(0, (i + 0.5) n_in / n_out - 0.5) as i0 + remainder / den."""
    i = np.arange(n_out, dtype=np.int64)
    num = (2 * i + 1) * n_in - n_out
    den = 2 * n_out
    pos = num > 0
    i0 = np.where(pos, num // den, 0)
    rem = np.where(pos, num - i0 * den, 0)
    return i0, np.minimum(i0 + 1, n_in - 1), rem, den


def _lerp(a, b, t):
    with np.errstate(invalid="ignore"):
        return np.where(t == 0, a, a + t * (b - a))  # (each numpy op rounds once in the arrays' dtype)


def _bilinear32(im, h, w):
    """The header's float32 operation order: exact taps, the weight one division, lerps rows first."""
    H, W = im.shape[-2:]
    im = im.astype(np.float32)
    x0, x1, rx, dx = taps(w, W)
    y0, y1, ry, dy = taps(h, H)
    tx = (rx.astype(np.float32) / np.float32(dx))[None, None, :]
    ty = (ry.astype(np.float32) / np.float32(dy))[None, :, None]
    top = _lerp(im[:, y0][:, :, x0], im[:, y0][:, :, x1], tx)
    bot = _lerp(im[:, y1][:, :, x0], im[:, y1][:, :, x1], tx)
    out = _lerp(top, bot, ty)
    assert out.dtype == np.float32
    return out


def _coords64(n_out, n_in):
    """s = max(0, (i + 0.5) n_in / n_out - 0.5) in float64 arithmetic: (i0, i1, the weight of i1)."""
    s = np.maximum(0.0, (np.arange(n_out, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def restate64(im, depth, size):
    """(im, depth) at size (h, w): the formula in float64 arithmetic throughout (the coordinate included, as
    torch's float64 path forms it: a weighted sum of the four taps); the depth the copied source pixels."""
    h, w = size
    H, W = depth.shape[-2:]
    d = depth.reshape(H, W)[nearest_index(h, H)[:, None], nearest_index(w, W)[None, :]].reshape(1, h, w)
    im = im.astype(np.float64)
    x0, x1, tx = _coords64(w, W)
    y0, y1, ty = _coords64(h, H)
    assert np.array_equal(x0, taps(w, W)[0]) and np.array_equal(y0, taps(h, H)[0])  # (the integer taps agree)
    tx, ty = tx[None, None, :], ty[None, :, None]
    top = (1.0 - tx) * im[:, y0][:, :, x0] + tx * im[:, y0][:, :, x1]
    bot = (1.0 - tx) * im[:, y1][:, :, x0] + tx * im[:, y1][:, :, x1]
    return (1.0 - ty) * top + ty * bot, d


def restate32(im, depth, size):
    """The contract in float32 with the header's operation order: the taps and the weight from integers (one
    division of two exactly converted integers), lerp(a, b, t) = a + t * (b - a) with each operation rounded,
    rows first."""
    h, w = size
    _, d = restate64(im, depth, size)
    return _bilinear32(im, h, w), d


def make_frame(H: int, W: int, seed: int = 0):
    """A seeded frame: colour in [0, 1), depth in [0.5, 5) with a tenth of the pixels unmeasured (0)."""
    rng = np.random.RandomState(seed)
    im = rng.uniform(size=(3, H, W)).astype(np.float32)
    depth = rng.uniform(0.5, 5.0, size=(1, H, W)).astype(np.float32)
    depth[rng.uniform(size=(1, H, W)) < 0.1] = 0.0
    return im, depth


def max_distance(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))
