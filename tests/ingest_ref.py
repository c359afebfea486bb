"""numpy restatements of gsr_ingest_frame's contract (include/gsr_glue.h) for tests/test_ingest_cpu.py and
tests/test_gpu_ingest.py, written from the header and independent of splatam_amd.ingest: the colour through a
256-entry table of correctly rounded float32 quotients, the depth as numpy's float64 quotient rounded to float32
once, the far readings' -1, and the small frames as tests/resize_ref.py's float32 restatement of the float frame."""
import numpy as np

import resize_ref as rr

SCALES = (1000.0, 6553.5, 5000.0)  # the reference's Replica / ScanNet / TUM png_depth_scale
MAX_DEPTH = 9.5                    # the reference's depth[depth >= 9.5] = -1

# byte -> colour: one float32 division per entry (numpy's float32 `/` is IEEE division)
TABLE = np.array([np.float32(i) / np.float32(255) for i in range(256)], dtype=np.float32)

bits = rr.bits


def colour(rgb_u8: np.ndarray) -> np.ndarray:
    """[H,W,3] uint8 -> [3,H,W] float32."""
    assert rgb_u8.dtype == np.uint8 and rgb_u8.ndim == 3 and rgb_u8.shape[2] == 3
    return np.ascontiguousarray(TABLE[rgb_u8].transpose(2, 0, 1))


def depth(depth_u16: np.ndarray, scale: float, max_depth=None) -> np.ndarray:
    """[H,W] uint16 -> [1,H,W] float32: (float)((double)u / scale); d >= max_depth (float32 compare) -> -1."""
    assert depth_u16.dtype == np.uint16 and depth_u16.ndim == 2
    q = depth_u16.astype(np.float64) / np.float64(scale)
    d = q.astype(np.float32)
    if max_depth is not None:
        d = np.where(d >= np.float32(max_depth), np.float32(-1.0), d)
    return np.ascontiguousarray(d[None])


def depth_f32_division(depth_u16: np.ndarray, scale: float) -> np.ndarray:
    """The correctly rounded float32 division by the scale rounded to float32 first.  For a scale that IS a
    float32 value this is the contract's bits: rounding the float64 quotient again is innocuous for a division
    when the wider format has at least 2 * 24 + 2 bits."""
    return (depth_u16.astype(np.float32) / np.float32(scale))[None]


def depth_f32_reciprocal(depth_u16: np.ndarray, scale: float) -> np.ndarray:
    """What the contract is NOT: a float32 multiply by the rounded reciprocal of the scale (how torch divides by
    a scalar on the device)."""
    return (depth_u16.astype(np.float32) * (np.float32(1) / np.float32(scale)))[None]


def frame(rgb_u8, depth_u16, scale, max_depth=None):
    return colour(rgb_u8), depth(depth_u16, scale, max_depth)


def small(rgb_u8, depth_u16, scale, max_depth, size):
    """The small frame: gsr_resize_frame's restatement (resize_ref.restate32) of the float frame."""
    im, d = frame(rgb_u8, depth_u16, scale, max_depth)
    return rr.restate32(im, d, size)


def all_bytes_image() -> np.ndarray:
    """16x16x3: every byte 0..255 in every channel, each channel in an order of its own."""
    b = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack([b, b[::-1], np.roll(b, 97)], axis=-1).reshape(16, 16, 3))


def all_u16_image() -> np.ndarray:
    """256x256: every uint16 value once."""
    return np.arange(65536, dtype=np.uint16).reshape(256, 256)


def raw_frame(H: int, W: int, seed: int = 0):
    """A seeded raw frame of any size whose bytes and readings run through the all-values images above (every
    byte value appears as soon as H W >= 256), with a tenth of the readings 0 and some beyond 9.5 m at any scale."""
    rng = np.random.RandomState(seed)
    n = H * W
    rgb = all_bytes_image().reshape(-1, 3)[(np.arange(n) * 7 + seed) % 256].reshape(H, W, 3)
    d = all_u16_image().reshape(-1)[rng.randint(0, 65536, size=n)].reshape(H, W).copy()
    d[rng.uniform(size=(H, W)) < 0.1] = 0
    return np.ascontiguousarray(rgb), np.ascontiguousarray(d)


def pose_matrix(pose) -> np.ndarray:
    """(x, y, z, qx, qy, qz, qw) -> [4,4] float64, the quaternion normalised: R = I + 2 w [v]x + 2 [v]x^2."""
    p = np.asarray(pose, dtype=np.float64)
    q = p[3:] / np.linalg.norm(p[3:])
    v, w = q[:3], q[3]
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + 2 * w * K + 2 * K @ K
    m[:3, 3] = p[:3]
    return m
