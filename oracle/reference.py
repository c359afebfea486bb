"""ctypes front-end of ``oracle/_ref/libref_raster.so``: the reference's own kernels
(``cuda_rasterizer/forward.cu``, ``backward.cu``, ``rasterizer_impl.cu``) compiled unmodified by
hipcc for gfx950 behind ``oracle/ref_driver.cpp`` (``make -C oracle ref``).

TEST INFRASTRUCTURE ONLY, like ``oracle.py``: imported by ``tests/`` and ``tools/``, never by the
product package ``splatam_amd``.  ``forward`` / ``backward`` / ``mark_visible`` take the arguments of
their namesakes in ``oracle.py`` and return the same frame fields and the same gradient dictionary
(``harness.GRAD_KEYS``, same shapes), in float32: what the reference computes on the GPU.

The library exists only where ``build()`` found a reference checkout (or where a tree built there was
copied to); ``available()`` says whether it does and ``why_unavailable()`` why not.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from .oracle import ForwardResult, _arr, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_ref", "libref_raster.so")
_lib = None
_why = None

_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_B = ctypes.POINTER(ctypes.c_ubyte)


class _In(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int), ("D", ctypes.c_int), ("M", ctypes.c_int), ("W", ctypes.c_int),
                ("H", ctypes.c_int), ("bg", _F), ("means3D", _F), ("shs", _F), ("colors", _F), ("opacities", _F),
                ("scales", _F), ("rotations", _F), ("cov3D_precomp", _F), ("scale_modifier", ctypes.c_float),
                ("view", _F), ("proj", _F), ("campos", _F), ("tan_fovx", ctypes.c_float),
                ("tan_fovy", ctypes.c_float)]


class _FwdOut(ctypes.Structure):
    _fields_ = [("out_color", _F), ("out_depth", _F), ("radii", _I), ("means2D", _F), ("depths", _F),
                ("conic_opacity", _F), ("rgb", _F), ("clamped", _B), ("tiles_touched", _I), ("final_T", _F),
                ("n_contrib", _I), ("ranges", _I), ("num_rendered", ctypes.c_int)]


class _Grads(ctypes.Structure):
    _fields_ = [(k, _F) for k in ("dmeans2D", "dcolors", "dopacity", "dmeans3D", "dcov3D", "dsh", "dscales", "drot")]


def _load():
    global _lib, _why
    if _lib is not None or _why is not None:
        return _lib
    if not os.path.exists(LIB):
        _why = f"{os.path.relpath(LIB, os.path.dirname(_HERE))} is not built (make -C oracle ref needs a reference checkout)"
        return None
    try:
        lib = ctypes.CDLL(LIB)
    except OSError as e:
        _why = f"libref_raster.so does not load: {e}"
        return None
    lib.ref_forward.argtypes = [ctypes.POINTER(_In), ctypes.POINTER(_FwdOut), ctypes.POINTER(ctypes.c_void_p)]
    lib.ref_forward.restype = ctypes.c_int
    lib.ref_point_list.argtypes = [ctypes.c_void_p, _I, ctypes.c_int]
    lib.ref_point_list.restype = ctypes.c_int
    lib.ref_backward.argtypes = [ctypes.c_void_p, _F, ctypes.c_int, ctypes.POINTER(_Grads)]
    lib.ref_backward.restype = ctypes.c_int
    lib.ref_mark_visible.argtypes = [ctypes.c_int, _F, _F, _F, _B]
    lib.ref_mark_visible.restype = ctypes.c_int
    lib.ref_free.argtypes = [ctypes.c_void_p]
    lib.ref_free.restype = None
    lib.ref_strerror.argtypes = [ctypes.c_int]
    lib.ref_strerror.restype = ctypes.c_char_p
    _lib = lib
    return _lib


def available() -> bool:
    """True where the reference library is built and loads."""
    return _load() is not None


def why_unavailable() -> str:
    _load()
    return _why or ""


class ReferenceError_(RuntimeError):
    """A refusal of the driver or a HIP error it returned (``code``: < 0 the driver's, > 0 a hipError_t)."""

    def __init__(self, where, code, text):
        super().__init__(f"{where}: {text} ({code})")
        self.code = code


def _check(where, rc):
    if rc != 0:
        raise ReferenceError_(where, rc, _lib.ref_strerror(rc).decode())


class _Context:
    """Owns the driver's device state of one forward (inputs and the three chunk buffers)."""

    def __init__(self, handle):
        self.handle = handle

    def close(self):
        if self.handle and _lib is not None:
            _lib.ref_free(self.handle)
        self.handle = None

    __del__ = close


def forward(means3D, opacities, *, view, proj, campos, tanfovx, tanfovy, H, W, bg=(0.0, 0.0, 0.0),
            shs=None, colors=None, scales=None, rotations=None, cov3D=None, scale_modifier=1.0,
            sh_degree=0, dtype=np.float32) -> ForwardResult:
    """Rasterizer::forward of the reference on the GPU (prefiltered=False).  The result's
    ``unstable*`` masks are all False and ``pair_evals`` is 0: the reference reports neither."""
    lib = _load()
    if lib is None:
        raise RuntimeError(why_unavailable())
    if np.dtype(dtype) != np.float32:
        raise ValueError("the reference computes in float32")
    f4 = np.float32
    keep = dict(
        means3D=_arr(means3D, f4).reshape(-1, 3), opac=_arr(opacities, f4).reshape(-1),
        shs=_arr(shs, f4), colors=_arr(colors, f4), scales=_arr(scales, f4), rot=_arr(rotations, f4),
        cov3D=_arr(cov3D, f4), view=_arr(view, f4).reshape(-1), proj=_arr(proj, f4).reshape(-1),
        campos=_arr(campos, f4).reshape(-1), bg=_arr(bg, f4).reshape(-1))
    P = keep["means3D"].shape[0]
    M = 0 if keep["shs"] is None or keep["shs"].size == 0 else keep["shs"].shape[1]
    H, W = int(H), int(W)
    for name, n in (("opac", P), ("view", 16), ("proj", 16), ("campos", 3), ("bg", 3), ("colors", P * 3),
                    ("shs", P * M * 3), ("scales", P * 3), ("rot", P * 4), ("cov3D", P * 6)):
        a = keep[name]
        if a is not None and (name != "shs" or M) and a.size != n:
            raise ValueError(f"{name}: {a.size} values, {n} expected")
    inp = _In(P=P, D=int(sh_degree), M=M, W=W, H=H, bg=_ptr(keep["bg"], ctypes.c_float),
              means3D=_ptr(keep["means3D"], ctypes.c_float), shs=_ptr(keep["shs"] if M else None, ctypes.c_float),
              colors=_ptr(keep["colors"], ctypes.c_float), opacities=_ptr(keep["opac"], ctypes.c_float),
              scales=_ptr(keep["scales"], ctypes.c_float), rotations=_ptr(keep["rot"], ctypes.c_float),
              cov3D_precomp=_ptr(keep["cov3D"], ctypes.c_float), scale_modifier=float(scale_modifier),
              view=_ptr(keep["view"], ctypes.c_float), proj=_ptr(keep["proj"], ctypes.c_float),
              campos=_ptr(keep["campos"], ctypes.c_float), tan_fovx=float(tanfovx), tan_fovy=float(tanfovy))
    gx, gy = (W + 15) // 16, (H + 15) // 16
    o = dict(color=np.zeros((3, H, W), f4), depth=np.zeros((1, H, W), f4), radii=np.zeros(P, np.int32),
             means2D=np.zeros((P, 2), f4), depths=np.zeros(P, f4), conic_opacity=np.zeros((P, 4), f4),
             rgb=np.zeros((P, 3), f4), clamped=np.zeros((P, 3), np.uint8), tiles_touched=np.zeros(P, np.int32),
             final_T=np.zeros((H, W), f4), n_contrib=np.zeros((H, W), np.int32),
             ranges=np.zeros((gx * gy, 2), np.int32))
    fo = _FwdOut(out_color=_ptr(o["color"], ctypes.c_float), out_depth=_ptr(o["depth"], ctypes.c_float),
                 radii=_ptr(o["radii"], ctypes.c_int), means2D=_ptr(o["means2D"], ctypes.c_float),
                 depths=_ptr(o["depths"], ctypes.c_float), conic_opacity=_ptr(o["conic_opacity"], ctypes.c_float),
                 rgb=_ptr(o["rgb"], ctypes.c_float), clamped=_ptr(o["clamped"], ctypes.c_ubyte),
                 tiles_touched=_ptr(o["tiles_touched"], ctypes.c_int), final_T=_ptr(o["final_T"], ctypes.c_float),
                 n_contrib=_ptr(o["n_contrib"], ctypes.c_int), ranges=_ptr(o["ranges"], ctypes.c_int))
    handle = ctypes.c_void_p()
    _check("ref_forward", lib.ref_forward(ctypes.byref(inp), ctypes.byref(fo), ctypes.byref(handle)))
    ctx = _Context(handle)
    n = int(fo.num_rendered)
    pl = np.zeros(n, np.int32)
    _check("ref_point_list", lib.ref_point_list(ctx.handle, _ptr(pl, ctypes.c_int), n))
    # invisible Gaussians keep whatever the chunk held (zeros here); the oracle leaves zeros as well
    keep.update(ctx=ctx, dtype=np.dtype(f4), M=M)
    z = np.zeros((H, W), bool)
    return ForwardResult(num_rendered=n, point_list=pl, pair_evals=0, _keep=keep, unstable=np.zeros(P, bool),
                         unstable_pix=z, unstable_depth_pix=z.copy(), **o)


def backward(fr: ForwardResult, dL_dcolor, *, power=1, **_ignored) -> dict:
    """Rasterizer::backward of the reference (always BACKWARD::renderFused, the oracle's FUSED mode, with
    grad_power = power) on the state of ``fr`` (a result of ``reference.forward``).  Returns the eight
    gradient arrays of rasterize_points.cu under ``harness.GRAD_KEYS``.  Float atomics: two calls differ
    in the last bits."""
    lib = _load()
    ctx = fr._keep.get("ctx")
    if lib is None or ctx is None or not ctx.handle:
        raise RuntimeError("reference.backward needs a frame of reference.forward")
    P = fr.radii.shape[0]
    M = fr._keep["M"]
    H, W = fr.final_T.shape
    f4 = np.float32
    g = dict(dmeans2D=np.zeros((P, 3), f4), dcolors=np.zeros((P, 3), f4), dopacity=np.zeros((P, 1), f4),
             dmeans3D=np.zeros((P, 3), f4), dcov3D=np.zeros((P, 6), f4), dsh=np.zeros((P, M, 3), f4),
             dscales=np.zeros((P, 3), f4), drot=np.zeros((P, 4), f4))
    go = _Grads(**{k: _ptr(v if v.size else None, ctypes.c_float) for k, v in g.items()})
    dpix = np.ascontiguousarray(np.asarray(dL_dcolor, f4).reshape(3, H, W))
    _check("ref_backward", lib.ref_backward(ctx.handle, _ptr(dpix, ctypes.c_float), int(power), ctypes.byref(go)))
    return g


def mark_visible(means3D, view, proj) -> np.ndarray:
    """Rasterizer::markVisible of the reference."""
    lib = _load()
    if lib is None:
        raise RuntimeError(why_unavailable())
    m = _arr(means3D, np.float32).reshape(-1, 3)
    v = _arr(view, np.float32).reshape(-1)
    p = _arr(proj, np.float32).reshape(-1)
    if v.size != 16 or p.size != 16:
        raise ValueError("view and proj are 4x4")
    out = np.zeros(m.shape[0], np.uint8)
    _check("ref_mark_visible", lib.ref_mark_visible(m.shape[0], _ptr(m, ctypes.c_float), _ptr(v, ctypes.c_float),
                                                    _ptr(p, ctypes.c_float), _ptr(out, ctypes.c_ubyte)))
    return out.astype(bool)
