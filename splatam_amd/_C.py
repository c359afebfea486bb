"""Torch <-> C-ABI marshalling for libgsr.so: the drop-in for the reference's
pybind11 extension ``_C`` (hessian-diff-gaussian-rasterization-w-depth/ext.cpp:15-18).

Same three functions, same positional arguments, same return tuples as
rasterize_points.cu:35-216.  Tensors are turned into raw device pointers
(``.contiguous()`` float32, empty tensor -> NULL exactly like the reference's
``data_ptr()`` of an empty tensor), the current torch stream of the Gaussians'
device is passed down, and the opaque state buffers are allocated as uint8
torch tensors through the C allocator callback (replacing
``resizeFunctional``, rasterize_points.cu:27-33).

There is no CPU fallback: if libgsr.so is missing or the tensors are not on a
ROCm device, these functions raise.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from typing import NamedTuple

import torch

from ._lib import ALLOC_FN, GsrGaussians, GsrGrads, GsrSettings, GsrTrackXform, lib

_tls = threading.local()


def _alloc(ctx, kind, nbytes):  # called from C, under the GIL
    try:
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=_tls.device)
        _tls.buffers[int(kind)] = t
        return t.data_ptr()
    except Exception as exc:  # pragma: no cover - reported through the NULL return
        _tls.alloc_error = exc
        return None


_ALLOC_CB = ALLOC_FN(_alloc)

# The native torch binding (csrc/gsr_torch.cpp, built in-tree by splatam_amd.build next to libgsr.so) takes
# the drop-in path's per-iteration calls -- rasterize_gaussians in dynamic mode and
# rasterize_gaussians_backward -- at a fraction of this module's Python host cost; the same library
# calls, so the same bits.  GSR_NATIVE_BINDING=0 keeps them on ctypes (A/B, tests).  The binding links the
# in-tree libgsr.so, so a library loaded from another path (GSR_LIB: A/B builds) keeps every call on ctypes.
_NATIVE_ON = os.environ.get("GSR_NATIVE_BINDING", "1") != "0" and not os.environ.get("GSR_LIB")
_native_mod = None


def _native():
    """The native binding module, or None when it cannot be imported (stale or missing build): a warning once,
    and every call stays on the ctypes binding of the same libgsr.so."""
    global _native_mod, _NATIVE_ON
    if _native_mod is None:
        try:
            from . import _gsr_torch  # noqa: F401  (run `python -m splatam_amd.build` to rebuild it)
        except ImportError as exc:
            import warnings
            warnings.warn(f"splatam_amd: native torch binding unavailable ({exc}); using the ctypes binding of "
                          "libgsr.so", RuntimeWarning)
            _NATIVE_ON = False
            return None
        _native_mod = _gsr_torch
    return _native_mod


_EMPTY = torch.Tensor([])


def _t(x):  # None -> the empty tensor the reference passes for an absent input
    return _EMPTY if x is None else x


def _begin(device):
    _tls.device = device
    _tls.buffers = {}
    _tls.alloc_error = None


def _check(rc: int, what: str):
    if rc < 0:
        err = getattr(_tls, "alloc_error", None)
        msg = lib.gsr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what}: {msg}" + (f" ({err})" if err else ""))


def _dev_f32(t: torch.Tensor, device, name: str) -> torch.Tensor | None:
    """Contiguous float32 on `device`, or None for an empty tensor (-> NULL)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected scalar type Float but found {t.dtype}")
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


# The camera tensors (bg, viewmatrix, projmatrix, campos) are the same objects on every call of an
# iteration, and SplaTAM passes the matrices as transposed views (utils/recon_helpers.py setup_camera):
# each call's .contiguous() was a copy kernel (8 launches per RGB + depth fwd+bwd unit).  The copy is
# reused while the source tensor object is alive and unmodified (weak reference + version counter, which
# views share with their base), on the same stream, and never during stream capture (a captured graph must
# re-copy on replay).  GSR_CAM_CACHE=0 disables it.
_CAM_CACHE = os.environ.get("GSR_CAM_CACHE", "1") != "0"


def _cam_f32(t: torch.Tensor, device, name: str, stream: int) -> torch.Tensor | None:
    if t is None or t.numel() == 0:
        return None
    if t.dtype == torch.float32 and t.device == device and t.is_contiguous():
        return t
    if not _CAM_CACHE or torch.cuda.is_current_stream_capturing():
        return _dev_f32(t, device, name)
    cache = getattr(_tls, "cam_cache", None)
    if cache is None:
        cache = _tls.cam_cache = {}
    e = cache.get(id(t))
    if e is not None and e[0]() is t and e[1] == t._version and e[2] == stream and e[3].device == device:
        return e[3]
    c = _dev_f32(t, device, name)
    if len(cache) >= 64:  # drop the dead entries; still full: the oldest half (bounded either way)
        for k in [k for k, v in cache.items() if v[0]() is None]:
            del cache[k]
        if len(cache) >= 64:
            for k in list(cache)[:32]:
                del cache[k]
    cache[id(t)] = (weakref.ref(t), t._version, stream, c)
    return c


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _settings(bg, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, H, W, scale_modifier, degree, prefiltered,
              device, stream=None):
    if stream is None:
        stream = _stream(device)
    keep = [_cam_f32(bg, device, "bg", stream), _cam_f32(viewmatrix, device, "viewmatrix", stream),
            _cam_f32(projmatrix, device, "projmatrix", stream), _cam_f32(campos, device, "campos", stream)]
    s = GsrSettings(image_height=int(H), image_width=int(W), tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy),
                    bg=_ptr(keep[0]), scale_modifier=float(scale_modifier), viewmatrix=_ptr(keep[1]),
                    projmatrix=_ptr(keep[2]), sh_degree=int(degree), campos=_ptr(keep[3]),
                    prefiltered=int(bool(prefiltered)), binning=binning_mode())
    return s, keep


def _gaussians(means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, device):
    P = means3D.size(0)
    M = sh.size(1) if (sh is not None and sh.numel() > 0 and sh.dim() >= 2 and sh.size(0) != 0) else 0
    keep = [_dev_f32(means3D, device, "means3D"), _dev_f32(sh, device, "sh") if M else None,
            _dev_f32(colors, device, "colors"), _dev_f32(opacity, device, "opacity"),
            _dev_f32(scales, device, "scales"), _dev_f32(rotations, device, "rotations"),
            _dev_f32(cov3D_precomp, device, "cov3D_precomp")]
    g = GsrGaussians(P=P, M=M, means3D=_ptr(keep[0]), shs=_ptr(keep[1]), colors_precomp=_ptr(keep[2]),
                     opacities=_ptr(keep[3]), scales=_ptr(keep[4]), rotations=_ptr(keep[5]),
                     cov3D_precomp=_ptr(keep[6]))
    return g, keep, M


class TrackXform(NamedTuple):
    """The transform a static forward forms inside its preprocess: gsr_track_xform (include/gsr_glue.h) by field,
    as the tensors and addresses it is filled from (`xform_struct`).  The forward's means3D, colors2, opacity,
    scales and rotations arguments are then the transform's OUTPUTS: preallocated contiguous float32, written when
    store_rendervars is true (the mapping forward refuses anything else).  Built by glue.map_transform(defer=...)
    and glue.tracking_iteration; read by rasterize_gaussians_dual(xform=) and track_forward_dual_static(xform=)."""
    means_world: torch.Tensor
    unnorm_rot: torch.Tensor
    logit_opac: torch.Tensor
    log_scales: torch.Tensor
    scale_cols: int
    cam_q: int        # address of the pose column's quaternion (stride q_stride floats) ...
    cam_t: int        # ... and of its translation
    q_stride: int
    w2c: torch.Tensor
    store_rendervars: bool = True
    alive: torch.Tensor | None = None  # uint8 [P], 0 = culled
    keep: tuple = ()  # the tensors cam_q / cam_t point into: alive as long as the record is


def xform_struct(x: TrackXform) -> GsrTrackXform:
    return GsrTrackXform(means_world=x.means_world.data_ptr(), unnorm_rot=x.unnorm_rot.data_ptr(),
                         logit_opac=x.logit_opac.data_ptr(), log_scales=x.log_scales.data_ptr(),
                         scale_cols=int(x.scale_cols), cam_q=x.cam_q, cam_t=x.cam_t, q_stride=int(x.q_stride),
                         w2c=x.w2c.data_ptr(), store_rendervars=int(bool(x.store_rendervars)), alive=_ptr(x.alive))


def _check_status(status, device):
    if status is None or status.device != device or status.numel() < 4:
        raise RuntimeError("a static forward needs a device status tensor of 4 int32")


def _check_alive(alive, P, device):
    if alive is not None and (alive.device != device or alive.dtype != torch.uint8 or alive.numel() != P or
                              not alive.is_contiguous()):
        raise RuntimeError("alive must be a contiguous uint8 tensor of P entries on the render device")


def _check_xform_outputs(device, *outs):
    if any(t is None or not t.is_contiguous() or t.dtype != torch.float32 or t.device != device for t in outs):
        raise RuntimeError("a forward with xform writes means3D, colors2, opacity, scales and rotations: they must "
                           "be contiguous float32 tensors on the device")


def _settings_of(st, prefiltered):
    """_settings' leading arguments from a GaussianRasterizationSettings."""
    return (st.bg, st.viewmatrix, st.projmatrix, st.campos, st.tanfovx, st.tanfovy, int(st.image_height),
            int(st.image_width), st.scale_modifier, st.sh_degree, prefiltered)


def _forward_state(R, geomBuffer, binningBuffer, imageBuffer):
    """The backwards' (num_rendered, geometry, binning, image) segment: what their forward returned."""
    return (int(R), geomBuffer.data_ptr(), binningBuffer.data_ptr() if binningBuffer.numel() else None,
            imageBuffer.data_ptr())


class _Frame:
    """What the dual and tracking entry points share around their one library call: the settings and Gaussians
    structs (their tensors kept alive here), then per call a fresh allocator state, the call itself --
    fn(settings, gaussians, *middle, allocator, NULL, stream) -- its error check and the buffers it allocated.
    A family's variants differ in `fn` and in the segments of `middle`; a new variant's argument goes into the
    segment it belongs to, once."""

    def __init__(self, device, settings, gaussians):
        self.device, self.stream = device, _stream(device)
        self.s, self._keep_s = _settings(*settings, device, self.stream)
        self.g, self.keep_g, _ = _gaussians(*gaussians, device)

    def call(self, what, fn, *middle, release=False):
        """(return value, {kind: buffer}); release: the buffers are scratch, handed back to torch's allocator."""
        _begin(self.device)
        rc = fn(ctypes.byref(self.s), ctypes.byref(self.g), *middle, _ALLOC_CB, None, self.stream)
        _check(rc, what)
        bufs = _tls.buffers
        if release:
            _tls.buffers = {}
        return int(rc), bufs


# ---------------------------------------------------------------------------------------------
# Geometry reuse across consecutive calls (SURVEY.md 8(f) row 1 for unchanged callers): SplaTAM
# renders RGB and then the depth/silhouette image of the same Gaussians from the same camera
# (scripts/splatam.py:255,259), two RasterizeGaussiansCUDA calls whose preprocess, binning and
# tile sort are identical.  The second call reuses the first call's geometry / binning / image
# buffers when
#   * means3D and the camera tensors are the same storage at the same version, the scalar
#     settings and P are equal, the colours are precomputed (no SH) and no cov3D is given,
#   * the first call's buffers and its rotations / opacities / scales are still alive and
#     unmodified (weak references + tensor versions), and
#   * this call's rotations / opacities / scales equal the first call's bitwise -- compared on the
#     device by gsr_forward_reuse_if_equal, which enqueues the reuse and the full forward each gated on
#     the comparison, so the host waits once, on the counter copy every dynamic forward waits on.
# On by default (GSR_GEOM_CACHE=0 or set_geom_cache(False) disables it); the native binding
# (gsr_torch.cpp) applies the same rules.  (Until ABI 8 the comparison was read back by a second host
# synchronisation, which made the reuse slower than two full calls: profiles/r3_unit_ab.txt.)
_GEOM_CACHE = os.environ.get("GSR_GEOM_CACHE", "1") != "0"
REUSE_STATS = {"hits": 0, "misses": 0}  # eligible calls that did / did not reuse (ctypes path)


def set_geom_cache(on: bool):
    """Geometry reuse on / off for both bindings (tests, A/B runs)."""
    global _GEOM_CACHE
    _GEOM_CACHE = bool(on)
    nat = _native()
    if nat is not None:
        nat.set_geom_cache(bool(on))


def reuse_stats() -> dict:
    """Hits / misses of the geometry reuse over both bindings ("content": misses on the device comparison)."""
    out = dict(REUSE_STATS)
    nat = _native() if _NATIVE_ON else None
    if nat is not None:
        h, m, c = nat.reuse_stats()
        out["hits"] = out.get("hits", 0) + int(h)
        out["misses"] = out.get("misses", 0) + int(m)
        out["content"] = out.get("content", 0) + int(c)
    return out


class _Prev:
    """The last eager single-call forward on a (thread, device)."""
    __slots__ = ("key", "shared", "shared_versions", "others", "versions", "bufs", "radii", "radii_version",
                 "num_rendered")


def _try_reuse(key, shared, others, P):
    """The previous call's state if this call may reuse it (the host checks; the device compares the rest).
    key: device, stream and scalar settings; shared: tensors that must be the very same objects
    (means3D, bg, viewmatrix, projmatrix, campos) at the same versions."""
    prev = getattr(_tls, "prev", {}).get(key[0])
    if prev is None or prev.key != key:
        return _miss("key")
    for k, (r, v, t) in enumerate(zip(prev.shared, prev.shared_versions, shared)):
        if (r is None) != (t is None):
            return _miss(f"shared{k}_none")
        if t is not None and r() is None:
            return _miss(f"shared{k}_dead")
        if t is not None and r() is not t:
            return _miss(f"shared{k}_other")
        if t is not None and t._version != v:
            return _miss(f"shared{k}_version")
    po = [r() for r in prev.others]
    bufs = [r() for r in prev.bufs]
    radii = prev.radii()
    if any(t is None for t in po) or any(b is None for b in bufs) or radii is None:
        return _miss("dead")
    if any(t._version != v for t, v in zip(po, prev.versions)) or radii._version != prev.radii_version:
        return _miss("version")  # (radii: copied into this call's, so an in-place edit must miss)
    if any(a is None or a.shape != b.shape for a, b in zip(others, po)):
        return _miss("shape")
    return prev, bufs, radii, po


def _miss(reason):
    REUSE_STATS[reason] = REUSE_STATS.get(reason, 0) + 1
    return None


def _remember(key, shared, others, bufs, radii, num_rendered):
    if not hasattr(_tls, "prev"):
        _tls.prev = {}
    p = _Prev()
    p.key = key
    p.shared = [None if t is None else weakref.ref(t) for t in shared]
    p.shared_versions = [None if t is None else t._version for t in shared]
    p.others = [weakref.ref(t) for t in others]
    p.versions = [t._version for t in others]
    p.bufs = [weakref.ref(b) for b in bufs]
    p.radii = weakref.ref(radii)
    p.radii_version = radii._version
    p.num_rendered = num_rendered
    _tls.prev[key[0]] = p


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, capacity=0, status=None, alive=None):
    """RasterizeGaussiansCUDA (rasterize_points.cu:35-115).

    Returns (num_rendered, color[3,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer, depth[1,H,W]).
    capacity > 0 selects gsr_forward_static (no host synchronisation, HIP-graph capturable; `status` is a
    device int32[4] receiving the sticky counters, and num_rendered is the capacity).  alive (static mode
    only): a device uint8 [P] mask, 0 = culled (gsr_forward_static_alive: radius 0, no instances).
    """
    if capacity <= 0 and alive is not None:
        raise RuntimeError("the alive mask and the fused transform need the static (capacity > 0) forward")
    if (_NATIVE_ON and capacity <= 0 and binning_mode() == BINNING_CULLED and _native() is not None):
        return _native().rasterize_gaussians(
            _t(background), means3D, _t(colors), _t(opacity), _t(scales), _t(rotations), float(scale_modifier),
            _t(cov3D_precomp), _t(viewmatrix), _t(projmatrix), float(tan_fovx), float(tan_fovy), int(image_height),
            int(image_width), _t(sh), int(degree), _t(campos), bool(prefiltered))
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("splatam_amd rasterizer runs on ROCm devices only (no CPU fallback); "
                           f"means3D is on {device}")
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=device)
    if P == 0:
        empty = torch.empty(0, dtype=torch.uint8, device=device)
        return (0, torch.zeros(3, H, W, **f32), torch.zeros(0, dtype=torch.int32, device=device), empty,
                empty.clone(), empty.clone(), torch.zeros(1, H, W, **f32))
    with torch.cuda.device(device):
        stream = _stream(device)
        s, keep_s = _settings(background, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, H, W, scale_modifier,
                              degree, prefiltered, device, stream)
        g, keep_g, _ = _gaussians(means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, device)
        out_color = torch.empty(3, H, W, **f32)
        out_depth = torch.empty(1, H, W, **f32)
        radii = torch.empty(P, dtype=torch.int32, device=device)
        reusable = (_GEOM_CACHE and capacity <= 0 and keep_g[2] is not None and keep_g[1] is None and
                    keep_g[6] is None and None not in (keep_g[3], keep_g[4], keep_g[5]))
        if reusable:
            others = (keep_g[5], keep_g[3], keep_g[4])  # rotations, opacities, scales as passed down
            # identity of the caller's own tensors (SplaTAM's viewmatrix / projmatrix are transposed
            # views, so the contiguous copies passed down are new objects on every call)
            shared = (means3D, background, viewmatrix, projmatrix, campos)
            key = (device, stream, P, H, W, float(tan_fovx), float(tan_fovy), float(scale_modifier), int(degree),
                   bool(prefiltered))
            hit = _try_reuse(key, shared, others, P)
            if hit is not None:
                prev, bufs, prev_radii, po = hit
                _begin(device)
                arr_a = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in others])
                arr_b = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in po])
                arr_n = (ctypes.c_longlong * 3)(*[t.numel() for t in others])
                reused = ctypes.c_int(0)
                n = lib.gsr_forward_reuse_if_equal(
                    ctypes.byref(s), ctypes.byref(g), 3, arr_a, arr_b, arr_n, int(prev.num_rendered),
                    bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), prev_radii.data_ptr(),
                    out_color.data_ptr(), out_depth.data_ptr(), radii.data_ptr(), ctypes.byref(reused), _ALLOC_CB,
                    None, stream)
                _check(n, "rasterize_gaussians (geometry reuse)")
                if reused.value:
                    REUSE_STATS["hits"] += 1
                    return (int(n), out_color, radii, _tls.buffers[0], bufs[1], bufs[2], out_depth)
                _miss("content")  # a full forward ran: this call's own buffers
                REUSE_STATS["misses"] += 1
                bufs = _tls.buffers
                _remember(key, shared, others, (bufs[0], bufs[1], bufs[2]), radii, int(n))
                return (int(n), out_color, radii, bufs[0], bufs[1], bufs[2], out_depth)
            REUSE_STATS["misses"] += 1
        _begin(device)
        if capacity > 0:
            _check_status(status, device)
            _check_alive(alive, P, device)
            if alive is not None:
                n = lib.gsr_forward_static_alive(ctypes.byref(s), ctypes.byref(g), int(capacity), status.data_ptr(),
                                                 out_color.data_ptr(), out_depth.data_ptr(), radii.data_ptr(),
                                                 alive.data_ptr(), _ALLOC_CB, None, stream)
            else:
                n = lib.gsr_forward_static(ctypes.byref(s), ctypes.byref(g), int(capacity), status.data_ptr(),
                                           out_color.data_ptr(), out_depth.data_ptr(), radii.data_ptr(), _ALLOC_CB,
                                           None, stream)
        else:
            n = lib.gsr_forward(ctypes.byref(s), ctypes.byref(g), out_color.data_ptr(), out_depth.data_ptr(),
                                radii.data_ptr(), _ALLOC_CB, None, stream)
        _check(n, "rasterize_gaussians")
        bufs = _tls.buffers
        if reusable:
            _remember(key, shared, others, (bufs[0], bufs[1], bufs[2]), radii, int(n))
        return (int(n), out_color, radii, bufs[0], bufs[1], bufs[2], out_depth)


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree,
                                 campos, geomBuffer, R, binningBuffer, imageBuffer, power=1, needs=None):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-196).

    Returns (dmeans2D[P,3], dcolors[P,3], dopacity[P,1], dmeans3D[P,3], dcov3D[P,6], dsh[P,M,3],
    dscales[P,3], drotations[P,4]).  `needs` (8 bools in that order) skips the gradients nobody
    wants: they come back as None and their per-pair sums are not formed.  With power != 1 it is
    honoured only for the Fisher-selective request -- dmeans3D (+ dopacity) of a render with
    precomputed colours (scripts/ros_handler.py:884-889 reads no other gradient) -- which runs the
    4-value-per-pair kernel; any other power != 1 request forms every gradient.
    """
    if _NATIVE_ON and _native() is not None:
        return tuple(_native().rasterize_gaussians_backward(
            _t(background), means3D, radii, _t(colors), _t(scales), _t(rotations), float(scale_modifier),
            _t(cov3D_precomp), _t(viewmatrix), _t(projmatrix), float(tan_fovx), float(tan_fovy), dL_dout_color, _t(sh),
            int(degree), _t(campos), geomBuffer, int(R), binningBuffer, imageBuffer, int(power),
            [] if needs is None else [bool(x) for x in needs]))
    device = means3D.device
    P = means3D.size(0)
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = sh.size(1) if (sh is not None and sh.numel() > 0 and sh.size(0) != 0) else 0
    f32 = dict(dtype=torch.float32, device=device)
    if needs is not None and int(power) != 1:
        fisher = M == 0 and colors is not None and colors.numel() > 0 and \
            not any(bool(needs[k]) for k in (0, 1, 4, 5, 6, 7))
        if not fisher:
            needs = None
    needs = [True] * 8 if needs is None else list(needs)
    needs[3] = True  # dmeans3D is always produced
    shapes = [(P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4)]
    out = [torch.empty(*sh_, **f32) if nd else None for sh_, nd in zip(shapes, needs)]
    if P == 0:
        return tuple(out)
    with torch.cuda.device(device):
        stream = _stream(device)
        s, keep_s = _settings(background, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, H, W, scale_modifier,
                              degree, False, device, stream)
        # opacities are not an input of the backward (rasterize_points.cu:117-139): they live in geomBuffer
        g, keep_g, _ = _gaussians(means3D, sh, colors, None, scales, rotations, cov3D_precomp, device)
        dpix = _dev_f32(dL_dout_color, device, "dL_dout_color")
        radii_c = radii.to(device=device, dtype=torch.int32).contiguous()
        grads = GsrGrads(*[o.data_ptr() if (o is not None and o.numel() > 0) else None for o in out])
        _begin(device)
        rc = lib.gsr_backward(ctypes.byref(s), ctypes.byref(g), radii_c.data_ptr(), dpix.data_ptr(), int(R),
                              geomBuffer.data_ptr(), binningBuffer.data_ptr() if binningBuffer.numel() else None,
                              imageBuffer.data_ptr(), int(power), ctypes.byref(grads), _ALLOC_CB, None,
                              stream)
        _check(rc, "rasterize_gaussians_backward")
        _tls.buffers = {}  # scratch is released to torch's caching allocator (stream-ordered)
        return tuple(out)


def rasterize_gaussians_dual(background, means3D, colors, colors2, opacity, scales, rotations, scale_modifier,
                             cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                             degree, campos, prefiltered, capacity=0, status=None, alive=None, xform=None):
    """gsr_forward_dual: rasterize_gaussians with a second precomputed colour set
    composited in the same pass.  Returns (num_rendered, color, color2, radii,
    geomBuffer, binningBuffer, imgBuffer, depth).  capacity > 0 selects
    gsr_forward_dual_static (no host synchronisation; `status` is a device int32[4]
    receiving the counters, and num_rendered is the capacity).  alive (static mode only): a
    device uint8 [P] mask, 0 = pruned (gsr_forward_dual_static_alive: culled, radius 0).
    xform (static mode only): a TrackXform -- the mapping transform inside preprocess
    (gsr_forward_dual_static_xf: it always stores the rendervars and its mask is the `alive` argument; the record's
    store_rendervars and alive fields are the tracking forward's and are not read here).
    The library's arguments by segment: colors2 [, xform] [, capacity, status], the four outputs [, alive]."""
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("splatam_amd rasterizer runs on ROCm devices only (no CPU fallback); "
                           f"means3D is on {device}")
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=device)
    if colors2 is None or colors2.shape != (P, 3):
        raise RuntimeError("colors2 must have dimensions (num_points, 3)")
    if capacity <= 0 and (alive is not None or xform is not None):
        raise RuntimeError("the alive mask and the fused transform need the static (capacity > 0) forward")
    with torch.cuda.device(device):
        fr = _Frame(device, (background, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, H, W, scale_modifier,
                             degree, prefiltered), (means3D, sh, colors, opacity, scales, rotations, cov3D_precomp))
        c2 = _dev_f32(colors2, device, "colors2")
        out_color = torch.empty(3, H, W, **f32)
        out_color2 = torch.empty(3, H, W, **f32)
        out_depth = torch.empty(1, H, W, **f32)
        radii = torch.empty(P, dtype=torch.int32, device=device)
        fn, static, mask = lib.gsr_forward_dual, (), ()
        if capacity > 0:
            _check_status(status, device)
            _check_alive(alive, P, device)
            static = (int(capacity), status.data_ptr())
            if xform is not None:
                _check_xform_outputs(device, means3D, colors2, opacity, scales, rotations)
                xf = xform_struct(xform)
                xf.store_rendervars, xf.alive = 1, _ptr(alive)  # (as before the record: its own two are not read)
                fn, static = lib.gsr_forward_dual_static_xf, (ctypes.byref(xf),) + static
            elif alive is not None:
                fn, mask = lib.gsr_forward_dual_static_alive, (alive.data_ptr() if P else None,)
            else:
                fn = lib.gsr_forward_dual_static
        n, bufs = fr.call("rasterize_gaussians_dual", fn, _ptr(c2), *static, out_color.data_ptr(),
                          out_color2.data_ptr(), out_depth.data_ptr(), radii.data_ptr() if P else None, *mask)
        return (n, out_color, out_color2, radii, bufs[0], bufs[1], bufs[2], out_depth)


def rasterize_gaussians_dual_backward(background, means3D, radii, colors, colors2, scales, rotations, scale_modifier,
                                      cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                      dL_dout_color2, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                      needs=None, dl2_channels=3, sh_adam=None, means2D_color1=False):
    """gsr_backward_dual.  Returns (dmeans2D, dcolors, dcolors2, dopacity, dmeans3D, dcov3D, dsh, dscales,
    drotations); geometric gradients are the sums over both colour sets.  `needs` (9 bools in that
    order, default all) skips the gradients nobody wants: they come back as None and the kernels do
    not form their per-pair sums.  dl2_channels=1 promises dL_dout_color2[1:] == 0 (only the depth
    channel is differentiated): those channels are not read and dcolors2[:, 1:] comes back zero.
    sh_adam: a GsrMapAdam (the mapping optimizer, colour group = index 4, step = the upcoming one): the
    colour Adam step is applied to `sh` in place (gsr_backward_dual_sh_adam) and dsh comes back None.
    means2D_color1: dmeans2D is the FIRST colour set's own means2D gradient instead of the sum over both
    (gsr_backward_dual_m2d: the mapping form only -- dl2_channels=1, dcolors or SH, dcolors2 and dopacity
    wanted, no sh_adam)."""
    if means2D_color1 and sh_adam is not None:
        raise ValueError("means2D_color1: gsr_backward_dual_sh_adam has no such sibling (step SH colours with "
                         "glue.FusedAdam)")
    device = means3D.device
    P = means3D.size(0)
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = sh.size(1) if (sh is not None and sh.numel() > 0 and sh.size(0) != 0) else 0
    f32 = dict(dtype=torch.float32, device=device)
    needs = [True] * 9 if needs is None else list(needs)
    needs[4] = True  # dmeans3D is always produced
    if sh_adam is not None:
        needs[6] = False  # dsh: consumed by the fused colour Adam step
    shapes = [(P, 3), (P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4)]
    res = [torch.empty(*sh_, **f32) if nd else None for sh_, nd in zip(shapes, needs)]
    out = [res[0], res[1], res[3], res[4], res[5], res[6], res[7], res[8]]
    dcolors2 = res[2]
    if P == 0:
        return (out[0], out[1], dcolors2, *out[2:])
    with torch.cuda.device(device):
        # opacities are not an input of the backward (rasterize_points.cu:117-139): they live in geomBuffer
        fr = _Frame(device, (background, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, H, W, scale_modifier,
                             degree, False), (means3D, sh, colors, None, scales, rotations, cov3D_precomp))
        c2 = _dev_f32(colors2, device, "colors2")
        dpix = _dev_f32(dL_dout_color, device, "dL_dout_color")
        dpix2 = _dev_f32(dL_dout_color2, device, "dL_dout_color2")
        radii_c = radii.to(device=device, dtype=torch.int32).contiguous()
        grads = GsrGrads(*[o.data_ptr() if (o is not None and o.numel() > 0) else None for o in out])
        fn, step = lib.gsr_backward_dual, ()
        if means2D_color1:  # the same tensor comes back as dmeans2D; the sum over both renders is not formed
            if out[0] is None:
                raise ValueError("means2D_color1 needs dmeans2D among `needs`")
            grads.dmeans2D = None
            fn, step = lib.gsr_backward_dual_m2d, (out[0].data_ptr(),)
        if sh_adam is not None:
            if fr.keep_g[1] is None or fr.keep_g[1].data_ptr() != sh.data_ptr():
                raise RuntimeError("sh_adam steps the SH coefficients in place: sh must be contiguous float32")
            fn, step = lib.gsr_backward_dual_sh_adam, (ctypes.byref(sh_adam),)
        fr.call("rasterize_gaussians_dual_backward", fn, radii_c.data_ptr(), _ptr(c2), dpix.data_ptr(),
                dpix2.data_ptr(), *_forward_state(R, geomBuffer, binningBuffer, imageBuffer), ctypes.byref(grads),
                _ptr(dcolors2), int(dl2_channels), *step, release=True)
        return (out[0], out[1], dcolors2, *out[2:])


BINNING_CULLED, BINNING_REFERENCE = 0, 1  # gsr_settings.binning (include/gsr.h)


def binning_mode() -> int:
    """The calling thread's gsr_settings.binning for the calls it makes: BINNING_CULLED (default) or
    BINNING_REFERENCE inside `reference_binning()`.  Per thread and per call -- the library keeps no mode."""
    return getattr(_tls, "binning", BINNING_CULLED)


class reference_binning:
    """Context (this thread only): the forwards built here -- eager, static or captured in a HIP graph -- list
    every rect instance, i.e. rasterizer_impl.cu's num_rendered, ranges and (tile, depth, id) point list entry
    for entry (gsr_settings.binning = GSR_BINNING_REFERENCE).  Outside it the tile lists leave out the instances
    that reach no pixel of their tile.  Images, radii, num_rendered and gradients are the same bits either way;
    the oracle tests compare the lists themselves."""

    def __enter__(self):
        self.prev = binning_mode()
        _tls.binning = BINNING_REFERENCE
        return self

    def __exit__(self, *exc):
        _tls.binning = self.prev
        return False


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (rasterize_points.cu:198-216): bool[P], view_z > 0.001."""
    device = means3D.device
    P = means3D.size(0)
    present = torch.zeros(P, dtype=torch.bool, device=device)
    if P == 0:
        return present
    with torch.cuda.device(device):
        m = _dev_f32(means3D, device, "means3D")
        v = _dev_f32(viewmatrix, device, "viewmatrix")
        p = _dev_f32(projmatrix, device, "projmatrix")
        rc = lib.gsr_mark_visible(P, m.data_ptr(), v.data_ptr(), p.data_ptr(), present.data_ptr(), _stream(device))
        _check(rc, "mark_visible")
    return present


def track_backward_dual(settings, means3D, radii, colors, colors2, scales, rotations, dL_dout_color, dL_dout_color2,
                        geomBuffer, R, binningBuffer, imageBuffer, means_world, unnorm_rot, scale_cols, cam_q_ptr,
                        cam_t_ptr, q_stride, w2c, scratch, adam=None, dq_ptr=None, dt_ptr=None, track=None,
                        log_scales=None, records=None):
    """gsr_track_backward_dual (include/gsr_glue.h): the tracking backward with the pose chain fused into
    the per-Gaussian backward.  adam = (lr_q, lr_t, beta1, beta2, eps, state tensor) applies the Adam step
    to the pose in place; otherwise the pose gradient is written at dq_ptr / dt_ptr.  track: an optional
    GsrPoseTrack (best-candidate selection; the Adam step is skipped on an overflowing forward).
    log_scales: recompute the rendervars (means3D / rotations / scales) from the world-frame map
    instead of reading them (a forward run with store_rendervars = 0).  records: the per-instance sums of
    a fused forward (track_forward_dual_static(records=...)): gsr_track_backward_dual_records, only the
    per-Gaussian backward runs and the gradient images are not read (may be None)."""
    device = means3D.device
    with torch.cuda.device(device):
        fr = _Frame(device, _settings_of(settings, False), (means3D, None, colors, None, scales, rotations, None))
        c2 = _dev_f32(colors2, device, "colors2")
        lr_q, lr_t, b1, b2, eps, state = adam if adam is not None else (0.0, 0.0, 0.0, 0.0, 0.0, None)
        # the library's arguments by segment: radii, colors2 [, the gradient images], the forward's state, the pose
        # chain (the map, the pose column, the Adam step or the gradient's address, ...) [, records]
        fn, what, images, rec = lib.gsr_track_backward_dual, "track_backward_dual", (), ()
        if records is not None:
            fn, what, rec = lib.gsr_track_backward_dual_records, "track_backward_dual_records", (records.data_ptr(),)
        else:
            dpix = _dev_f32(dL_dout_color, device, "dL_dout_color")  # (named: alive until the call returns)
            dpix2 = _dev_f32(dL_dout_color2, device, "dL_dout_color2")
            images = (dpix.data_ptr(), dpix2.data_ptr())
        fr.call(what, fn, radii.data_ptr(), _ptr(c2), *images,
                *_forward_state(R, geomBuffer, binningBuffer, imageBuffer), means_world.data_ptr(),
                unnorm_rot.data_ptr(), int(scale_cols), cam_q_ptr, cam_t_ptr, int(q_stride), w2c.data_ptr(),
                float(lr_q), float(lr_t), float(b1), float(b2), float(eps), _ptr(state), dq_ptr, dt_ptr,
                scratch.data_ptr(), ctypes.byref(track) if track is not None else None, _ptr(log_scales), *rec,
                release=True)


def terms_ptr(terms: torch.Tensor, device) -> int:
    """The address of a `terms` output (the gsr_track_*_terms entries): two contiguous float32 on `device`."""
    if (not torch.is_tensor(terms) or terms.device != device or terms.dtype != torch.float32 or
            terms.numel() != 2 or not terms.is_contiguous()):
        raise RuntimeError("terms: a contiguous float32 tensor of 2 elements on the forward's device")
    return terms.data_ptr()


def track_forward_dual_static(settings, means3D, colors, colors2, opacity, scales, rotations, capacity, status, gt_im,
                              gt_depth, sil_thres, w_im, w_depth, seed, scratch, xform=None, records=None,
                              images=True, terms=None):
    """gsr_track_forward_dual_static (include/gsr_glue.h): the static dual forward with SplaTAM's
    tracking L1 loss and its gradient images formed in the render epilogue.  Returns (num_rendered=capacity,
    color, color2, radii, geomBuffer, binningBuffer, imgBuffer, depth, loss, dL_dim, dL_ddepth_sil).
    xform (a TrackXform): gsr_track_forward_dual_static_xf -- the tracking transform runs inside preprocess.
    records (with xform; device float32 of lib.gsr_track_records_floats(capacity)):
    gsr_track_forward_backward_dual_static_xf -- the tracking render backward runs in the same launch
    and leaves its per-instance sums in records (track_backward_dual(records=...)); dL_dim / dL_ddepth_sil
    come back None (not formed).  images=False (with records): the rendered images are not stored either
    (color, color2 and depth come back None; the loss and the backward consume them in registers).
    terms (device float32, 2 elements): the call's _terms sibling -- the loss's two weighted terms
    (w_im * image sum, w_depth * depth sum) are written there next to the loss."""
    st = settings
    device = means3D.device
    P = means3D.size(0)
    H, W = int(st.image_height), int(st.image_width)
    f32 = dict(dtype=torch.float32, device=device)
    if records is not None and xform is None:
        raise RuntimeError("track_forward_dual_static: records needs the transform-fused forward (xform)")
    if not images and records is None:
        raise RuntimeError("track_forward_dual_static: images=False needs the fused render (xform and records)")
    with torch.cuda.device(device):
        fr = _Frame(device, _settings_of(st, st.prefiltered), (means3D, None, colors, opacity, scales, rotations, None))
        c2 = _dev_f32(colors2, device, "colors2")
        gi, gd, sd = (_dev_f32(gt_im, device, "gt_im"), _dev_f32(gt_depth, device, "gt_depth"),
                      _dev_f32(seed, device, "seed"))
        out_color = out_color2 = out_depth = None
        if images:
            out_color, out_color2 = torch.empty(3, H, W, **f32), torch.empty(3, H, W, **f32)
            out_depth = torch.empty(1, H, W, **f32)
        radii = torch.empty(P, dtype=torch.int32, device=device)
        loss = torch.empty((), **f32)
        _check_status(status, device)
        # The library's arguments by segment: colors2 [, xform], capacity, status, the image outputs and radii | the
        # L1 block (targets, threshold, weights, seed, loss) [, terms] | the gradient images or, with the render
        # backward in the same launch, its records -- scratch between them.  The entry point's name says which
        # segments it takes.
        name, xf, dim, dds = "gsr_track_forward_dual_static", (), None, None
        if xform is not None:
            _check_xform_outputs(device, means3D, colors2, opacity, scales, rotations)
            _check_alive(xform.alive, P, device)
            xf_struct = xform_struct(xform)
            name, xf = name + "_xf", (ctypes.byref(xf_struct),)
        if records is not None:
            if (records.device != device or records.dtype != torch.float32 or not records.is_contiguous() or
                    records.numel() < lib.gsr_track_records_floats(int(capacity))):
                raise RuntimeError("records: contiguous float32 of gsr_track_records_floats(capacity) on the device")
            name = "gsr_track_forward_backward_dual_static_xf"
            tail = (scratch.data_ptr(), records.data_ptr())
        else:
            dim, dds = torch.empty(3, H, W, **f32), torch.empty(3, H, W, **f32)
            tail = (dim.data_ptr(), dds.data_ptr(), scratch.data_ptr())
        # the _terms sibling of each call: `terms` behind `loss`
        tp = () if terms is None else (terms_ptr(terms, device),)
        n, bufs = fr.call(name[4:], getattr(lib, name + "_terms" if tp else name), _ptr(c2), *xf, int(capacity),
                          status.data_ptr(), _ptr(out_color), _ptr(out_color2), _ptr(out_depth),
                          radii.data_ptr() if P else None, gi.data_ptr(), gd.data_ptr(), float(sil_thres),
                          float(w_im), float(w_depth), sd.data_ptr(), loss.data_ptr(), *tp, *tail)
        return (n, out_color, out_color2, radii, bufs[0], bufs[1], bufs[2], out_depth, loss, dim, dds)

