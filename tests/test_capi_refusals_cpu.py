"""The C entry points' refusals that need no device (csrc/gsr_capi.hip): return code and the full
gsr_last_error() text of every call that is turned away before the library's first HIP runtime call.

A table: one row per refusal, arguments by name over a set of defaults that would pass every such check
(small host buffers stand in for device memory: these checks compare pointers with NULL and never
dereference them).  The rows with two defects at once pin which message wins.

Not in the table, because the check sits behind a HIP call (the stream's device, the current device): `radii`
NULL, the allocator returning NULL, "dmeans3D output pointer required", the backward_power != 1 requests and
"missing binning buffer" -- tests/test_gpu_capi_paths.py has the first two.  Two refusals cannot be reached
through an exported entry point at all: "the fused render backward needs the static dual forward with the
L1 loss" (the only caller passing records has checked colors2, capacity and the loss pointers already; the
row `fused forward, validate fails` is the nearest reachable call) and "dual render supports
backward_power == 1 only" (every dual entry passes power 1).
"""
import ctypes

import pytest

from splatam_amd._lib import (ALLOC_FN, SIGNATURES, GsrGaussians, GsrGrads, GsrMapAdam, GsrPoseTrack, GsrSettings,
                              GsrTrackXform, lib)

INVALID, OK = -1, 0
_BUF = (ctypes.c_float * 64)()
D = ctypes.addressof(_BUF)  # a non-null pointer nobody dereferences


@ALLOC_FN
def _no_memory(ctx, kind, nbytes):  # (never reached by a refused call)
    return None


NO_ALLOC = ctypes.cast(None, ALLOC_FN)  # a NULL callback (ctypes takes no None for a function pointer)
_PTRS8 = (ctypes.c_void_p * 8)(*([D] * 8))
_NULLS8 = (ctypes.c_void_p * 8)()
_N8 = (ctypes.c_longlong * 8)(*([4] * 8))
_NEG8 = (ctypes.c_longlong * 8)(*([4, -1] + [4] * 6))
_REUSED = ctypes.c_int(0)

STRUCTS = {
    "settings": (GsrSettings, dict(image_height=32, image_width=48, tan_fovx=1.0, tan_fovy=1.0, bg=D,
                                   scale_modifier=1.0, viewmatrix=D, projmatrix=D, sh_degree=0, campos=D,
                                   prefiltered=0, binning=0)),
    "gaussians": (GsrGaussians, dict(P=4, M=0, means3D=D, shs=None, colors_precomp=D, opacities=D, scales=D,
                                     rotations=D, cov3D_precomp=None)),
    "grads": (GsrGrads, dict(dmeans2D=D, dcolors=D, dopacity=D, dmeans3D=D, dcov3D=D, dsh=D, dscales=D,
                             drotations=D)),
    "xform": (GsrTrackXform, dict(means_world=D, unnorm_rot=D, logit_opac=D, log_scales=D, scale_cols=1, cam_q=D,
                                  cam_t=D, q_stride=1, w2c=D, store_rendervars=1, alive=None)),
    "sh_adam": (GsrMapAdam, dict(exp_avg=(ctypes.c_void_p * 5)(*([D] * 5)),
                                 exp_avg_sq=(ctypes.c_void_p * 5)(*([D] * 5)), lr=(ctypes.c_double * 5)(*([1e-3] * 5)),
                                 step=1, beta1=0.9, beta2=0.999, eps=1e-8, status=None, capacity=0, halted=None)),
    "track": (GsrPoseTrack, None),
}
DEFAULTS = dict(
    colors2=D, out_color=D, out_color2=D, out_depth=D, radii=D, alloc=_no_memory, alloc_ctx=None, stream=None,
    capacity=64, status=D, gt_im=D, gt_depth=D, sil_thres=0.99, w_im=0.5, w_depth=1.0, dL_dloss=D, loss=D, dL_dim=D,
    dL_ddepth_sil=D, scratch=D, inst_records=D, alive=D, num_rendered=8, prev_geom=D, binning_buffer=D,
    image_buffer=D, geom_buffer=D, prev_radii=D, dL_dout_color=D, dL_dout_color2=D, power=1, dcolors2=D,
    dl2_channels=3, means_world=D, unnorm_rot=D, scale_cols=1, cam_q=D, cam_t=D, q_stride=1, w2c=D, lr_q=1e-3,
    lr_t=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, adam_state=D, dL_dcam_q=D, dL_dcam_t=D, log_scales=None, npairs=3,
    a=_PTRS8, b=_PTRS8, n=_N8, prev_num_rendered=8, prev_binning=D, prev_image=D, reused=ctypes.byref(_REUSED),
    P=4, means3D=D, viewmatrix=D, projmatrix=D, visible=D, flag=D)

_FWD_TAIL = ["alloc", "alloc_ctx", "stream"]
_L1 = ["gt_im", "gt_depth", "sil_thres", "w_im", "w_depth", "dL_dloss", "loss"]
_STATE = ["num_rendered", "geom_buffer", "binning_buffer", "image_buffer"]
_POSE = ["means_world", "unnorm_rot", "scale_cols", "cam_q", "cam_t", "q_stride", "w2c", "lr_q", "lr_t", "beta1",
         "beta2", "eps", "adam_state", "dL_dcam_q", "dL_dcam_t", "scratch", "track", "log_scales"]
_XF_HEAD = ["settings", "gaussians", "colors2", "xform", "capacity", "status", "out_color", "out_color2", "out_depth",
            "radii"]
_DUAL_BWD = ["settings", "gaussians", "radii", "colors2", "dL_dout_color", "dL_dout_color2", *_STATE, "grads",
             "dcolors2", "dl2_channels"]
PARAMS = {
    "gsr_forward": ["settings", "gaussians", "out_color", "out_depth", "radii", *_FWD_TAIL],
    "gsr_forward_dual": ["settings", "gaussians", "colors2", "out_color", "out_color2", "out_depth", "radii",
                         *_FWD_TAIL],
    "gsr_forward_static": ["settings", "gaussians", "capacity", "status", "out_color", "out_depth", "radii",
                           *_FWD_TAIL],
    "gsr_forward_dual_static": ["settings", "gaussians", "colors2", "capacity", "status", "out_color", "out_color2",
                                "out_depth", "radii", *_FWD_TAIL],
    "gsr_forward_dual_static_alive": ["settings", "gaussians", "colors2", "capacity", "status", "out_color",
                                      "out_color2", "out_depth", "radii", "alive", *_FWD_TAIL],
    "gsr_track_forward_dual_static": ["settings", "gaussians", "colors2", "capacity", "status", "out_color",
                                      "out_color2", "out_depth", "radii", *_L1, "dL_dim", "dL_ddepth_sil", "scratch",
                                      *_FWD_TAIL],
    "gsr_track_forward_dual_static_xf": [*_XF_HEAD, *_L1, "dL_dim", "dL_ddepth_sil", "scratch", *_FWD_TAIL],
    "gsr_track_forward_backward_dual_static_xf": [*_XF_HEAD, *_L1, "scratch", "inst_records", *_FWD_TAIL],
    "gsr_forward_dual_static_xf": [*_XF_HEAD, *_FWD_TAIL],
    "gsr_forward_reuse": ["settings", "gaussians", "num_rendered", "prev_geom", "binning_buffer", "image_buffer",
                          "prev_radii", "out_color", "out_depth", "radii", *_FWD_TAIL],
    "gsr_forward_reuse_if_equal": ["settings", "gaussians", "npairs", "a", "b", "n", "prev_num_rendered", "prev_geom",
                                   "prev_binning", "prev_image", "prev_radii", "out_color", "out_depth", "radii",
                                   "reused", *_FWD_TAIL],
    "gsr_bitwise_equal": ["npairs", "a", "b", "n", "flag", "stream"],
    "gsr_backward": ["settings", "gaussians", "radii", "dL_dout_color", *_STATE, "power", "grads", *_FWD_TAIL],
    "gsr_backward_dual": [*_DUAL_BWD, *_FWD_TAIL],
    "gsr_backward_dual_sh_adam": [*_DUAL_BWD, "sh_adam", *_FWD_TAIL],
    "gsr_track_backward_dual": ["settings", "gaussians", "radii", "colors2", "dL_dout_color", "dL_dout_color2",
                                *_STATE, *_POSE, *_FWD_TAIL],
    "gsr_track_backward_dual_records": ["settings", "gaussians", "radii", "colors2", *_STATE, *_POSE, "inst_records",
                                        *_FWD_TAIL],
    "gsr_mark_visible": ["P", "means3D", "viewmatrix", "projmatrix", "visible", "stream"],
}


def call(fn, **over):
    """fn(defaults, overridden by name).  A struct argument takes None (NULL) or a dict of field overrides."""
    unknown = set(over) - set(PARAMS[fn])
    assert not unknown, (fn, unknown)
    keep, args = [], []
    for name in PARAMS[fn]:
        if name in STRUCTS:
            cls, base = STRUCTS[name]
            v = over.get(name, {} if base is not None else None)
            if v is not None:
                keep.append(cls(**{**(base or {}), **v}))
                v = ctypes.byref(keep[-1])
        else:
            v = over.get(name, DEFAULTS[name])
        args.append(v)
    rc = getattr(lib, fn)(*args)
    return rc, lib.gsr_last_error().decode()


def test_parameter_lists_match_the_ctypes_table():
    for fn, names in PARAMS.items():
        assert len(names) == len(SIGNATURES[fn][1]), fn


def test_defaults_pass_the_host_checks_of_an_empty_map():
    """The defaults themselves are not what the rows' refusals come from: with P = 0 the backward entries
    accept them and return before any device work (gsr_backward: 'if (P == 0) return GSR_OK')."""
    empty = dict(gaussians=dict(P=0))
    for fn in ("gsr_backward", "gsr_backward_dual", "gsr_track_backward_dual", "gsr_track_backward_dual_records"):
        assert call(fn, **empty)[0] == OK, fn
    assert call("gsr_backward_dual_sh_adam", gaussians=dict(P=0, shs=D, M=1))[0] == OK
    assert call("gsr_mark_visible", P=0)[0] == OK


M_NULL = "null settings or gaussians"
M_P = "P must be >= 0"
M_BINNING = "settings.binning must be GSR_BINNING_CULLED or GSR_BINNING_REFERENCE"
M_SIZE = "image size must be positive"
M_LARGE = "image too large for 16-bit tile coordinates"
M_MEANS = "means3D is required"
M_OPAC = "opacities are required"
M_CAM = "camera matrices / bg missing"
M_COLOURS = "Please provide excatly one of either SHs or precomputed colors!"
M_CAMPOS = "campos required for SH colours"
M_DEGREE = "sh_degree must be in [0,3] with (deg+1)^2 <= M"
M_COV = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
M_ALLOC = "allocator callback required"
M_OUT = "output image pointers required"
M_OUT2 = "out_color2 required with colors2"
M_C2 = "colors2 required"
M_STATIC = "static mode needs capacity > 0 and status"
M_ALIVE = "alive mask required"
M_TRACK_NULL = "track_forward_dual_static: null pointer"
M_TXF = "track_forward_dual_static_xf: "
M_MXF = "forward_dual_static_xf: "
M_XF_COLOURS = "precomputed colours, scales / rotations only"
M_FB_RECORDS = "track_forward_backward_dual_static_xf: null records"
M_REUSE_SH = "geometry reuse needs precomputed colours (no SH)"
M_REUSE_STATE = "geometry reuse needs the previous call's state and the outputs"
M_IFEQ_COLOURS = "geometry reuse needs precomputed colours (no SH, no cov3D)"
M_IFEQ_PAIRS = "gsr_forward_reuse_if_equal: 1..8 pairs and `reused`"
M_IFEQ_STATE = "geometry reuse needs the previous call's state"
M_IFEQ_PAIR = "gsr_forward_reuse_if_equal: pair"
M_EQ = "gsr_bitwise_equal: 0..8 pairs and a flag"
M_EQ_PAIR = "gsr_bitwise_equal: pair"
M_DL2 = "dl2_channels must be 1 or 3"
M_DUAL_BWD = "dual backward needs dL_dout_color2"
M_GRADS = "grads required"
M_NR = "num_rendered must be >= 0"
M_SH_ADAM_ENTRY = "backward_dual_sh_adam: SH colours and the colour group's state required"
M_SH_ADAM = "sh_adam needs staged SH colours (M == (D+1)^2) and power 1"
M_STATE = "missing forward state"
M_TB_SIZES = "track_backward_dual: bad sizes"
M_TB_NULL = "track_backward_dual: null pointer"
M_TB_ANISO = "track_backward_dual: anisotropic maps need the rendered rotations"
M_TB_RECORDS = "track_backward_dual_records: null records"

SH = dict(shs=D, M=16, colors_precomp=None)
ROWS = []


def row(label, fn, msg, **over):
    ROWS.append(pytest.param(fn, over, msg, id=f"{fn}-{label}"))


# ---- every refusal of validate(), through gsr_forward and gsr_backward ----
for _fn in ("gsr_forward", "gsr_backward"):
    row("settings_null", _fn, M_NULL, settings=None)
    row("gaussians_null", _fn, M_NULL, gaussians=None)
    row("P_negative", _fn, M_P, gaussians=dict(P=-1))
    row("binning", _fn, M_BINNING, settings=dict(binning=2))
    row("width_zero", _fn, M_SIZE, settings=dict(image_width=0))
    row("height_negative", _fn, M_SIZE, settings=dict(image_height=-3))
    row("width_large", _fn, M_LARGE, settings=dict(image_width=16 * 65535 + 1))
    row("height_large", _fn, M_LARGE, settings=dict(image_height=16 * 65535 + 1))
    row("means3D", _fn, M_MEANS, gaussians=dict(means3D=None))
    row("viewmatrix", _fn, M_CAM, settings=dict(viewmatrix=None))
    row("projmatrix", _fn, M_CAM, settings=dict(projmatrix=None))
    row("bg", _fn, M_CAM, settings=dict(bg=None))
    row("no_colours", _fn, M_COLOURS, gaussians=dict(colors_precomp=None))
    row("shs_without_M", _fn, M_COLOURS, gaussians=dict(colors_precomp=None, shs=D, M=0))
    row("campos", _fn, M_CAMPOS, gaussians=SH, settings=dict(campos=None))
    row("degree_negative", _fn, M_DEGREE, gaussians=SH, settings=dict(sh_degree=-1))
    row("degree_4", _fn, M_DEGREE, gaussians=SH, settings=dict(sh_degree=4))
    row("degree_over_M", _fn, M_DEGREE, gaussians=dict(shs=D, M=3, colors_precomp=None), settings=dict(sh_degree=1))
    row("no_scales", _fn, M_COV, gaussians=dict(scales=None))
    row("no_rotations", _fn, M_COV, gaussians=dict(rotations=None))
row("opacities", "gsr_forward", M_OPAC, gaussians=dict(opacities=None))

# ---- gsr_forward / gsr_forward_dual: allocator and output pointers ----
row("alloc", "gsr_forward", M_ALLOC, alloc=NO_ALLOC)
row("alloc_empty_map", "gsr_forward", M_ALLOC, alloc=NO_ALLOC, gaussians=dict(P=0))
row("out_color", "gsr_forward", M_OUT, out_color=None)
row("out_depth", "gsr_forward", M_OUT, out_depth=None)
row("colors2", "gsr_forward_dual", M_C2, colors2=None)
row("alloc", "gsr_forward_dual", M_ALLOC, alloc=NO_ALLOC)
row("out_color", "gsr_forward_dual", M_OUT, out_color=None)
row("out_color2", "gsr_forward_dual", M_OUT2, out_color2=None)
row("validate", "gsr_forward_dual", M_OPAC, gaussians=dict(opacities=None))

# ---- the three static forwards ----
for _fn in ("gsr_forward_static", "gsr_forward_dual_static", "gsr_forward_dual_static_alive"):
    row("capacity_zero", _fn, M_STATIC, capacity=0)
    row("capacity_negative", _fn, M_STATIC, capacity=-5)
    row("status", _fn, M_STATIC, status=None)
    row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
    row("validate", _fn, M_SIZE, settings=dict(image_width=0))
row("colors2", "gsr_forward_dual_static", M_C2, colors2=None)
row("colors2", "gsr_forward_dual_static_alive", M_C2, colors2=None)
row("alive", "gsr_forward_dual_static_alive", M_ALIVE, alive=None)
row("alive_gaussians_null", "gsr_forward_dual_static_alive", M_NULL, alive=None, gaussians=None)
row("out_color2", "gsr_forward_dual_static", M_OUT2, out_color2=None)

# ---- gsr_track_forward_dual_static ----
row("colors2", "gsr_track_forward_dual_static", M_C2, colors2=None)
row("capacity", "gsr_track_forward_dual_static", M_STATIC, capacity=0)
row("status", "gsr_track_forward_dual_static", M_STATIC, status=None)
for _p in ("gt_im", "gt_depth", "dL_dloss", "loss", "dL_dim", "dL_ddepth_sil", "scratch"):
    row(_p, "gsr_track_forward_dual_static", M_TRACK_NULL, **{_p: None})
row("validate", "gsr_track_forward_dual_static", M_BINNING, settings=dict(binning=7))
row("alloc", "gsr_track_forward_dual_static", M_ALLOC, alloc=NO_ALLOC)
row("out_depth", "gsr_track_forward_dual_static", M_OUT, out_depth=None)

# ---- the tracking _xf forward (and the fused forward + backward over it) ----
_XF_PTRS = ("means_world", "unnorm_rot", "logit_opac", "log_scales", "cam_q", "cam_t", "w2c")
_G_PTRS = ("means3D", "rotations", "opacities", "scales")
for _fn in ("gsr_track_forward_dual_static_xf", "gsr_track_forward_backward_dual_static_xf"):
    row("xform_null", _fn, M_TXF + "null pointer", xform=None)
    row("gaussians_null", _fn, M_TXF + "null pointer", gaussians=None)
    row("scale_cols", _fn, M_TXF + "bad sizes", xform=dict(scale_cols=2))
    row("q_stride", _fn, M_TXF + "bad sizes", xform=dict(q_stride=0))
    for _p in _XF_PTRS:
        row(_p, _fn, M_TXF + "null pointer", xform={_p: None})
    for _p in _G_PTRS:
        row("g_" + _p, _fn, M_TXF + "null pointer", gaussians={_p: None})
    row("colors2", _fn, M_TXF + "null pointer", colors2=None)
    row("colors2_empty_map", _fn, M_C2, colors2=None, gaussians=dict(P=0))
    row("shs", _fn, M_TXF + M_XF_COLOURS, gaussians=dict(shs=D, M=16))
    row("cov3D", _fn, M_TXF + M_XF_COLOURS, gaussians=dict(cov3D_precomp=D))
    row("capacity", _fn, M_STATIC, capacity=0)
    row("status", _fn, M_STATIC, status=None)
    for _p in ("gt_im", "gt_depth", "dL_dloss", "loss", "scratch"):
        row(_p, _fn, M_TXF + "null pointer", **{_p: None})
    row("validate", _fn, M_COLOURS, gaussians=dict(colors_precomp=None))
    row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
row("dL_dim", "gsr_track_forward_dual_static_xf", M_TXF + "null pointer", dL_dim=None)
row("dL_ddepth_sil", "gsr_track_forward_dual_static_xf", M_TXF + "null pointer", dL_ddepth_sil=None)
row("out_color", "gsr_track_forward_dual_static_xf", M_OUT, out_color=None)
row("records", "gsr_track_forward_backward_dual_static_xf", M_FB_RECORDS, inst_records=None)
# (all three images NULL is the fused call's "store nothing" form; one or two NULL is refused)
row("out_depth_only", "gsr_track_forward_backward_dual_static_xf", M_OUT, out_depth=None)
row("out_color2_only", "gsr_track_forward_backward_dual_static_xf", M_OUT2, out_color2=None)
row("fused forward, validate fails", "gsr_track_forward_backward_dual_static_xf", M_SIZE,
    settings=dict(image_height=0), out_color=None, out_color2=None, out_depth=None)

# ---- the mapping _xf forward ----
_fn = "gsr_forward_dual_static_xf"
row("xform_null", _fn, M_MXF + "null pointer", xform=None)
row("gaussians_null", _fn, M_MXF + "null pointer", gaussians=None)
row("scale_cols", _fn, M_MXF + "bad sizes", xform=dict(scale_cols=0))
row("q_stride", _fn, M_MXF + "bad sizes", xform=dict(q_stride=-1))
row("store_rendervars", _fn, M_MXF + "store_rendervars must be 1", xform=dict(store_rendervars=0))
row("shs", _fn, M_MXF + M_XF_COLOURS, gaussians=dict(shs=D, M=16))
row("cov3D", _fn, M_MXF + M_XF_COLOURS, gaussians=dict(cov3D_precomp=D))
for _p in _XF_PTRS:
    row(_p, _fn, M_MXF + "null pointer", xform={_p: None})
for _p in _G_PTRS + ("colors_precomp",):
    row("g_" + _p, _fn, M_MXF + "null pointer", gaussians={_p: None})
row("colors2", _fn, M_C2, colors2=None)
row("capacity", _fn, M_STATIC, capacity=0)
row("status", _fn, M_STATIC, status=None)
row("validate", _fn, M_CAM, settings=dict(bg=None))
row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
row("out_color2", _fn, M_OUT2, out_color2=None)

# ---- gsr_forward_reuse ----
_fn = "gsr_forward_reuse"
row("validate", _fn, M_NULL, settings=None)
row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
row("sh_colours", _fn, M_REUSE_SH, gaussians=SH)
row("sh_and_colours", _fn, M_REUSE_SH, gaussians=dict(shs=D, M=16))
row("empty_map", _fn, M_REUSE_STATE, gaussians=dict(P=0))
row("num_rendered", _fn, M_REUSE_STATE, num_rendered=-1)
for _p in ("prev_geom", "binning_buffer", "image_buffer", "prev_radii", "out_color", "out_depth", "radii"):
    row(_p, _fn, M_REUSE_STATE, **{_p: None})

# ---- gsr_forward_reuse_if_equal: its four messages, then the forward's ----
_fn = "gsr_forward_reuse_if_equal"
row("gaussians_null", _fn, M_IFEQ_COLOURS, gaussians=None)
row("no_colours", _fn, M_IFEQ_COLOURS, gaussians=dict(colors_precomp=None))
row("shs", _fn, M_IFEQ_COLOURS, gaussians=dict(shs=D, M=16))
row("cov3D", _fn, M_IFEQ_COLOURS, gaussians=dict(cov3D_precomp=D))
row("npairs_zero", _fn, M_IFEQ_PAIRS, npairs=0)
row("npairs_nine", _fn, M_IFEQ_PAIRS, npairs=9)
for _p in ("a", "b", "n", "reused"):
    row(_p, _fn, M_IFEQ_PAIRS, **{_p: None})
row("prev_num_rendered", _fn, M_IFEQ_STATE, prev_num_rendered=-1)
for _p in ("prev_geom", "prev_binning", "prev_image", "prev_radii"):
    row(_p, _fn, M_IFEQ_STATE, **{_p: None})
row("pair_negative", _fn, M_IFEQ_PAIR, n=_NEG8)
row("pair_a_null", _fn, M_IFEQ_PAIR, a=_NULLS8)
row("pair_b_null", _fn, M_IFEQ_PAIR, b=_NULLS8)
row("validate", _fn, M_NULL, settings=None)
row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
row("out_depth", _fn, M_OUT, out_depth=None)

# ---- gsr_bitwise_equal ----
_fn = "gsr_bitwise_equal"
row("npairs_negative", _fn, M_EQ, npairs=-1)
row("npairs_nine", _fn, M_EQ, npairs=9)
for _p in ("a", "b", "n", "flag"):
    row(_p, _fn, M_EQ, **{_p: None})
row("flag_no_pairs", _fn, M_EQ, npairs=0, flag=None)
row("pair_negative", _fn, M_EQ_PAIR, n=_NEG8)
row("pair_a_null", _fn, M_EQ_PAIR, a=_NULLS8)
row("pair_b_null", _fn, M_EQ_PAIR, b=_NULLS8)

# ---- the backward's own refusals ----
row("dl2_channels", "gsr_backward_dual", M_DL2, dl2_channels=2)
row("dl2_channels_zero", "gsr_backward_dual_sh_adam", M_DL2, dl2_channels=0, gaussians=dict(shs=D, M=1))
row("colors2", "gsr_backward_dual", M_C2, colors2=None)
row("dL_dout_color2", "gsr_backward_dual", M_DUAL_BWD, dL_dout_color2=None)
row("dL_dout_color2", "gsr_track_backward_dual", M_DUAL_BWD, dL_dout_color2=None)
for _fn in ("gsr_backward", "gsr_backward_dual"):
    row("grads", _fn, M_GRADS, grads=None)
    row("num_rendered", _fn, M_NR, num_rendered=-1)
    for _p in ("geom_buffer", "image_buffer", "radii", "dL_dout_color"):
        row(_p, _fn, M_STATE, **{_p: None})
row("colors2", "gsr_backward_dual_sh_adam", M_C2, colors2=None)
row("sh_adam_null", "gsr_backward_dual_sh_adam", M_SH_ADAM_ENTRY, sh_adam=None, gaussians=dict(shs=D, M=1))
row("gaussians_null", "gsr_backward_dual_sh_adam", M_SH_ADAM_ENTRY, gaussians=None)
row("no_shs", "gsr_backward_dual_sh_adam", M_SH_ADAM_ENTRY)
row("step", "gsr_backward_dual_sh_adam", M_SH_ADAM_ENTRY, sh_adam=dict(step=0), gaussians=dict(shs=D, M=1))
row("exp_avg", "gsr_backward_dual_sh_adam", M_SH_ADAM_ENTRY, gaussians=dict(shs=D, M=1),
    sh_adam=dict(exp_avg=(ctypes.c_void_p * 5)(D, D, D, D, None)))
row("exp_avg_sq", "gsr_backward_dual_sh_adam", M_SH_ADAM_ENTRY, gaussians=dict(shs=D, M=1),
    sh_adam=dict(exp_avg_sq=(ctypes.c_void_p * 5)(D, D, D, D, None)))
row("not_staged", "gsr_backward_dual_sh_adam", M_SH_ADAM, gaussians=dict(shs=D, M=16))
row("state", "gsr_backward_dual_sh_adam", M_STATE, gaussians=dict(shs=D, M=1), image_buffer=None)

# ---- track_backward's three messages, through both public entries ----
for _fn in ("gsr_track_backward_dual", "gsr_track_backward_dual_records"):
    row("gaussians_null", _fn, M_TB_SIZES, gaussians=None)
    row("scale_cols", _fn, M_TB_SIZES, scale_cols=2)
    row("q_stride", _fn, M_TB_SIZES, q_stride=0)
    for _p in ("colors2", "means_world", "unnorm_rot", "cam_q", "cam_t", "w2c", "scratch"):
        row(_p, _fn, M_TB_NULL, **{_p: None})
    row("no_adam_no_dq", _fn, M_TB_NULL, adam_state=None, dL_dcam_q=None)
    row("no_adam_no_dt", _fn, M_TB_NULL, adam_state=None, dL_dcam_t=None)
    row("anisotropic", _fn, M_TB_ANISO, scale_cols=3, gaussians=dict(rotations=None, cov3D_precomp=D))
    row("validate", _fn, M_SIZE, settings=dict(image_width=-1))
    row("num_rendered", _fn, M_NR, num_rendered=-2)
    row("geom_buffer", _fn, M_STATE, geom_buffer=None)
row("records", "gsr_track_backward_dual_records", M_TB_RECORDS, inst_records=None)
row("dL_dout_color", "gsr_track_backward_dual", M_STATE, dL_dout_color=None)

# ---- gsr_mark_visible ----
row("P_negative", "gsr_mark_visible", M_P, P=-1)
for _p in ("means3D", "viewmatrix", "visible"):
    row(_p, "gsr_mark_visible", "null pointer", **{_p: None})

# ---- two defects at once: the message that wins ----
# validate's code is returned only after dl2_channels has been reported
row("2: dl2_channels over validate", "gsr_backward_dual", M_DL2, dl2_channels=2, settings=None)
row("2: dl2_channels over P", "gsr_backward_dual", M_DL2, dl2_channels=4, gaussians=dict(P=-1))
row("2: validate over dual", "gsr_backward_dual", M_MEANS, gaussians=dict(means3D=None), dL_dout_color2=None)
row("2: dual over grads", "gsr_backward_dual", M_DUAL_BWD, dL_dout_color2=None, grads=None)
row("2: grads over num_rendered", "gsr_backward", M_GRADS, grads=None, num_rendered=-1)
row("2: num_rendered over state", "gsr_backward", M_NR, num_rendered=-1, geom_buffer=None)
row("2: sh_adam over state", "gsr_backward_dual_sh_adam", M_SH_ADAM, gaussians=dict(shs=D, M=16), geom_buffer=None)
row("2: colors2 over sh_adam", "gsr_backward_dual_sh_adam", M_C2, colors2=None, sh_adam=None)
row("2: validate over alloc", "gsr_forward", M_P, gaussians=dict(P=-1), alloc=NO_ALLOC)
row("2: alloc over outputs", "gsr_forward", M_ALLOC, alloc=NO_ALLOC, out_color=None)
row("2: out_color over out_color2", "gsr_forward_dual", M_OUT, out_color=None, out_color2=None)
row("2: colors2 over capacity", "gsr_forward_dual_static", M_C2, colors2=None, capacity=0)
row("2: capacity over alive", "gsr_forward_dual_static_alive", M_STATIC, capacity=0, alive=None)
row("2: alive over validate", "gsr_forward_dual_static_alive", M_ALIVE, alive=None, settings=None)
row("2: colors2 over null pointer", "gsr_track_forward_dual_static", M_C2, colors2=None, gt_im=None)
row("2: capacity over null pointer", "gsr_track_forward_dual_static", M_STATIC, status=None, loss=None)
# the two _xf forwards check SH colours and the null pointers in opposite orders
row("2: null pointer over shs", "gsr_track_forward_dual_static_xf", M_TXF + "null pointer",
    gaussians=dict(shs=D, M=16), xform=dict(means_world=None))
row("2: shs over null pointer", "gsr_forward_dual_static_xf", M_MXF + M_XF_COLOURS, gaussians=dict(shs=D, M=16),
    xform=dict(means_world=None))
row("2: sizes over shs", "gsr_track_forward_dual_static_xf", M_TXF + "bad sizes", gaussians=dict(shs=D, M=16),
    xform=dict(scale_cols=2))
row("2: store over shs", "gsr_forward_dual_static_xf", M_MXF + "store_rendervars must be 1",
    gaussians=dict(shs=D, M=16), xform=dict(store_rendervars=0))
row("2: shs over capacity", "gsr_track_forward_dual_static_xf", M_TXF + M_XF_COLOURS, gaussians=dict(cov3D_precomp=D),
    capacity=0)
row("2: records over xform", "gsr_track_forward_backward_dual_static_xf", M_FB_RECORDS, inst_records=None,
    xform=None)
row("2: xf checks over validate", "gsr_track_forward_dual_static_xf", M_STATIC, capacity=0, settings=None)
row("2: sizes over null pointer", "gsr_track_backward_dual", M_TB_SIZES, scale_cols=2, colors2=None)
row("2: null pointer over anisotropic", "gsr_track_backward_dual", M_TB_NULL, scale_cols=3, w2c=None,
    gaussians=dict(rotations=None, cov3D_precomp=D))
row("2: records over sizes", "gsr_track_backward_dual_records", M_TB_RECORDS, inst_records=None, q_stride=0)
row("2: colours over pairs", "gsr_forward_reuse_if_equal", M_IFEQ_COLOURS, gaussians=dict(colors_precomp=None),
    npairs=0)
row("2: pairs over state", "gsr_forward_reuse_if_equal", M_IFEQ_PAIRS, npairs=0, prev_geom=None)
row("2: state over pair", "gsr_forward_reuse_if_equal", M_IFEQ_STATE, prev_image=None, n=_NEG8)
row("2: pair over validate", "gsr_forward_reuse_if_equal", M_IFEQ_PAIR, n=_NEG8, settings=None)
row("2: validate over alloc", "gsr_forward_reuse", M_SIZE, settings=dict(image_width=0), alloc=NO_ALLOC)
row("2: alloc over colours", "gsr_forward_reuse", M_ALLOC, alloc=NO_ALLOC, gaussians=dict(shs=D, M=16))
row("2: colours over state", "gsr_forward_reuse", M_REUSE_SH, gaussians=dict(shs=D, M=16), prev_geom=None)
row("2: pairs over pair", "gsr_bitwise_equal", M_EQ, flag=None, n=_NEG8)
row("2: P over null pointer", "gsr_mark_visible", M_P, P=-1, means3D=None)


@pytest.mark.parametrize("fn,over,msg", ROWS)
def test_refusal(fn, over, msg):
    rc, got = call(fn, **over)
    assert (rc, got) == (INVALID, msg)
