"""use_depth_loss_thres (scripts/splatam.py:464-466, :745-758) without a device: the _terms entry points' exports,
table rows and host-side refusals, the rule that decides whether a frame tracks once more (splatam_amd.tracker.run_frame,
driven by a stub tracker), and the configuration defaults."""
import ctypes
import math

import pytest
import torch

from test_abi_cpu import header_functions, header_struct_fields
from test_capi_refusals_cpu import (_FWD_TAIL, _L1, _XF_HEAD, DEFAULTS, INVALID, NO_ALLOC, PARAMS, STRUCTS, D,
                                    M_ALLOC, M_C2, M_FB_RECORDS, M_OUT, M_SIZE, M_STATIC, M_TRACK_NULL, M_TXF)

from splatam_amd import _lib
from splatam_amd._lib import SIGNATURES, lib

_L1_ALONE = ["H", "W", "im", "depth_sil", "gt_im", "gt_depth", "sil_thres", "w_im", "w_depth"]
# each _terms entry: its sibling's parameters with `terms` behind `loss`
TERMS_PARAMS = {
    "gsr_track_l1_fwd_terms": [*_L1_ALONE, "loss", "terms", "scratch", "stream"],
    "gsr_track_l1_fwd_bwd_terms": [*_L1_ALONE, "dL_dloss", "loss", "terms", "dL_dim", "dL_ddepth_sil", "scratch",
                                   "stream"],
    "gsr_track_forward_dual_static_terms": ["settings", "gaussians", "colors2", "capacity", "status", "out_color",
                                            "out_color2", "out_depth", "radii", *_L1, "terms", "dL_dim",
                                            "dL_ddepth_sil", "scratch", *_FWD_TAIL],
    "gsr_track_forward_dual_static_xf_terms": [*_XF_HEAD, *_L1, "terms", "dL_dim", "dL_ddepth_sil", "scratch",
                                               *_FWD_TAIL],
    "gsr_track_forward_backward_dual_static_xf_terms": [*_XF_HEAD, *_L1, "terms", "scratch", "inst_records",
                                                        *_FWD_TAIL],
}
SIBLING = {fn: fn[:-len("_terms")] for fn in TERMS_PARAMS}
TERMS_DEFAULTS = dict(DEFAULTS, H=32, W=48, im=D, depth_sil=D, terms=D)


def call(fn, **over):
    """test_capi_refusals_cpu.call over the new entries' parameter lists."""
    unknown = set(over) - set(TERMS_PARAMS[fn])
    assert not unknown, (fn, unknown)
    keep, args = [], []
    for name in TERMS_PARAMS[fn]:
        if name in STRUCTS:
            cls, base = STRUCTS[name]
            v = over.get(name, {} if base is not None else None)
            if v is not None:
                keep.append(cls(**{**(base or {}), **v}))
                v = ctypes.byref(keep[-1])
        else:
            v = over.get(name, TERMS_DEFAULTS[name])
        args.append(v)
    rc = getattr(lib, fn)(*args)
    return rc, lib.gsr_last_error().decode()


# ---------------------------------------------------------------- exports --
def test_terms_entries_are_declared_exported_and_in_the_table():
    declared = header_functions()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn, names in TERMS_PARAMS.items():
        assert fn in declared, fn
        assert hasattr(raw, fn), fn
        assert fn in SIGNATURES, fn
        res, args = SIGNATURES[fn]
        assert res is ctypes.c_int and len(args) == len(names), fn
        # the sibling's row with one more pointer, where `terms` stands
        sres, sargs = SIGNATURES[SIBLING[fn]]
        k = names.index("terms")
        assert names[k - 1] == "loss"
        assert args[:k] == sargs[:k] and args[k] is ctypes.c_void_p and args[k + 1:] == sargs[k:], fn
    # the siblings keep their lists (no existing signature changed)
    for fn in ("gsr_track_forward_dual_static", "gsr_track_forward_dual_static_xf",
               "gsr_track_forward_backward_dual_static_xf"):
        assert [n for n in TERMS_PARAMS[fn + "_terms"] if n != "terms"] == PARAMS[fn]
    assert lib.gsr_abi_version() == 8


def test_pinned_structs_are_unchanged():
    want = {
        "gsr_settings": ["image_height", "image_width", "tan_fovx", "tan_fovy", "bg", "scale_modifier", "viewmatrix",
                         "projmatrix", "sh_degree", "campos", "prefiltered", "binning"],
        "gsr_gaussians": ["P", "M", "means3D", "shs", "colors_precomp", "opacities", "scales", "rotations",
                          "cov3D_precomp"],
        "gsr_grads": ["dmeans2D", "dcolors", "dopacity", "dmeans3D", "dcov3D", "dsh", "dscales", "drotations"],
        "gsr_track_xform": ["means_world", "unnorm_rot", "logit_opac", "log_scales", "scale_cols", "cam_q", "cam_t",
                            "q_stride", "w2c", "store_rendervars", "alive"],
        "gsr_pose_track": ["status", "capacity", "loss", "best"],
        "gsr_map_adam": ["exp_avg", "exp_avg_sq", "lr", "step", "beta1", "beta2", "eps", "status", "capacity",
                         "halted"],
    }
    for name, fields in want.items():
        assert header_struct_fields(name) == fields, name


# -------------------------------------------------------------- refusals --
ROWS = []


def row(label, fn, msg, **over):
    ROWS.append(pytest.param(fn, over, msg, id=f"{fn}-{label}"))


for _fn in TERMS_PARAMS:
    _name = _fn[len("gsr_"):]
    row("terms_null", _fn, _name + ": null terms", terms=None)
    row("terms_misaligned", _fn, _name + ": terms must be 4-byte aligned", terms=D + 2)
    row("terms_misaligned_1", _fn, _name + ": terms must be 4-byte aligned", terms=D + 1)
# the siblings' own checks follow, under the siblings' names
for _fn, _m in (("gsr_track_l1_fwd_terms", "track_l1_fwd"), ("gsr_track_l1_fwd_bwd_terms", "track_l1_fwd_bwd")):
    row("H_zero", _fn, _m + ": bad image size", H=0)
    row("W_negative", _fn, _m + ": bad image size", W=-1)
    for _p in ("im", "depth_sil", "gt_im", "gt_depth", "loss", "scratch"):
        row(_p, _fn, _m + ": null pointer", **{_p: None})
    row("2: terms over size", _fn, _fn[len("gsr_"):] + ": null terms", terms=None, H=0)
for _p in ("dL_dloss", "dL_dim", "dL_ddepth_sil"):
    row(_p, "gsr_track_l1_fwd_bwd_terms", "track_l1_fwd_bwd: null pointer", **{_p: None})
_fn = "gsr_track_forward_dual_static_terms"
row("colors2", _fn, M_C2, colors2=None)
row("capacity", _fn, M_STATIC, capacity=0)
row("status", _fn, M_STATIC, status=None)
for _p in ("gt_im", "gt_depth", "dL_dloss", "loss", "dL_dim", "dL_ddepth_sil", "scratch"):
    row(_p, _fn, M_TRACK_NULL, **{_p: None})
row("validate", _fn, M_SIZE, settings=dict(image_width=0))
row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
row("out_depth", _fn, M_OUT, out_depth=None)
row("2: terms over colors2", _fn, "track_forward_dual_static_terms: null terms", terms=None, colors2=None)
for _fn in ("gsr_track_forward_dual_static_xf_terms", "gsr_track_forward_backward_dual_static_xf_terms"):
    row("xform_null", _fn, M_TXF + "null pointer", xform=None)
    row("scale_cols", _fn, M_TXF + "bad sizes", xform=dict(scale_cols=2))
    row("means_world", _fn, M_TXF + "null pointer", xform=dict(means_world=None))
    row("capacity", _fn, M_STATIC, capacity=0)
    for _p in ("gt_im", "gt_depth", "dL_dloss", "loss", "scratch"):
        row(_p, _fn, M_TXF + "null pointer", **{_p: None})
    row("alloc", _fn, M_ALLOC, alloc=NO_ALLOC)
row("dL_dim", "gsr_track_forward_dual_static_xf_terms", M_TXF + "null pointer", dL_dim=None)
row("records", "gsr_track_forward_backward_dual_static_xf_terms", M_FB_RECORDS, inst_records=None)
row("2: terms over records", "gsr_track_forward_backward_dual_static_xf_terms",
    "track_forward_backward_dual_static_xf_terms: null terms", terms=None, inst_records=None)


@pytest.mark.parametrize("fn,over,msg", ROWS)
def test_terms_refusal(fn, over, msg):
    rc, got = call(fn, **over)
    assert (rc, got) == (INVALID, msg)


def test_terms_tensor_is_checked_before_the_call():
    from splatam_amd._C import terms_ptr
    cpu = torch.device("cpu")
    assert terms_ptr(torch.zeros(2), cpu) != 0
    for bad in (torch.zeros(3), torch.zeros(2, dtype=torch.float64), torch.zeros(4)[::2], None):
        with pytest.raises(RuntimeError, match="terms"):
            terms_ptr(bad, cpu)
    with pytest.raises(RuntimeError, match="terms"):
        terms_ptr(torch.zeros(2), torch.device("cuda", 0))  # another device than the forward's


# ------------------------------------------------------ the decision rule --
class _Unreadable:
    def __getitem__(self, key):
        raise AssertionError("terms read without a threshold")


class StubTracker:
    """What run_frame drives: `iters` iterations per run(); `terms` as the last replay left them."""

    def __init__(self, iters, depth, readable=True):
        self.iters, self.log = iters, []
        self.terms = torch.zeros(iters, 2) if readable else _Unreadable()
        if readable:
            self.terms[:, 1] = -1.0     # only the last row's depth term may decide
            self.terms[:, 0] = 1e30     # ... and never the image term
            self.terms[iters - 1, 1] = depth

    def begin_frame(self):
        self.log.append("begin")

    def run(self):
        self.log.append("run")

    def end_frame(self):
        self.log.append("end")


N, S, THRES = 8, 4, 2.5


@pytest.mark.parametrize("depth,thres,total", [
    # depth < thres (down to the float32 just below it): the frame ends
    (2.0, THRES, N), (float(torch.nextafter(torch.tensor(THRES), torch.tensor(0.0))), THRES, N),
    (THRES, THRES, 2 * N),                                    # equal is not below
    (3.0, THRES, 2 * N), (float("inf"), THRES, 2 * N),
    (float("nan"), THRES, 2 * N),                             # a NaN is not below
    (0.0, 0.0, 2 * N),                                        # threshold 0 always extends
    (1e30, float("inf"), N),                                  # ... and +inf never
    (2.0, None, N),
])
def test_decision_rule(depth, thres, total):
    from splatam_amd.tracker import run_frame
    tr = StubTracker(S, depth)
    assert run_frame(tr, N, thres) == total
    # begin once, the replays, end exactly once and after the last replay; never a third batch
    assert tr.log == ["begin"] + ["run"] * (total // S) + ["end"]
    assert total <= 2 * N


def test_no_threshold_never_reads_terms():
    from splatam_amd.tracker import run_frame
    tr = StubTracker(S, 0.0, readable=False)
    assert run_frame(tr, N) == N
    assert tr.log == ["begin", "run", "run", "end"]
    with pytest.raises(AssertionError, match="terms read"):
        run_frame(StubTracker(S, 0.0, readable=False), N, THRES)


def test_threshold_compares_in_float32_as_published():
    """The term is the float32 the kernel wrote: a threshold between that float and the next double above it
    sees it below."""
    from splatam_amd.tracker import run_frame
    x = float(torch.tensor(0.1, dtype=torch.float32))
    assert run_frame(StubTracker(S, 0.1), N, math.nextafter(x, 1.0)) == N
    assert run_frame(StubTracker(S, 0.1), N, x) == 2 * N


# -------------------------------------------------------------- defaults --
def test_config_defaults_are_the_reference():
    from splatam_amd.slam import TrackingConfig
    cfg = TrackingConfig()
    assert cfg.use_depth_loss_thres is False and cfg.depth_loss_thres == 100000.0  # scripts/splatam.py:464-466
    assert isinstance(cfg.depth_loss_thres, float)


def test_track_frame_signature():
    import inspect

    from splatam_amd.tracker import GraphTracker
    sig = inspect.signature(GraphTracker.track_frame)
    assert list(sig.parameters) == ["self", "num_iters", "check", "depth_loss_thres"]
    assert sig.parameters["check"].default is True and sig.parameters["depth_loss_thres"].default is None
    assert inspect.signature(GraphTracker.__init__).parameters["loss_terms"].default is False
