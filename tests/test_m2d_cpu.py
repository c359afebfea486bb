"""The RGB render's own means2D gradient from the dual backward, and the densification statistics kernel: what
needs no device.  The header declares gsr_backward_dual_m2d and gsr_accumulate_mean2d, the library exports
them and the ctypes table carries their argument lists; the sibling's refusals come back before the first HIP
call (the style of tests/test_capi_refusals_cpu.py, whose defaults and `call` this reuses);
surgery.densify(accumulate=False) after accumulating by hand equals today's path; the two means2D keywords of
rasterize_gaussians_dual exclude each other."""
import copy
import ctypes
import os
import re

import pytest
import torch

import test_capi_refusals_cpu as rc
from splatam_amd import _lib, rasterizer, surgery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, OK = -1, 0
M2D = "gsr_backward_dual_m2d"
M2D_PARAMS = [*rc._DUAL_BWD, "dmeans2D_color1", *rc._FWD_TAIL]


def _declaration(header, name):
    txt = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, re.S)
    assert m, f"{header} does not declare {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_new_symbols():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for header, name in (("gsr.h", M2D), ("gsr_glue.h", "gsr_accumulate_mean2d")):
        args = _declaration(header, name)
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(args), (name, args)
    base, m2d = _declaration("gsr.h", "gsr_backward_dual"), _declaration("gsr.h", M2D)
    # the sibling: gsr_backward_dual's arguments with dmeans2D_color1 behind dl2_channels
    assert m2d == base[:13] + ["float* dmeans2D_color1"] + base[13:]
    assert _lib.SIGNATURES[M2D][1] == (_lib.SIGNATURES["gsr_backward_dual"][1][:13] + [ctypes.c_void_p] +
                                       _lib.SIGNATURES["gsr_backward_dual"][1][13:])
    assert len(M2D_PARAMS) == len(_lib.SIGNATURES[M2D][1])
    acc = _declaration("gsr_glue.h", "gsr_accumulate_mean2d")
    assert [a.split()[-1].lstrip("*") for a in acc] == ["P", "radii", "dmeans2D", "accum", "denom", "max_2D_radius",
                                                        "stream"]


@pytest.fixture()
def m2d_call(monkeypatch):
    monkeypatch.setitem(rc.PARAMS, M2D, M2D_PARAMS)
    monkeypatch.setitem(rc.DEFAULTS, "dmeans2D_color1", rc.D)
    monkeypatch.setitem(rc.DEFAULTS, "dl2_channels", 1)
    return lambda **over: rc.call(M2D, **over)


def test_m2d_sibling_refusals_need_no_device(m2d_call):
    assert m2d_call(gaussians=dict(P=0)) == (OK, rc.lib.gsr_last_error().decode())  # the defaults themselves pass
    rows = [
        (dict(dmeans2D_color1=None), "backward_dual_m2d: dmeans2D_color1 must not be NULL"),
        (dict(dmeans2D_color1=rc.D + 2), "backward_dual_m2d: dmeans2D_color1 must be 4-byte aligned"),
        (dict(dl2_channels=3), "backward_dual_m2d: dl2_channels must be 1"),
        (dict(colors2=None), "colors2 required"),
        (dict(grads=None), "backward_dual_m2d: the mapping form only (dopacity, dcolors2 and dcolors or SH colours)"),
        (dict(grads=dict(dopacity=None)),
         "backward_dual_m2d: the mapping form only (dopacity, dcolors2 and dcolors or SH colours)"),
        (dict(dcolors2=None), "backward_dual_m2d: the mapping form only (dopacity, dcolors2 and dcolors or SH colours)"),
        (dict(grads=dict(dcolors=None)),
         "backward_dual_m2d: the mapping form only (dopacity, dcolors2 and dcolors or SH colours)"),
        # the sibling's own pointer check wins over the shared ones
        (dict(dmeans2D_color1=None, dl2_channels=3), "backward_dual_m2d: dmeans2D_color1 must not be NULL"),
    ]
    for over, msg in rows:
        assert m2d_call(**over) == (INVALID, msg), over
    # SH colours stand in for dcolors (the colour sums are formed for the SH chain): accepted on an empty map
    assert m2d_call(grads=dict(dcolors=None), gaussians=dict(P=0, shs=rc.D, M=1))[0] == OK


def test_accumulate_mean2d_refusals_need_no_device():
    fn, D = rc.lib.gsr_accumulate_mean2d, rc.D
    err = lambda: rc.lib.gsr_last_error().decode()  # noqa: E731
    assert fn(0, None, None, None, None, None, None) == OK
    assert (fn(-1, D, D, D, D, D, None), err()) == (INVALID, "accumulate_mean2d: bad size")
    for k in range(5):
        args = [D] * 5
        args[k] = None
        assert (fn(4, *args, None), err()) == (INVALID, "accumulate_mean2d: null pointer"), k


def test_means2d_keywords_exclude_each_other():
    st = rasterizer.GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4)[None],
                                                  torch.eye(4)[None], 0, torch.zeros(3), False)
    z = torch.zeros(2, 3)
    args = (z, z, None, z, z, torch.zeros(2, 1), z, torch.zeros(2, 4), None, st)
    with pytest.raises(ValueError, match="exclude each other"):
        rasterizer.rasterize_gaussians_dual(*args, grad2_channels=1, means2D_grad_sum=True, means2D_grad_color1=True)
    with pytest.raises(ValueError, match="mapping form"):  # the variant differentiates the depth channel only
        rasterizer.rasterize_gaussians_dual(*args, grad2_channels=3, means2D_grad_color1=True)
    with pytest.raises(ValueError, match="mapping form"):
        rasterizer.rasterize_gaussians_dual(*args, grad2_channels=1, means2D_grad_color1=True, sh_adam=object())


def _cpu_map(P=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = {"means3D": torch.randn(P, 3, generator=g), "rgb_colors": torch.rand(P, 3, generator=g),
              "unnorm_rotations": torch.randn(P, 4, generator=g), "logit_opacities": torch.randn(P, 1, generator=g),
              "log_scales": torch.log(0.02 + 0.2 * torch.rand(P, 1, generator=g)),  # both sides of 0.01 r
              "cam_unnorm_rots": torch.zeros(1, 4, 2), "cam_trans": torch.zeros(1, 3, 2)}
    params = {k: torch.nn.Parameter(v) for k, v in params.items()}
    means2D = torch.zeros(P, 3, requires_grad=True)
    means2D.grad = 4e-4 * torch.randn(P, 3, generator=g)
    variables = {"means2D_gradient_accum": 2e-4 * torch.rand(P, generator=g), "denom": torch.ones(P),
                 "max_2D_radius": torch.zeros(P), "scene_radius": torch.tensor(10.0),
                 "seen": torch.rand(P, generator=g) > 0.3, "means2D": means2D}
    opt = torch.optim.Adam([{"params": [v], "name": k, "lr": 1e-3} for k, v in params.items()], eps=1e-15)
    sum((v * v).sum() for v in params.values()).backward()  # one step, so the moments exist and are not zero
    opt.step()
    return params, variables, opt


def test_densify_without_its_own_accumulation_equals_accumulating_by_hand():
    """surgery.densify(accumulate=False) after the caller added the iteration's statistics itself is today's
    path: the same clones, splits (torch.normal under the same seed), removals, parameters and Adam moments."""
    dd = dict(start_after=0, remove_big_after=0, stop_after=4, densify_every=2, grad_thresh=2e-4, num_to_split_into=2,
              removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005, reset_opacities_every=3000,
              reset_opacities=False)
    pa, va, oa = _cpu_map()
    pb, vb, ob = _cpu_map()
    torch.manual_seed(7)
    pa, va = surgery.densify(pa, va, oa, 2, dd)
    seen = vb["seen"]  # slam_external.py:100-104, by hand
    vb["means2D_gradient_accum"][seen] += torch.norm(vb["means2D"].grad[seen, :2], dim=-1)
    vb["denom"][seen] += 1
    before = copy.deepcopy({k: vb[k] for k in ("means2D_gradient_accum", "denom")})
    torch.manual_seed(7)
    pb, vb = surgery.densify(pb, vb, ob, 2, dd, accumulate=False)
    assert pa["means3D"].shape[0] != 40  # clones / splits / removals happened
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
        sa, sb = oa.state[pa[k]], ob.state[pb[k]]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), k
    for k in ("means2D_gradient_accum", "denom", "max_2D_radius"):
        assert torch.equal(va[k], vb[k]), k
    # outside the schedule accumulate=False leaves the statistics alone; the default still accumulates
    pc, vc, oc = _cpu_map()
    vc["means2D_gradient_accum"], vc["denom"] = before["means2D_gradient_accum"].clone(), before["denom"].clone()
    surgery.densify(pc, vc, oc, 3, dd, accumulate=False)
    assert torch.equal(vc["means2D_gradient_accum"], before["means2D_gradient_accum"])
    surgery.densify(pc, vc, oc, 3, dd)
    assert not torch.equal(vc["means2D_gradient_accum"], before["means2D_gradient_accum"])
