"""Every Python wrapper form makes the libgsr.so calls it made when tests/golden/py_call_forms.json was recorded.

The `lib` that splatam_amd._C and splatam_amd.glue see is replaced by a proxy that forwards every call and notes
the entry point's name and, per argument, "null" / "ptr" for a pointer, the value of an int, the repr of a float,
and for a struct passed by reference its type name with the same classification of every field (so
store_rendervars, alive, q_stride, capacity, step, ... are pinned).  The golden file is written by
tools/record_call_forms.py, which runs this module's CASES through this module's recorder; the test holds no
expectation of its own.

This is not a complete pin: every pointer is noted only as "ptr" or "null", so two pointer arguments of the same
kind changing places (out_color / out_color2, dim / dds, cam_q / cam_t) or a wrong column offset do not show here.
The bit-for-bit suites (test_gpu_slam, test_gpu_mapping, test_gpu_track_extend, test_gpu_parity, ...) catch those.

Scene: make_scene(10, 48, 32, seed=0) (6 tiles, 10 Gaussians), static capacity 4096, two pose columns, t = 1.
"""
import ctypes
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "py_call_forms.json")
CAP = 4096
_INTS = (ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_size_t)
_FLOATS = (ctypes.c_float, ctypes.c_double)


def _struct(s):
    return {"struct": type(s).__name__, "fields": {n: _classify(getattr(s, n), t) for n, t in s._fields_}}


def _classify(v, ctype):
    """One argument (or struct field) as the entry point declares it."""
    if isinstance(ctype, type) and issubclass(ctype, ctypes.Array):  # a struct's array field
        return [_classify(x, ctype._type_) for x in v]
    if ctype in _INTS:
        return int(v)
    if ctype in _FLOATS:
        return repr(float(v))
    if v is None:
        return "null"
    if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer) and \
            issubclass(ctype._type_, ctypes.Structure):
        if isinstance(v, ctypes.Array):  # an array of structs (gsr_adam_step)
            return [_struct(x) for x in v]
        return _struct(v._obj)  # ctypes.byref(struct)
    if isinstance(ctype, type) and issubclass(ctype, ctypes._CFuncPtr):
        return "callback"
    if isinstance(v, int):
        return "ptr" if v else "null"
    return "ptr"  # a ctypes array or byref handed to a void pointer


class Recorder:
    """Stands in for `lib`: forwards every call, noting it in `log`."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)  # (AttributeError for a missing symbol, as on the library itself)

        def call(*args):
            types = fn.argtypes or []
            assert len(args) == len(types), (name, len(args), len(types))
            self.log.append([name, [_classify(a, t) for a, t in zip(args, types)]])
            return fn(*args)
        return call


class Rig:
    """The scene's tensors and the small builders the cases share."""

    def __init__(self, dev):
        from splatam_amd.scenes import make_scene
        from splatam_amd.slam import MappingConfig, TrackingConfig, camera_settings, init_tracking_params
        self.dev = dev
        sc = make_scene(10, 48, 32, seed=0)
        self.params = init_tracking_params(sc, num_frames=2, device=dev)
        self.cam = camera_settings(sc.cam, dev)
        self.P, self.H, self.W = sc.P, self.cam.image_height, self.cam.image_width
        g = torch.Generator().manual_seed(7)
        self.gt_im = torch.rand(3, self.H, self.W, generator=g).to(dev)
        self.gt_d = (0.5 + 4.0 * torch.rand(1, self.H, self.W, generator=g)).to(dev)
        self.shs = torch.rand(self.P, 1, 3, generator=g).to(dev)
        self.w2c = torch.eye(4, device=dev)
        self.curr = {"cam": self.cam, "w2c": self.w2c, "im": self.gt_im, "depth": self.gt_d}
        self.seed = torch.ones((), device=dev)
        self.cfg, self.mcfg = TrackingConfig(), MappingConfig()
        self.empty = torch.Tensor([])

    def status(self):
        return torch.zeros(4, dtype=torch.int32, device=self.dev)

    def terms(self):
        return torch.zeros(2, dtype=torch.float32, device=self.dev)

    def alive(self):
        a = torch.ones(self.P, dtype=torch.uint8, device=self.dev)
        a[3] = 0
        return a

    def pose_leaves(self):
        p = dict(self.params)
        for k in ("cam_unnorm_rots", "cam_trans"):
            p[k] = self.params[k].detach().clone().requires_grad_(True)
        return p

    def map_leaves(self, shs=False):
        p = {k: v.detach().clone() for k, v in self.params.items()}
        if shs:
            p["shs"] = self.shs.clone()
            del p["rgb_colors"]
        for k, v in p.items():
            if not k.startswith("cam_"):
                v.requires_grad_(True)
        return p

    def pose_adam(self, status=None):
        """With the bookkeeping the trackers give it: best-candidate selection and a status row to guard on."""
        from splatam_amd.glue import PoseAdam
        a = PoseAdam(self.dev, track_best=True)
        a.status, a.capacity = (self.status() if status is None else status), CAP
        return a

    def rendervars(self):
        from splatam_amd.glue import track_transform
        with torch.no_grad():
            return track_transform(self.params, 1, self.w2c)  # means, rot, dcol, opac, scales

    def dual(self, _C, capacity=0, status=None, alive=None, xform=None, rv=None, sh=None):
        c = self.cam
        means, rot, dcol, opac, scales = rv if rv is not None else self.rendervars()
        colors = self.empty if sh is not None else self.params["rgb_colors"]
        return _C.rasterize_gaussians_dual(
            c.bg, means, colors, dcol, opac, scales, rot, c.scale_modifier, self.empty, c.viewmatrix, c.projmatrix,
            c.tanfovx, c.tanfovy, c.image_height, c.image_width, self.empty if sh is None else sh, c.sh_degree,
            c.campos, c.prefiltered, capacity=capacity, status=status, alive=alive, xform=xform), \
            (means, rot, dcol, opac, scales)

    def dual_backward(self, _C, sh=None, **kw):
        c = self.cam
        (n, _, _, radii, geom, binning, img, _), (means, rot, dcol, _, scales) = self.dual(_C, sh=sh)
        d1 = torch.ones(3, self.H, self.W, device=self.dev)
        d2 = torch.zeros(3, self.H, self.W, device=self.dev)
        d2[0] = 1.0
        colors = self.empty if sh is not None else self.params["rgb_colors"]
        return _C.rasterize_gaussians_dual_backward(
            c.bg, means, radii, colors, dcol, scales, rot, c.scale_modifier, self.empty, c.viewmatrix, c.projmatrix,
            c.tanfovx, c.tanfovy, d1, d2, self.empty if sh is None else sh, c.sh_degree, c.campos, geom, n, binning,
            img, **kw)


# ------------------------------------------------------------------------------------------- cases --
def _tracking_iteration(rig, mp, adam, flags=(), static=True, seed=True, backward_seed=None, **kw):
    from splatam_amd import glue
    for name, value in flags:
        mp.setattr(glue, name, value)
    status = rig.status() if static else None
    opt = rig.pose_adam(status) if adam else None
    p = rig.pose_leaves()
    s = rig.seed if seed else None
    loss, _ = glue.tracking_iteration(p, rig.curr, 1, rig.cfg, pose_adam=opt, capacity=CAP if static else 0,
                                      status=status, seed=s, **kw)
    if backward_seed is not None:
        torch.autograd.backward(loss, backward_seed)
    elif s is not None:
        torch.autograd.backward(loss, s)
    else:
        loss.backward()


def _ti(**kw):
    return lambda rig, mp, adam: _tracking_iteration(rig, mp, adam, **kw)


_TI_FORMS = {
    "eager": _ti(static=False, seed=False),
    "eager_seed": _ti(static=False),
    "static_xf_unfused": _ti(flags=(("_XF_FUSED", False),)),
    "static_render_unfused": _ti(flags=(("_RENDER_FUSED", False),)),
    "fused_images": _ti(images=True),
    "fused_no_images": _ti(images=False),
    "fused_alive": lambda rig, mp, adam: _tracking_iteration(rig, mp, adam, alive=rig.alive()),
    "fused_terms": lambda rig, mp, adam: _tracking_iteration(rig, mp, adam, terms=rig.terms()),
}


def _dual_forms(rig, mp):
    from splatam_amd import _C, glue
    rig.dual(_C)
    rig.dual(_C, CAP, rig.status())
    rig.dual(_C, CAP, rig.status(), alive=rig.alive())
    defer = []
    p = rig.map_leaves()
    with torch.no_grad():
        rv = glue.map_transform(p, 1, rig.w2c, defer=defer)[:5]
    rig.dual(_C, CAP, rig.status(), xform=defer[0], rv=rv)
    rig.dual(_C, CAP, rig.status(), alive=rig.alive(), xform=defer[0], rv=rv)


def _dual_backward_forms(rig, mp):
    from splatam_amd import _C
    from splatam_amd.glue import MapAdam
    rig.dual_backward(_C)
    rig.dual_backward(_C, needs=(False, True, False, True, False, False, False, True, False))
    rig.dual_backward(_C, dl2_channels=1)
    p = rig.map_leaves(shs=True)
    adam = MapAdam(p, rig.mcfg.lrs, color_key="shs")
    sa = adam.struct()
    sa.step = 1
    rig.dual_backward(_C, sh=p["shs"].detach(), sh_adam=sa)


def _track_transform(rig, mp):
    from splatam_amd import glue
    for opt in (None, rig.pose_adam()):
        p = rig.pose_leaves()
        means, rot, dcol, _, _ = glue.track_transform(p, 1, rig.w2c, opt)
        (means.sum() + dcol.sum()).backward()


def _tracking_l1(rig, mp):
    from splatam_amd import glue
    for seed, terms, other in ((None, None, False), (rig.seed, None, False), (None, rig.terms(), False),
                               (rig.seed, rig.terms(), False), (rig.seed, None, True)):
        im = torch.rand(3, rig.H, rig.W, device=rig.dev, requires_grad=True)
        ds = torch.rand(3, rig.H, rig.W, device=rig.dev, requires_grad=True)
        loss = glue.tracking_l1(im, ds, rig.gt_im, rig.gt_d, seed=seed, terms=terms)
        if seed is None:
            loss.backward()
        else:
            torch.autograd.backward(loss, 2.0 * seed if other else seed)


def _map_transform(rig, mp):
    from splatam_amd import _C, glue
    p = rig.map_leaves()
    outs = glue.map_transform(p, 1, rig.w2c)
    sum(o.sum() for o in outs).backward()
    p = rig.map_leaves()
    adam = glue.MapAdam(p, rig.mcfg.lrs)
    outs = glue.map_transform(p, 1, rig.w2c, adam=adam)
    sum(o.sum() for o in outs).backward()
    p = rig.map_leaves()
    defer = []
    outs = glue.map_transform(p, 1, rig.w2c, defer=defer)
    rig.dual(_C, CAP, rig.status(), xform=defer[0], rv=[o.detach() for o in outs[:5]])
    sum(o.sum() for o in outs).backward()


def _mapping_loss(rig, mp):
    from splatam_amd import glue
    im = torch.rand(3, rig.H, rig.W, device=rig.dev, requires_grad=True)
    ds = torch.rand(3, rig.H, rig.W, device=rig.dev, requires_grad=True)
    glue.mapping_loss(im, ds, rig.gt_im, rig.gt_d).backward()


def _mapping_iteration(rig, mp):
    """The fused mapping iteration (slam._get_loss_mapping_fused): eager, then static with the transform deferred
    into the forward and the optimizer guarded by it."""
    from splatam_amd import glue, slam
    for cap in (0, CAP):
        p = rig.map_leaves()
        adam = glue.MapAdam(p, rig.mcfg.lrs)
        status = rig.status() if cap else None
        adam.status, adam.capacity = status, cap
        loss, _, _ = slam._get_loss_mapping_fused(p, rig.curr, 1, rig.mcfg, adam=adam, capacity=cap, status=status)
        loss.backward()


def _dual_render_l1(rig, mp):
    from splatam_amd import glue
    for other, terms in ((False, None), (True, None), (False, rig.terms())):
        means, rot, dcol, opac, scales = [t.clone().requires_grad_(True) for t in rig.rendervars()]
        loss, _ = glue.dual_render_tracking_l1(means, rig.params["rgb_colors"], dcol, opac, scales, rot, rig.cam, CAP,
                                               rig.status(), rig.gt_im, rig.gt_d, rig.cfg, rig.seed, terms=terms)
        torch.autograd.backward(loss, 2.0 * rig.seed if other else rig.seed)


def _single_ctypes(rig, mp):
    """rasterize_gaussians on the ctypes binding: a miss (the rig's tensors are new objects, so whatever forward the
    binding remembers is another's), a geometry-reuse hit, the backward."""
    from splatam_amd import _C
    mp.setattr(_C, "_NATIVE_ON", False)
    mp.setattr(_C, "_GEOM_CACHE", True)
    c = rig.cam
    means, rot, dcol, opac, scales = rig.rendervars()
    outs = []
    for colors in (rig.params["rgb_colors"], dcol):
        outs.append(_C.rasterize_gaussians(c.bg, means, colors, opac, scales, rot, c.scale_modifier, rig.empty,
                                           c.viewmatrix, c.projmatrix, c.tanfovx, c.tanfovy, c.image_height,
                                           c.image_width, rig.empty, c.sh_degree, c.campos, c.prefiltered))
    n, _, radii, geom, binning, img, _ = outs[1]
    _C.rasterize_gaussians_backward(c.bg, means, radii, dcol, scales, rot, c.scale_modifier, rig.empty, c.viewmatrix,
                                    c.projmatrix, c.tanfovx, c.tanfovy, torch.ones(3, rig.H, rig.W, device=rig.dev),
                                    rig.empty, c.sh_degree, c.campos, geom, n, binning, img)


CASES = {}
for _name, _fn in _TI_FORMS.items():
    for _adam in (False, True):
        CASES[f"tracking_iteration/{_name}/{'adam' if _adam else 'grad'}"] = \
            (lambda rig, mp, fn=_fn, adam=_adam: fn(rig, mp, adam))
CASES["tracking_iteration/fused_images/other_seed"] = \
    lambda rig, mp: _tracking_iteration(rig, mp, False, images=True, backward_seed=2.0 * rig.seed)
CASES["tracking_iteration/fused_images/xf_store"] = \
    lambda rig, mp: _tracking_iteration(rig, mp, False, flags=(("_XF_STORE", True),), images=True)
CASES.update({
    "rasterize_gaussians_dual": _dual_forms,
    "rasterize_gaussians_dual_backward": _dual_backward_forms,
    "track_transform": _track_transform,
    "tracking_l1": _tracking_l1,
    "map_transform": _map_transform,
    "mapping_loss": _mapping_loss,
    "mapping_iteration": _mapping_iteration,
    "dual_render_tracking_l1": _dual_render_l1,
    "rasterize_gaussians_ctypes": _single_ctypes,
})


def record(name, dev, mp):
    """The calls case `name` makes, as the JSON-ready list the golden file holds.  mp: a pytest MonkeyPatch."""
    from splatam_amd import _C, glue
    from splatam_amd._lib import lib
    with torch.cuda.device(dev):
        torch.manual_seed(0)
        rig = Rig(dev)  # (built on the real library: its own launches are not part of the case)
        rec = Recorder(lib)
        mp.setattr(_C, "lib", rec)
        mp.setattr(glue, "lib", rec)
        CASES[name](rig, mp)
        torch.cuda.synchronize(dev)
    return rec.log


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_call_form(cuda, name, golden, monkeypatch):
    got = json.loads(json.dumps(record(name, cuda, monkeypatch)))
    want = golden[name]
    assert [c[0] for c in got] == [c[0] for c in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {k}: {g[0]}"
