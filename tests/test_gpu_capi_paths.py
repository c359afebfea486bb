"""The C entry points' host paths on the device (csrc/gsr_capi.hip): the refusals that come after the stream's
device has been looked up, and the allocator calls (kind, bytes) of the main call forms.

Scene: make_scene(10, 48, 32, seed=0), 6 tiles.  The refusals here all return before any launch that would use
the missing buffer (radii: before preprocess; geometry / image and the count matrix: before the first launch;
the binning buffer: after preprocess and the count scan, before the duplicate; the backward scratch: before the
first launch), so nothing faults; each test then repeats a valid call on the same stream and expects the image
it rendered before the refusal.

The allocator sequences are compared with tests/golden/capi_alloc_sequence.json, recorded from the commit before
the entry points were split into call records and steps.  Bytes depend on P, the image size, num_rendered and
(through the geometry layout's shift) the device's CU count: they are asserted on a 256-CU device, kinds and
order on any other.
"""
import ctypes
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_alloc_sequence.json")
GEOM, BINNING, IMAGE, SCRATCH = 0, 1, 2, 3
INVALID, ALLOC = -1, -2


class Rig:
    """One scene's device tensors, ctypes structs and a recording allocator that can refuse one kind."""

    def __init__(self, device):
        from splatam_amd import _C
        from splatam_amd._lib import ALLOC_FN, GsrGaussians, lib
        from splatam_amd.scenes import make_scene
        from splatam_amd.slam import camera_settings
        self.lib, self.device = lib, device
        sc = make_scene(10, 48, 32, seed=0).to(device)
        self.sc = sc
        st = camera_settings(sc.cam, device)
        self.H, self.W, self.P = st.image_height, st.image_width, sc.P
        self.s, self._keep = _C._settings(st.bg, st.viewmatrix, st.projmatrix, st.campos, st.tanfovx, st.tanfovy,
                                          self.H, self.W, st.scale_modifier, st.sh_degree, st.prefiltered, device)
        self.g = GsrGaussians(P=sc.P, M=0, means3D=sc.means3D.data_ptr(), colors_precomp=sc.colors.data_ptr(),
                              opacities=sc.opacities.data_ptr(), scales=sc.scales.data_ptr(),
                              rotations=sc.rotations.data_ptr())
        f32 = dict(dtype=torch.float32, device=device)
        self.colors2 = torch.rand(sc.P, 3, **f32)
        self.color, self.color2 = torch.empty(3, self.H, self.W, **f32), torch.empty(3, self.H, self.W, **f32)
        self.depth = torch.empty(1, self.H, self.W, **f32)
        self.radii = torch.empty(sc.P, dtype=torch.int32, device=device)
        self.stream = _C._stream(device)
        self.calls, self.bufs, self.refuse = [], {}, None
        self.cb = ALLOC_FN(self._alloc)

    def _alloc(self, ctx, kind, nbytes):
        self.calls.append([int(kind), int(nbytes)])
        if kind == self.refuse:
            return None
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
        self.bufs[int(kind)] = t
        return t.data_ptr()

    def err(self):
        return self.lib.gsr_last_error().decode()

    def forward(self, radii=True):
        self.color.fill_(-1.0)
        return self.lib.gsr_forward(ctypes.byref(self.s), ctypes.byref(self.g), self.color.data_ptr(),
                                    self.depth.data_ptr(), self.radii.data_ptr() if radii else None, self.cb, None,
                                    self.stream)

    def image(self):
        n = self.forward()
        assert n > 0, self.err()
        torch.cuda.synchronize()
        return n, self.color.clone()

    def grads(self, only=None):
        from splatam_amd._lib import GsrGrads
        f32 = dict(dtype=torch.float32, device=self.device)
        P = self.P
        shapes = dict(dmeans2D=(P, 3), dcolors=(P, 3), dopacity=(P, 1), dmeans3D=(P, 3), dcov3D=(P, 6),
                      dscales=(P, 3), drotations=(P, 4))
        self._gr = {k: torch.zeros(*v, **f32) for k, v in shapes.items() if only is None or k in only}
        return GsrGrads(**{k: t.data_ptr() for k, t in self._gr.items()})

    def backward(self, n, state, power=1, only=None):
        gr = self.grads(only)
        self._dpix = torch.ones(3, self.H, self.W, dtype=torch.float32, device=self.device)
        return self.lib.gsr_backward(ctypes.byref(self.s), ctypes.byref(self.g), self.radii.data_ptr(),
                                     self._dpix.data_ptr(), n, state[GEOM].data_ptr(), state[BINNING].data_ptr(),
                                     state[IMAGE].data_ptr(), power, ctypes.byref(gr), self.cb, None, self.stream)

    def reuse_if_equal(self, prev_n, prev, prev_radii, other):
        """gsr_forward_reuse_if_equal comparing this scene's rotations / opacities / scales with `other`'s."""
        mine = (self.sc.rotations, self.sc.opacities, self.sc.scales)
        a = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in mine])
        b = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in other])
        n = (ctypes.c_longlong * 3)(*[t.numel() for t in mine])
        reused = ctypes.c_int(-1)
        rc = self.lib.gsr_forward_reuse_if_equal(
            ctypes.byref(self.s), ctypes.byref(self.g), 3, a, b, n, prev_n, prev[GEOM].data_ptr(),
            prev[BINNING].data_ptr(), prev[IMAGE].data_ptr(), prev_radii.data_ptr(), self.color.data_ptr(),
            self.depth.data_ptr(), self.radii.data_ptr(), ctypes.byref(reused), self.cb, None, self.stream)
        return rc, reused.value


@pytest.fixture()
def rig(cuda):
    with torch.cuda.device(cuda):
        yield Rig(cuda)
        torch.cuda.synchronize()


def _renders_as_before(rig, before):
    rig.refuse = None
    n, after = rig.image()
    assert n == before[0] and torch.equal(after, before[1])


def test_radii_null_is_refused_before_preprocess(rig):
    before = rig.image()
    assert rig.forward(radii=False) == INVALID and rig.err() == "radii output required"
    _renders_as_before(rig, before)


@pytest.mark.parametrize("kind,msg", [(GEOM, "allocator returned NULL (geom/image buffer)"),
                                      (IMAGE, "allocator returned NULL (geom/image buffer)"),
                                      (SCRATCH, "allocator returned NULL (tile count matrix)"),
                                      (BINNING, "allocator returned NULL (binning buffer)")])
def test_forward_allocator_null(rig, kind, msg):
    before = rig.image()
    rig.refuse = kind
    assert rig.forward() == ALLOC and rig.err() == msg
    _renders_as_before(rig, before)


def test_backward_scratch_allocator_null(rig):
    before = rig.image()
    state = dict(rig.bufs)
    rig.refuse = SCRATCH
    assert rig.backward(before[0], state) == ALLOC and rig.err() == "allocator returned NULL (backward scratch)"
    rig.refuse = None
    assert rig.backward(before[0], state) == 0, rig.err()
    torch.cuda.synchronize()
    assert torch.isfinite(rig._gr["dmeans3D"]).all() and rig._gr["dmeans3D"].any()
    _renders_as_before(rig, before)


def alloc_sequences(rig):
    """{call form: [[kind, bytes], ...]} of the forms the golden file lists, and the scene's num_rendered."""
    lib, out = rig.lib, {}

    def take():
        seq, rig.calls = rig.calls, []
        return seq

    n = rig.forward()
    assert n > 0, rig.err()
    state, radii = dict(rig.bufs), rig.radii.clone()
    out["num_rendered"] = n
    assert rig.backward(n, state) == 0, rig.err()
    out["eager_forward_backward"] = take()

    status = torch.zeros(4, dtype=torch.int32, device=rig.device)
    rc = lib.gsr_forward_dual_static(ctypes.byref(rig.s), ctypes.byref(rig.g), rig.colors2.data_ptr(), 2048,
                                     status.data_ptr(), rig.color.data_ptr(), rig.color2.data_ptr(),
                                     rig.depth.data_ptr(), rig.radii.data_ptr(), rig.cb, None, rig.stream)
    assert rc == 2048, rig.err()
    out["static_dual_forward"] = take()

    assert rig.backward(n, state, power=2) == 0, rig.err()
    out["power2_backward"] = take()
    assert rig.backward(n, state, power=2, only=("dmeans3D", "dopacity")) == 0, rig.err()
    out["fisher_backward"] = take()

    same = (rig.sc.rotations, rig.sc.opacities, rig.sc.scales)
    rc, reused = rig.reuse_if_equal(n, state, radii, same)
    assert (rc, reused) == (n, 1), rig.err()
    out["reuse_if_equal_hit"] = take()
    other = (rig.sc.rotations, rig.sc.opacities + 0.25, rig.sc.scales)
    rc, reused = rig.reuse_if_equal(n, state, radii, other)
    assert (rc, reused) == (n, 0), rig.err()
    out["reuse_if_equal_miss"] = take()
    torch.cuda.synchronize()
    return out


def test_allocator_call_sequences(rig):
    gold = json.load(open(GOLDEN))
    assert gold["cus"] == 256
    got = alloc_sequences(rig)
    cus = torch.cuda.get_device_properties(rig.device).multi_processor_count
    forms = [k for k in gold if k not in ("cus", "num_rendered")]
    assert len(forms) == 6 and got["num_rendered"] == gold["num_rendered"]
    for form in forms:
        if cus == 256:
            assert got[form] == gold[form], form
        else:
            assert [k for k, _ in got[form]] == [k for k, _ in gold[form]], form
