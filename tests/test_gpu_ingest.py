"""The raw-frame intake on the GPU: gsr_ingest_frame (splatam_amd.ingest.ingest_device) bitwise against the numpy
restatement of tests/ingest_ref.py -- every byte, every uint16 reading, inputs at every byte / element offset of a
larger buffer, outputs inside poisoned guard bands, both store forms (float4 when H W % 4 == 0 and the outputs are
16-byte aligned, scalar otherwise) -- its small outputs against gsr_resize_frame of its own full frame, a graph
replay, and the two sequence loops fed raw frames against the same loops fed ingest_literal's float frames, plus
the on-arrival report.

The 64x48 capture is tests/test_gpu_track_res.py's (imported), quantised to a sensor's uint8 / uint16 (1 mm
units); the tracked sequence uses tests/test_gpu_online.py's scene (20 000 Gaussians, 320x240).  Everything is
bitwise except the arrival rows, which carry tests/test_gpu_eval.py's allowance for frame_metrics against
evaluate_literal (BOUND plus the literal's own distance from the float64 restatement on those very images)."""
import contextlib

import numpy as np
import pytest
import torch

import eval_ref as er
import ingest_ref as ir
from splatam_amd import ingest as ig
from splatam_amd import resize as rz

pytestmark = pytest.mark.gpu

POISON = -77.25
SCALE, MAX_DEPTH = 5000.0, ir.MAX_DEPTH  # (readings from 47500 up are far)
# 1 pixel; a tail quad alone; N % 4 != 0 over two quads; N % 4 == 0 (the float4 stores, when aligned); more than one block of quads
SIZES = ((1, 1), (3, 1), (5, 7), (4, 6), (37, 53))
OFFSETS = ((0, 0), (1, 1), (2, 0), (3, 1))  # (colour byte offset, depth element offset) inside the capture buffers
GUARDS = (8, 5)  # floats ahead of each output: 32 bytes (16-byte aligned) and 20 bytes (4-byte aligned only)


def _dev_raw(rgb: np.ndarray, d16: np.ndarray, dev, boff: int = 0, eoff: int = 0, int16: bool = False):
    """The raw frame as slices of larger device buffers that start `boff` bytes / `eoff` elements in."""
    H, W = d16.shape
    cb = torch.zeros(boff + rgb.size + 5, dtype=torch.uint8, device=dev)
    cb[boff:boff + rgb.size] = torch.from_numpy(rgb.reshape(-1)).to(dev)
    db = torch.zeros(eoff + d16.size + 3, dtype=torch.int16, device=dev)
    db[eoff:eoff + d16.size] = torch.from_numpy(np.ascontiguousarray(d16).view(np.int16).reshape(-1)).to(dev)
    d = db[eoff:eoff + d16.size].view(H, W)
    return cb[boff:boff + rgb.size].view(H, W, 3), (d if int16 else d.view(torch.uint16))


def _guarded_frame(size, dev, g: int):
    """An output frame inside poisoned buffers with g floats of guard on either side: (frame, buffers)."""
    h, w = size
    bufs = {k: torch.full((2 * g + c * h * w,), POISON, dtype=torch.float32, device=dev) for k, c in (("im", 3), ("depth", 1))}
    return {k: bufs[k][g:g + c * h * w].view(c, h, w) for k, c in (("im", 3), ("depth", 1))}, bufs


def _guards_intact(bufs, g: int) -> bool:
    return all(bool((b[:g] == POISON).all()) and bool((b[-g:] == POISON).all()) for b in bufs.values())


def _same_bits(frame: dict, im: np.ndarray, d: np.ndarray):
    assert np.array_equal(ir.bits(frame["im"].cpu().numpy()), ir.bits(im))
    assert np.array_equal(ir.bits(frame["depth"].cpu().numpy()), ir.bits(d))


# ------------------------------------------------------------------ the full frame

@pytest.mark.parametrize("guard", GUARDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_full_frame_bitwise_at_every_offset(cuda, H, W, guard):
    rgb, d16 = ir.raw_frame(H, W, seed=H + W)
    want = ir.frame(rgb, d16, SCALE, MAX_DEPTH)
    for boff, eoff in OFFSETS:
        r, d = _dev_raw(rgb, d16, cuda, boff, eoff)
        assert r.data_ptr() % 4 == boff and d.data_ptr() % 4 == 2 * eoff
        frame, bufs = _guarded_frame((H, W), cuda, guard)
        assert frame["im"].data_ptr() % 16 == (4 * guard) % 16
        out = ig.ingest_device(r, d, SCALE, MAX_DEPTH, out=frame)
        torch.cuda.synchronize()
        assert out is frame and _guards_intact(bufs, guard), (boff, eoff)
        _same_bits(frame, *want)
    if H * W > 100:
        assert (want[1] == -1).any() and (want[1] == 0).any() and (want[1] > 0).any()


@pytest.mark.parametrize("guard", GUARDS)
def test_every_byte_and_every_reading(cuda, guard):
    """The all-bytes colour image (16x16) and the all-uint16 depth image (256x256), each with the other input
    tiled from it, at the three scales with and without max_depth; H W % 4 == 0, so guard 8 takes the float4 stores."""
    rgb16, d256 = ir.all_bytes_image(), ir.all_u16_image()
    d16 = d256.reshape(-1)[(np.arange(256) * 257) % 65536].reshape(16, 16).copy()  # (readings across the whole range)
    rgb256 = np.ascontiguousarray(np.tile(rgb16, (16, 16, 1)))
    for rgb, d in ((rgb16, d16), (rgb256, d256)):
        H, W = d.shape
        for scale in ir.SCALES:
            for max_depth in (None, MAX_DEPTH):
                r, dd = _dev_raw(rgb, d, cuda)
                frame, bufs = _guarded_frame((H, W), cuda, guard)
                ig.ingest_device(r, dd, scale, max_depth, out=frame)
                torch.cuda.synchronize()
                assert _guards_intact(bufs, guard)
                _same_bits(frame, *ir.frame(rgb, d, scale, max_depth))
    # fresh outputs (torch's alignment), the int16 carrier of the same bytes, and the literal form on the device
    r, dd = _dev_raw(rgb256, d256, cuda, int16=True)
    out = ig.ingest_device(r, dd, 6553.5, MAX_DEPTH)
    lit = ig.ingest_literal(r, dd, 6553.5, MAX_DEPTH)
    torch.cuda.synchronize()
    _same_bits(out, *ir.frame(rgb256, d256, 6553.5, MAX_DEPTH))
    assert torch.equal(out["im"], lit["im"]) and torch.equal(out["depth"], lit["depth"])
    # the depth rule is the float64 quotient rounded once, not a float32 multiply by the reciprocal (249 readings
    # tell at this scale), and the scale is taken as a double (6553.7 is no float32 value)
    plain = ig.ingest_device(r, dd, 6553.5)["depth"].cpu().numpy()
    assert int((ir.bits(plain) != ir.bits(ir.depth_f32_reciprocal(d256, 6553.5))).sum()) == 249
    other = ig.ingest_device(r, dd, 6553.7)["depth"].cpu().numpy()
    assert np.array_equal(ir.bits(other), ir.bits(ir.depth(d256, 6553.7)))
    assert not np.array_equal(ir.bits(other), ir.bits(ir.depth_f32_division(d256, 6553.7)))


def test_device_call_checks(cuda):
    rgb, d16 = ir.raw_frame(4, 6)
    r, d = _dev_raw(rgb, d16, cuda)
    for bad in (lambda: ig.ingest_device(r.float(), d, SCALE), lambda: ig.ingest_device(r, d.view(torch.int16).int(), SCALE),
                lambda: ig.ingest_device(r.permute(1, 0, 2), d.view(torch.int16).t().view(torch.uint16), SCALE),
                lambda: ig.ingest_device(r, d, SCALE, out=rz.empty_frame((4, 5), cuda)),
                lambda: ig.ingest_device(r.cpu(), d, SCALE)):
        with pytest.raises(RuntimeError):
            bad()
    for bad in (lambda: ig.ingest_device(r, d, 0.0), lambda: ig.ingest_device(r, d, SCALE, full=False),
                lambda: ig.ingest_device(r, d, SCALE, size2=(2, 3)), lambda: ig.ingest_device(r, d, SCALE, size=(0, 3)),
                lambda: ig.ingest_device(r, d, SCALE, size=(2, 3), out=rz.empty_frame((4, 6), cuda))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------ the small outputs

def test_small_outputs_are_resize_of_the_full_frame(cuda):
    H, W = 37, 53
    rgb, d16 = ir.raw_frame(H, W, seed=11)
    r, d = _dev_raw(rgb, d16, cuda, 1, 1)
    guard = 5
    outs, bufs = zip(*[_guarded_frame(s, cuda, guard) for s in ((H, W), (17, 29), (74, 106))])
    full, down, up = ig.ingest_device(r, d, SCALE, MAX_DEPTH, size=(17, 29), size2=(74, 106), out=outs)
    same = ig.ingest_device(r, d, SCALE, MAX_DEPTH, size=(H, W))[1]
    torch.cuda.synchronize()
    assert all(_guards_intact(b, guard) for b in bufs)
    _same_bits(full, *ir.frame(rgb, d16, SCALE, MAX_DEPTH))
    plain = ig.ingest_device(r, d, SCALE, MAX_DEPTH)
    for got, size in ((down, (17, 29)), (up, (74, 106)), (same, (H, W))):
        via = rz.resize_device(plain, size)  # gsr_resize_frame of the float frame: the same bits
        assert torch.equal(got["im"], via["im"]) and torch.equal(got["depth"], via["depth"]), size
        _same_bits(got, *ir.small(rgb, d16, SCALE, MAX_DEPTH, size))
    assert torch.equal(same["im"], full["im"]) and torch.equal(same["depth"], full["depth"])  # every weight zero
    # full=False: the same small frames, and no full frame is written
    a, b = ig.ingest_device(r, d, SCALE, MAX_DEPTH, size=(17, 29), size2=(74, 106), full=False)
    only = ig.ingest_device(r, d, SCALE, MAX_DEPTH, size=(74, 106), full=False)
    for got, want in ((a, down), (b, up), (only, up)):
        assert torch.equal(got["im"], want["im"]) and torch.equal(got["depth"], want["depth"])
    # a far tap stays -1 in the small depth (nearest: a copied value, never a blend)
    assert (down["depth"] == -1).any() and (up["depth"] == -1).any()


def test_graph_replay(cuda):
    """One call captured, replayed after new bytes were written in place: the eager call's bits on the new bytes."""
    H, W = 37, 53
    a, b = ir.raw_frame(H, W, seed=1), ir.raw_frame(H, W, seed=2)
    r, d = _dev_raw(*a, cuda, 3, 1)
    outs = [rz.empty_frame(s, cuda) for s in ((H, W), (17, 29), (74, 106))]
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        ig.ingest_device(r, d, SCALE, MAX_DEPTH, size=(17, 29), size2=(74, 106), out=outs)  # (warm-up)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    first = [{k: v.clone() for k, v in o.items()} for o in outs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ig.ingest_device(r, d, SCALE, MAX_DEPTH, size=(17, 29), size2=(74, 106), out=outs)
    nr, nd = _dev_raw(*b, cuda)
    r.copy_(nr)
    d.view(torch.int16).copy_(nd.view(torch.int16))
    for o in outs:
        o["im"].fill_(POISON), o["depth"].fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    eager = ig.ingest_device(nr, nd, SCALE, MAX_DEPTH, size=(17, 29), size2=(74, 106))
    for got, want, old in zip(outs, eager, first):
        assert torch.equal(got["im"], want["im"]) and torch.equal(got["depth"], want["depth"])
        assert not torch.equal(got["im"], old["im"])
    _same_bits(outs[0], *ir.frame(*b, SCALE, MAX_DEPTH))


# ------------------------------------------------------------------ the sequence loops, fed raw frames

N_RAW = 3
SMALL = (24, 32)
PNG_SCALE = 1000.0
KW = dict(tracking_iters=20, track_replay=20, mapping_iters=10, prune=False, keyframe_policy="window",
          keyframe_every=2, window=3, track_size=SMALL, densify_size=SMALL, png_depth_scale=PNG_SCALE, max_depth=MAX_DEPTH)


def _quantise(frame: dict, dev):
    """A float frame as a sensor would deliver it: uint8 [H,W,3], uint16 [H,W] in 1 / PNG_SCALE m (device tensors)."""
    rgb = (frame["im"].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    d = (frame["depth"][0].clamp(0, 30) * PNG_SCALE).round().to(torch.int32)
    return rgb, (d & 0xFFFF).to(torch.int16).contiguous().view(torch.uint16)


def _odometry(gt, t: int) -> np.ndarray:
    """Frame t's true pose of tests/test_gpu_track_res.py's trajectory as an odometry pose (x, y, z, qx, qy, qz,
    qw): the camera-to-world transform, the inverse of w2c = [Rz(a) | (x_t, 0, 0)]."""
    q, tr = gt[0][0, :, t].double().cpu().numpy(), gt[1][0, :, t].double().cpu().numpy()
    a = 2.0 * np.arctan2(q[3], q[0])
    c, s = np.cos(a), np.sin(a)
    rt = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])  # Rz(a)^T
    return np.array([*(-rt @ tr), 0.0, 0.0, np.sin(-a / 2), np.cos(-a / 2)])


class RawCapture:
    def __init__(self, dev):
        import test_gpu_track_res as tr
        self.cap = cap = tr.Capture(dev)
        self.dev = dev
        self.raw = [_quantise(f, dev) for f in cap.frames[:N_RAW]]
        lit = [ig.ingest_literal(r, d, PNG_SCALE, MAX_DEPTH) for r, d in self.raw]
        self.lit = [{"im": f["im"], "depth": f["depth"]} for f in lit]
        self.poses = [_odometry(cap.gt, t) for t in range(N_RAW)]
        self.w2cs = [ig.odometry_w2c(self.poses[0], p).to(dev) for p in self.poses]
        self.capacity = cap.P0 + 2 * 64 * 48

    def sequence(self, frames, **kw):
        from splatam_amd.sequence import SlamSequence
        c = self.cap
        kw = dict(KW, **kw)
        return SlamSequence(kw.pop("params", c.params), frames, c.cam, c.w2c, c.intr, capacity=self.capacity,
                            bin_capacity=c.bin_cap, seed=0, num_frames=N_RAW, **kw)

    def per_frame(self, frames, **kw):
        from splatam_amd.sequence import PerFrameSlam
        c = self.cap
        return PerFrameSlam(c.params, frames, c.cam, c.w2c, c.intr, bin_capacity=c.bin_cap, num_frames=N_RAW,
                            **dict(KW, **kw))

    def first_raw(self):
        return [{"rgb_u8": self.raw[0][0], "depth_u16": self.raw[0][1], "pose": self.poses[0]}]


@pytest.fixture(scope="module")
def rawcap(cuda):
    return RawCapture(torch.device(cuda))


def _same_sequences(a, b):
    import test_gpu_track_res as tr
    tr._same_state(a, b)
    assert len(a.frames) == len(b.frames) == len(a.track_frames) == len(a.densify_frames)
    for t in range(len(a.frames)):
        for x, y in ((a.frames[t], b.frames[t]), (a.track_frames[t], b.track_frames[t]),
                     (a.densify_frames[t], b.densify_frames[t])):
            assert torch.equal(x["im"], y["im"]) and torch.equal(x["depth"], y["depth"]), t


@contextlib.contextmanager
def _counted_resizes():
    """The resize launches a capture makes while this is open (the list's length): resize_device as
    splatam_amd.capture's _make_small reads it, wrapped."""
    from splatam_amd import capture
    calls = []
    real = capture.resize_device
    capture.resize_device = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        yield calls
    finally:
        capture.resize_device = real


@pytest.fixture(scope="module")
def given_raw(rawcap):
    """The raw-fed sequence with given poses: the first raw frame at construction, the others pushed with their
    odometry poses; the resize launches it made are counted."""
    with _counted_resizes() as calls:
        seq = rawcap.sequence(rawcap.first_raw(), densify_mode="device", arrival_report=True)
        seq.frame(0)
        for t in range(1, N_RAW):
            assert seq.push_raw(*rawcap.raw[t], pose=rawcap.poses[t]) == t
    seq.check()
    torch.cuda.synchronize()
    return seq, len(calls)


def test_raw_sequence_with_given_poses(rawcap, given_raw):
    seq, resize_calls = given_raw
    assert resize_calls == 0  # the ingest launch made every small frame: _make_small was not called
    fed = rawcap.sequence(rawcap.lit[:1], densify_mode="device")
    fed.frame(0)
    with _counted_resizes() as fed_calls:
        for t in range(1, N_RAW):
            assert fed.push(rawcap.lit[t]["im"], rawcap.lit[t]["depth"], w2c=rawcap.w2cs[t]) == t
    assert len(fed_calls) >= N_RAW - 1  # (the counter is live: a float frame's small frames are resize launches)
    fed.check()
    torch.cuda.synchronize()
    _same_sequences(seq, fed)
    assert seq.tracking_iters_run == [0] * N_RAW and not hasattr(fed, "arrival")
    # the hole was densified: tests/test_gpu_track_res.py asks for more than 100 rows at 64x48; the densification
    # frame here has a quarter of those pixels
    assert int(seq.n_live.item()) - rawcap.cap.P0 > 25
    assert seq.track_frames[1]["im"].shape == (3, *SMALL) and seq.frames[1]["im"].shape == (3, 48, 64)
    with pytest.raises(ValueError):
        seq.push_raw(*rawcap.raw[0])  # beyond num_frames
    # w2c= is push()'s: the same column as the pose it came from
    other = rawcap.sequence(rawcap.first_raw(), densify_mode="device")
    other.frame(0)
    other.push_raw(*rawcap.raw[1], w2c=rawcap.w2cs[1])
    torch.cuda.synchronize()
    for k in ("cam_unnorm_rots", "cam_trans"):
        assert torch.equal(other.params[k][..., :2], seq.params[k][..., :2])


def test_raw_per_frame_loop(rawcap, given_raw):
    seq, _ = given_raw
    raw = rawcap.per_frame(rawcap.first_raw())
    raw.frame(0, seq.draws[0])
    for t in range(1, N_RAW):
        assert raw.push_raw(*rawcap.raw[t], sequence=seq.draws[t], pose=rawcap.poses[t]) == t
    lit = rawcap.per_frame(rawcap.lit)
    for t in range(N_RAW):
        lit.frame(t, seq.draws[t], w2c=rawcap.w2cs[t])
    torch.cuda.synchronize()
    assert raw.tracking_iters_run == lit.tracking_iters_run == [0] * N_RAW
    assert raw.p["means3D"].shape[0] == lit.p["means3D"].shape[0] > rawcap.cap.P0 + 25
    for k in raw.p:
        if torch.is_tensor(raw.p[k]):
            assert torch.equal(raw.p[k], lit.p[k]), k
    for t in range(N_RAW):
        for x, y in ((raw.frames[t], lit.frames[t]), (raw.track_frames[t], lit.track_frames[t]),
                     (raw.densify_frames[t], lit.densify_frames[t])):
            assert torch.equal(x["im"], y["im"]) and torch.equal(x["depth"], y["depth"]), t


def test_raw_first_frame_builds_the_map(rawcap):
    """SlamSequence(None, raw first frame): the map is born from the ingested frame's densification copy."""
    seq = rawcap.sequence(rawcap.first_raw(), params=None, densify_mode="device")
    lit = rawcap.sequence(rawcap.lit[:1], params=None, densify_mode="device")
    torch.cuda.synchronize()
    n = int(seq.n_live.item())
    assert n == int(lit.n_live.item()) == int((seq.densify_frames[0]["depth"] > 0).sum()) > 100
    for k, v in seq.live_params().items():
        if torch.is_tensor(v):
            assert torch.equal(v, lit.live_params()[k]), k


def test_arrival_report(rawcap, given_raw, monkeypatch):
    """Rows 1 and 2 of `arrival` against evaluate_literal of the render a PerFrameSlam run makes at the same point
    (after the frame's pose is written, before its densification), within tests/test_gpu_eval.py's allowance."""
    import test_gpu_eval as tge
    from splatam_amd import evaluate as ev
    seq, _ = given_raw
    assert seq.arrival.shape == (N_RAW, 8) and seq.arrival.dtype == torch.float32
    seen, real = [], ev.evaluate_literal
    monkeypatch.setattr(ev, "evaluate_literal", lambda *a, **k: (seen.append(a), real(*a, **k))[1])
    ref = rawcap.per_frame(rawcap.lit, densify_mode="device", arrival_report=True)
    for t in range(N_RAW):
        ref.frame(t, seq.draws[t], w2c=rawcap.w2cs[t])
    torch.cuda.synchronize()
    table = seq.arrival.cpu()
    assert torch.isnan(table[0]).all() and sorted(ref.arrival) == [1, 2] and len(seen) == 2
    for t, args in zip((1, 2), seen):
        im, ds, gt_im, gt_depth = (x.cpu() for x in args[:4])
        assert torch.equal(gt_im, rawcap.lit[t]["im"].cpu())
        lit = real(im, ds, gt_im, gt_depth, 0.5, ms_ssim=False).numpy().astype(np.float64)  # (CPU tensors)
        rst = er.frame_metrics(im.numpy(), ds.numpy(), gt_im.numpy(), gt_depth.numpy(), 0.5, False, False)
        own = np.abs(lit - rst) / np.abs(rst)  # the literal's own distance from the restatement
        tge._check(table[t], lit, f"arrival {t} vs literal", extra=np.nan_to_num(own))
        assert float(table[t, 4]) == lit[4] == float((rawcap.lit[t]["depth"] > 0).sum()) and np.isnan(lit[1])
        assert torch.isnan(table[t, 1])


@pytest.fixture(scope="module")
def online_capture(cuda):
    """tests/test_gpu_online.py's scene, three frames, quantised."""
    from splatam_amd.scenes import make_scene
    from splatam_amd.tracker import probe_num_rendered
    from splatam_amd.workloads import sequence_workload
    dev = torch.device(cuda)
    cap = sequence_workload(make_scene(20_000, 320, 240, seed=7), N_RAW, dev)
    params, frames, cam, w2c, _, _ = cap
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
    return cap, 4 * n + 400_000, [_quantise(f, dev) for f in frames]


def test_raw_sequence_tracked(cuda, online_capture):
    from splatam_amd.sequence import SlamSequence
    (params, _, cam, w2c, intr, _), bin_cap, raw = online_capture
    kw = dict(dict(KW, tracking_iters=10, track_replay=10, track_size=(120, 160), densify_size=(120, 160)),
              capacity=params["means3D"].shape[0] + 2 * 320 * 240, bin_capacity=bin_cap, seed=0, num_frames=N_RAW,
              densify_mode="device")
    seq = SlamSequence(params, [{"rgb_u8": raw[0][0], "depth_u16": raw[0][1]}], cam, w2c, intr, **kw)
    seq.frame(0)
    for t in range(1, N_RAW):
        assert seq.push_raw(*raw[t]) == t
    lit = [ig.ingest_literal(r, d, PNG_SCALE, MAX_DEPTH) for r, d in raw]
    fed = SlamSequence(params, lit[:1], cam, w2c, intr, **kw)
    fed.frame(0)
    for f in lit[1:]:
        fed.push(f["im"], f["depth"])
    seq.check(), fed.check()
    torch.cuda.synchronize()
    _same_sequences(seq, fed)
    assert seq.tracking_iters_run == [0, 10, 10] and seq.slot_curr["im"].shape == (3, 120, 160)
    assert not torch.equal(seq.params["cam_trans"][..., 1], seq.params["cam_trans"][..., 0])  # (it was tracked)
