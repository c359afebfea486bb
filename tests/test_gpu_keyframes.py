"""The overlap keyframe selection on the device (gsr_keyframe_select through splatam_amd.keyframes.select_device)
against the float64 numpy restatement of tests/keyframe_ref.py, its workspace contract, its replay from a
captured graph (no host read), the mapper's replay from device-resident draws, and the SLAM sequence under
keyframe_policy="overlap" against the per-frame loop that runs select_literal on the same random words.

The overlap band: a sample is borderline for a keyframe when its float64 u, v or z lies within delta of a
bound, delta derived from the float32 operation chain (keyframe_ref's module docstring); overlap[k] must lie
in [sure_k, sure_k + borderline_k].  The cases are valid inputs by the restatement alone (make_valid_case: at
most 1 % borderline samples per keyframe, no eligibility resting on one); everything else is exact."""
import numpy as np
import pytest
import torch

import keyframe_ref as kr
from splatam_amd import keyframes as kfm

pytestmark = pytest.mark.gpu

ZERO_ROWS = (0, 30, -1)  # the first row, a middle one and the last one are entirely zero
_CASES = {}


def _case(W, H, S, n_kf):
    key = (W, H, S, n_kf)
    if key not in _CASES:
        _CASES[key] = kr.make_valid_case(W, H, S, n_kf, seed=W + 7 * S + n_kf, zero_rows=ZERO_ROWS)
    return _CASES[key]


@pytest.mark.parametrize("n_kf", [0, 1, 2, 9, 300])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 1600])
@pytest.mark.parametrize("W,H", [(96, 64), (100, 75), (320, 240)])
def test_kernel_matches_restatement(cuda, W, H, S, n_kf):
    c, ref = _case(W, H, S, n_kf)
    out = kfm.select_device(*kr.to_torch(c, cuda), pixels=True)
    torch.cuda.synchronize()
    print(f"{W}x{H} S={S} n_kf={n_kf}: n_points {int(out['n_points'])}, eligible {ref['n_eligible']}, "
          f"borderline max {int(ref['borderline'].max(initial=0))}")
    kr.check(out, ref)


@pytest.mark.parametrize("W,H", [(64, 300), (64, 600)])
def test_row_scan_with_several_rows_per_thread(cuda, W, H):
    """More than 256 rows: the last workgroup's scan gives a thread two rows (H = 300, threads 150 .. 255 none)
    or three (H = 600, threads 200 .. 255 none).  The seed was picked with the restatement alone, so that the
    window is not trivial: a wrong row prefix moves the sampled pixels, and with them every other output."""
    c = kr.make_case(W, H, 65, 9, seed=1, zero_rows=ZERO_ROWS)
    ref = kr.restate(c)
    assert ref["n_points"] > 0 and (ref["sure"] > 0).any() and ref["borderline"].max() == 0
    out = kfm.select_device(*kr.to_torch(c, cuda), pixels=True)
    torch.cuda.synchronize()
    print(f"{W}x{H}: n_points {int(out['n_points'])}, eligible {ref['n_eligible']}, overlap {out['overlap'].tolist()}")
    kr.check(out, ref)
    assert torch.equal(out["overlap"].cpu().to(torch.int64), torch.from_numpy(ref["sure"]))  # (no borderline sample)


@pytest.mark.parametrize("W,H,S,n_kf", [(100, 75, 65, 9), (320, 240, 1600, 300)])
def test_kernel_equals_literal_bits(cuda, W, H, S, n_kf):
    """select_literal's elementwise float32 ops (here on CPU tensors) and the kernels form the same bits: every
    output equal, the overlap counts included."""
    c, _ = _case(W, H, S, n_kf)
    out = kfm.select_device(*kr.to_torch(c, cuda), pixels=True)
    lit = kfm.select_literal(*kr.to_torch(c, "cpu"))
    for k in ("overlap", "n_points", "window", "n_window", "draw_rows", "draw_times", "pixels"):
        assert torch.equal(out[k].cpu(), lit[k]), k


def test_workspace_reuse(cuda):
    """Two different calls back to back on one zero-filled workspace, into sentinel-filled outputs: both
    correct, the counter words zero afterwards."""
    (ca, ra), (cb, rb) = _case(320, 240, 1600, 9), _case(100, 75, 65, 300)
    ws = kfm.make_workspace(240, 1600, cuda)
    outs = []
    for c in (ca, cb, ca):
        o = kfm._outputs(c["n_kf"], c["k_select"], len(c["u_pix"]), len(c["u_draw"]), cuda, True)
        for v in o.values():
            v.fill_(-7777)
        outs.append(kfm.select_device(*kr.to_torch(c, cuda), workspace=ws, out=o))
    torch.cuda.synchronize()
    for o, r in zip(outs, (ra, rb, ra)):
        kr.check(o, r)
    assert int(ws[:16].abs().sum()) == 0


def test_graph_replay_without_host_read(cuda):
    """The selection captured on one stream as a linear chain, replayed after the depth, the poses and the
    random words changed in place: equal to the eager result on the new values."""
    (ca, _), (cb, rb) = _case(100, 75, 65, 9), kr.make_valid_case(100, 75, 65, 9, seed=4242, zero_rows=(3,))
    args = list(kr.to_torch(ca, cuda))
    ws = kfm.make_workspace(75, 65, cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        out = kfm.select_device(*args, workspace=ws, pixels=True)  # (warm-up; the outputs are reused below)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        kfm.select_device(*args, workspace=ws, out=out)
    new = kr.to_torch(cb, cuda)
    assert new[4:6] == tuple(args[4:6]) and new[10:] == tuple(args[10:])  # the host-known sizes are the graph's
    for i in (0, 2, 3, 6, 7, 8, 9):
        args[i].copy_(new[i])
    for v in out.values():
        v.fill_(-7777)
    graph.replay()
    torch.cuda.synchronize()
    kr.check(out, rb)
    eager = kfm.select_device(*new, pixels=True)
    for k, v in eager.items():
        assert torch.equal(v, out[k]), k


# ------------------------------------------------------------------ mapper / sequence

@pytest.fixture(scope="module")
def capture(cuda):
    from splatam_amd.scenes import make_scene
    from splatam_amd.workloads import sequence_workload
    return sequence_workload(make_scene(20_000, 320, 240, seed=7), 5, torch.device(cuda))


def test_mapper_device_sequence_equals_host_sequence(cuda, capture):
    from splatam_amd.mapper import GAUSS_KEYS, GraphMapper
    params, frames, cam, w2c, _, _ = capture
    keys = GAUSS_KEYS + ("rgb_colors",)
    kfs = [{"cam": cam, "w2c": w2c, "im": frames[t]["im"], "depth": frames[t]["depth"], "id": t} for t in range(4)]
    bank = kfm.KeyframeBank(frames[0]["im"].shape, frames[0]["depth"].shape, cuda, capacity=2)
    for t in range(3):  # (the third append doubles the bank)
        bank.append(frames[t]["im"], frames[t]["depth"], params, t)
    bank.set_current(frames[3]["im"], frames[3]["depth"])
    assert bank.n == 3 and bank.cap == 4 and bank.time[:3].tolist() == [0, 1, 2]
    from splatam_amd.tracker import probe_num_rendered
    bin_cap = 4 * probe_num_rendered(params, kfs[0], 0)[0] + 400_000
    seq = [2, 0, 3, 1, 3, 0]
    rows =torch.tensor([r if r < 3 else bank.cur_row for r in seq], dtype=torch.int64, device=cuda)
    times = torch.tensor(seq, dtype=torch.int64, device=cuda)
    got = []
    for device in (False, True):
        p = {k: (v.detach().clone().requires_grad_(True) if k in keys else v.detach().clone())
             for k, v in params.items()}
        m = GraphMapper(p, kfs[:1], iters_per_graph=6, seed=0, prune=False, capacity=bin_cap)
        if device:
            m.set_keyframe_bank(bank.im, bank.depth)
            m.run(device_sequence=(rows, times))
        else:
            m.set_keyframes(kfs)
            m.run(sequence=seq)
        torch.cuda.synchronize()
        got.append({k: p[k].detach().clone() for k in keys})
    assert not torch.equal(got[0]["means3D"], params["means3D"])  # the frame was mapped
    for k in keys:
        assert torch.equal(got[0][k], got[1][k]), k


def test_overlap_sequence_equals_per_frame_loop(cuda, capture):
    from splatam_amd.mapper import GAUSS_KEYS
    from splatam_amd.sequence import PerFrameSlam, SlamSequence
    from splatam_amd.tracker import probe_num_rendered
    params, frames, cam, w2c, intr, _ = capture
    n, _ = probe_num_rendered(params, {"cam": cam, "w2c": w2c, "im": frames[0]["im"], "depth": frames[0]["depth"]}, 0)
    bin_cap = 4 * n + 400_000
    kw = dict(tracking_iters=20, mapping_iters=10, window=3, keyframe_every=1, keyframe_policy="overlap")
    seq = SlamSequence(params, frames, cam, w2c, intr, capacity=params["means3D"].shape[0] + 2 * 320 * 240,
                       bin_capacity=bin_cap, seed=0, **kw)
    for t in range(5):
        seq.frame(t)
    seq.check()
    ref = PerFrameSlam(params, frames, cam, w2c, intr, bin_capacity=bin_cap, **kw)
    for t in range(5):
        ref.frame(t, seq.draws[t])
    torch.cuda.synchronize()
    # the windows (time indices): the same in both forms, and not the last-K window in every frame
    wins = []
    for t, sel in enumerate(seq.selections):
        rows = sel["window"][:int(sel["n_window"])].tolist()
        wins.append([t if r == seq.bank.cur_row else seq.bank.times[r] for r in rows])
    print("windows", wins)
    assert wins == ref.windows
    assert seq.bank.times == [0, 1, 2, 3, 4]
    assert any(w != list(range(max(0, t - 2), t + 1)) for t, w in enumerate(wins))
    live = seq.live_params()
    assert torch.equal(seq.params["cam_unnorm_rots"], ref.p["cam_unnorm_rots"])
    assert torch.equal(seq.params["cam_trans"], ref.p["cam_trans"])
    for k in GAUSS_KEYS + ("rgb_colors",):
        assert torch.equal(live[k], ref.p[k]), k
