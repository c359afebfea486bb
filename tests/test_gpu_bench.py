"""The plain bench run (bench.py --gpus 1 --steps N --warmup W): exactly N timed steps, the headline fields,
none of the --full legs, and --dump-outputs' arrays of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dump_outputs(cuda, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    b = lines[0]
    assert b["unit"] == "frames/s" and b["higher_is_better"] is True and b["dtype"] == "f32" and b["n_gpus"] == 1
    assert b["steps"] == 20 and b["roofline"]["launches_timed"] == 20  # --steps sets the timed steps
    assert b["ms_per_step"] > 0 and abs(b["value"] - 1e3 / b["ms_per_step"]) <= 0.01 * b["value"]
    # a plain run measures the headline only: every other leg is --full's
    for leg in ("cpu_baseline", "dropin", "fisher", "mapping", "sequence", "configs", "broadcast"):
        assert b[leg] is None, leg
    assert "unfused" not in b["roofline"] and "timed replays" in b["stages_source"]
    arrs = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrs) == {"cam_unnorm_rots", "cam_trans", "loss", "best_candidate", "pose_adam_state"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64e6
    # the frame's pose column holds the best candidate the last timed frame wrote back
    best = arrs["best_candidate"]
    assert np.array_equal(arrs["cam_unnorm_rots"][0, :, 0], best[1:5])
    assert np.array_equal(arrs["cam_trans"][0, :, 0], best[5:8])
    assert 0 < best[0] <= 1e20 and arrs["loss"] > 0 and np.abs(arrs["pose_adam_state"]).sum() > 0
