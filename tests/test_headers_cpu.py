"""The shared headers of splatam_amd/csrc stand alone, and the one Adam coefficient fill is the old fill.

Needs hipcc and no GPU (skipped without hipcc).  Every csrc/*.h compiles on its own with the library's flags;
gsr_common.h, which the headers were cut from, is gone; the files that launch no render kernel do not reach
gsr_launch.h (read from the preprocessor's dependency output, not from the source text); and adam_coef
(csrc/gsr_adam.h), called from a stand-alone host program, returns bit for bit the five floats the three fills
it replaced computed.
"""
import glob
import math
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from splatam_amd import build

CSRC = build.CSRC
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h")))
NO_LAUNCHERS = ["gsr_seq_common.h", "gsr_eval.hip", "gsr_keyframe.hip", "gsr_densify.hip", "gsr_viewgain.hip"]


@pytest.fixture(scope="module")
def hipcc():
    try:
        return build.hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True)


def test_every_header_compiles_alone(hipcc):
    assert len(HEADERS) >= 10, HEADERS
    with ThreadPoolExecutor(max_workers=min(16, len(HEADERS))) as ex:
        done = list(ex.map(lambda h: _run([hipcc, *build.flags(), "-x", "hip", "-fsyntax-only", h]), HEADERS))
    bad = {os.path.basename(h): r.stderr[-2000:] for h, r in zip(HEADERS, done) if r.returncode != 0}
    assert not bad, bad


def test_gsr_common_is_gone():
    assert not os.path.exists(os.path.join(CSRC, "gsr_common.h"))


@pytest.mark.parametrize("name", NO_LAUNCHERS)
def test_does_not_reach_the_launchers(hipcc, name):
    r = _run([hipcc, *build.flags(), "-x", "hip", "-M", os.path.join(CSRC, name)])
    assert r.returncode == 0, r.stderr[-2000:]
    deps = {os.path.basename(d) for d in r.stdout.replace("\\\n", " ").split()}
    assert "gsr_layout.h" in deps or "gsr_wave.h" in deps, deps  # (the output does list the csrc headers)
    assert "gsr_launch.h" not in deps


ADAM_MAIN = r"""
#include <stdio.h>

#include "gsr_adam.h"

int main() {
    const double eps[2] = {1e-8, 1e-15};
    const int steps[5] = {1, 2, 59, 1000, 1000000};
    for (int e = 0; e < 2; e++)
        for (int s = 0; s < 5; s++) {
            const gsr::AdamCoef c = gsr::adam_coef(0.9, 0.999, eps[e], steps[s]);
            printf("%d %d %a %a %a %a %a\n", e, steps[s], c.w1, c.beta2, c.omb2, c.bc2_sqrt, c.eps);
        }
    return 0;
}
"""


def test_adam_coef_is_the_replaced_fills(hipcc, tmp_path):
    """The fills adam_coef replaced, in the parent commit: fill_adam_common (gsr_mapping.hip:589-596, called
    from gsr_map_transform_bwd_adam at :707 and from gsr_adam_step at :753) and the hand-written one of
    gsr_backward_dual_sh_adam (gsr_capi.hip:1225-1229).  All three computed, in double, 1 - beta1, beta2,
    1 - beta2, sqrt(1 - pow(beta2, step)) and eps, each rounded to float; Python's float ** is the same libm
    pow() call, so the comparison is bitwise."""
    src, exe = tmp_path / "adam_coef_main.hip", tmp_path / "adam_coef_main"
    src.write_text(ADAM_MAIN)
    r = _run([hipcc, *build.flags(), "--cuda-host-only", str(src), "-o", str(exe)])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run([str(exe)])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert [(int(w[0]), int(w[1])) for w in rows] == [(e, s) for e in (0, 1) for s in (1, 2, 59, 1000, 1000000)]
    beta1, beta2 = 0.9, 0.999
    for w in rows:
        eps, step = (1e-8, 1e-15)[int(w[0])], int(w[1])
        got = np.array([float.fromhex(x) for x in w[2:]], dtype=np.float64)
        assert (got == got.astype(np.float32)).all(), w  # (floats, printed exactly)
        want = np.array([1 - beta1, beta2, 1 - beta2, math.sqrt(1 - beta2 ** step), eps]).astype(np.float32)
        assert got.astype(np.float32).tobytes() == want.tobytes(), (w, want)
