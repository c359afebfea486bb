"""The shared headers of splatam_amd/csrc stand alone, and the one Adam coefficient fill is the old fill.

Needs hipcc and no GPU (skipped without hipcc).  Every csrc/*.h compiles on its own with the library's flags;
gsr_common.h, which the headers were cut from, is gone; the files that launch no render kernel do not reach
gsr_launch.h (read from the preprocessor's dependency output, not from the source text); and adam_coef
(csrc/gsr_adam.h), called from a stand-alone host program, returns bit for bit the five floats the three fills
it replaced computed; and rec_sums (csrc/gsr_launch.h), likewise from a host program, gives the instance record
layouts the three statements it replaced gave.  Two tests read the source text alone (no hipcc): gsr_launch.h's
file banners name the file that defines each launcher below them, and every declared launcher has a caller.
"""
import glob
import math
import os
import re
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


_BANNER = re.compile(r"^// -+ (gsr_\w+\.hip) --$")
_LAUNCHER = re.compile(r"^hipError_t (launch_\w+)\(")


def _declared_launchers():
    """[(launcher, the file whose banner it stands under)] of gsr_launch.h, in order."""
    out, home = [], None
    for ln in open(os.path.join(CSRC, "gsr_launch.h")).read().splitlines():
        if m := _BANNER.match(ln):
            home = m.group(1)
        elif m := _LAUNCHER.match(ln):
            out.append((m.group(1), home))
    return out


def _defined_launchers(path):
    """The launchers a source defines: a definition starts its line with the return type, a call does not."""
    return {m.group(1) for ln in open(path).read().splitlines() if (m := _LAUNCHER.match(ln))}


def test_launch_header_names_each_launchers_file():
    """gsr_launch.h groups its declarations under one banner per defining file: every launch_* declared under a
    banner is defined in the file the banner names, and every named file is compiled: a translation unit of
    build.SOURCES, or one of build.FORWARD_STAGES, which the unit gsr_forward_unit.hip (in SOURCES) includes, all
    of them and nothing else, in that order.
    Works on the source text (no compiler): cheap, and the banners are comments, which only text can check."""
    decl = _declared_launchers()
    assert len(decl) >= 30 and all(home for _, home in decl), decl
    files = sorted({home for _, home in decl})
    unit = open(os.path.join(CSRC, "gsr_forward_unit.hip")).read()
    code = [ln for ln in unit.splitlines() if ln.strip() and not ln.startswith("//")]
    assert "gsr_forward_unit.hip" in build.SOURCES and code == [f'#include "{s}"' for s in build.FORWARD_STAGES], code
    compiled = set(build.SOURCES) | set(build.FORWARD_STAGES)
    assert set(files) <= compiled, sorted(set(files) - compiled)
    defined = {f: _defined_launchers(os.path.join(CSRC, f)) for f in files}
    misplaced = [(name, home) for name, home in decl if name not in defined[home]]
    assert not misplaced, misplaced


def test_no_launcher_is_dead():
    """Every launch_* that gsr_launch.h declares occurs, as a whole word, somewhere in csrc/*.hip or *.cpp other
    than on the line that defines it and outside `//` comments (the sources have no block comments naming a
    launcher): a launcher nobody calls (and its kernel) is deleted, not kept.  Source text only, like the test
    above."""
    lines = [ln.split("//")[0]
             for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))
             for ln in open(p).read().splitlines()]
    dead = [name for name, _ in _declared_launchers()
            if not any(re.search(rf"\b{name}\b", ln) for ln in lines if not ln.startswith(f"hipError_t {name}("))]
    assert not dead, dead


LAYOUT_MAIN = r"""
#include <stdio.h>

#include "gsr_render_bwd.h"

using namespace gsr;
// NV, RS and bytes of the parent's positional BwdShape instantiations (printed by a one-off program compiled
// against the parent's gsr_backward.hip)
#define SHAPE_IS(V, nv, rs, by) \
    static_assert(BwdShape<V>::NV == nv && BwdShape<V>::RS == rs && BwdShape<V>::bytes == by, #V)
SHAPE_IS(TrackVariant, 6, 6, 28064);       // BwdShape<true, false, false, true, 1, 0>
SHAPE_IS(MapM2dVariant, 12, 12, 34224);    // BwdShape<true, true, true, true, 1, 0, 3, true>
SHAPE_IS(MomVariant<1>, 16, 16, 32192);    // BwdShape<false, true, true, false, 3, 1>
SHAPE_IS(MomVariant<2>, 34, 34, 33296);    // BwdShape<false, true, true, false, 3, 2>
using Full1 = BwdVariant<false, true, true, false>;
using Col1 = BwdVariant<false, false, true, false>;
SHAPE_IS(Full1, 9, 10, 29616);             // BwdShape<false, true, true, false, 3, 0>
SHAPE_IS(OneColour<Full1>, 7, 10, 26528);  // BwdShape<false, true, true, false, 3, 0, 1>
SHAPE_IS(OneColour<Col1>, 6, 8, 24992);    // BwdShape<false, false, true, false, 3, 0, 1>

static void row(const char* tag, int a, int b, const RecSums& s) {
    printf("%s %d %d %d %d %d %d %d %d %d\n", tag, a, b, s.rec.stride, s.rec.o_op, s.rec.o_c1, s.rec.o_c2, s.rec.n_c2,
           s.o_m1, s.nv);
}
int main() {
    for (int dual = 0; dual < 2; dual++)
        for (unsigned need = 0; need < 16; need++)  // launch_render_bwd's decoding of (need, dual): bwd_terms()
            row("rec", dual, (int)need,
                rec_sums((need & NEED_OPACITY) != 0, (need & NEED_COLORS) != 0, dual && (need & NEED_COLORS2),
                         (dual && (need & NEED_DL2_CH0_ONLY)) ? 1 : 3));
    row("m2d", 1, 0, bwd_sums<MapM2dVariant>());
    printf("const %d %d\n", M2D_REC_PAIR, INST_REC_MAX);
    return 0;
}
"""

# (dual, need) -> (stride, o_op, o_c1, o_c2, n_c2, sums): the parent's bwd_rec_layout arithmetic -- five geometric
# sums, then the opacity sum (+1), the colour sums (+3) and the second colour set's (+q2, with a second image
# only; q2 = 1 under NEED_DL2_CH0_ONLY); absent terms -1; the stride is the count rounded up to even.
# need: NEED_OPACITY 1, NEED_COLORS 2, NEED_COLORS2 4, NEED_DL2_CH0_ONLY 8.
REC_LAYOUTS = {
    (0, 0): (6, -1, -1, -1, 0, 5), (0, 1): (6, 5, -1, -1, 0, 6), (0, 2): (8, -1, 5, -1, 0, 8),
    (0, 3): (10, 5, 6, -1, 0, 9), (0, 4): (6, -1, -1, -1, 0, 5), (0, 5): (6, 5, -1, -1, 0, 6),
    (0, 6): (8, -1, 5, -1, 0, 8), (0, 7): (10, 5, 6, -1, 0, 9), (0, 8): (6, -1, -1, -1, 0, 5),
    (0, 9): (6, 5, -1, -1, 0, 6), (0, 10): (8, -1, 5, -1, 0, 8), (0, 11): (10, 5, 6, -1, 0, 9),
    (0, 12): (6, -1, -1, -1, 0, 5), (0, 13): (6, 5, -1, -1, 0, 6), (0, 14): (8, -1, 5, -1, 0, 8),
    (0, 15): (10, 5, 6, -1, 0, 9),
    (1, 0): (6, -1, -1, -1, 0, 5), (1, 1): (6, 5, -1, -1, 0, 6), (1, 2): (8, -1, 5, -1, 0, 8),
    (1, 3): (10, 5, 6, -1, 0, 9), (1, 4): (8, -1, -1, 5, 3, 8), (1, 5): (10, 5, -1, 6, 3, 9),
    (1, 6): (12, -1, 5, 8, 3, 11), (1, 7): (12, 5, 6, 9, 3, 12), (1, 8): (6, -1, -1, -1, 0, 5),
    (1, 9): (6, 5, -1, -1, 0, 6), (1, 10): (8, -1, 5, -1, 0, 8), (1, 11): (10, 5, 6, -1, 0, 9),
    (1, 12): (6, -1, -1, 5, 1, 6), (1, 13): (8, 5, -1, 6, 1, 7), (1, 14): (10, -1, 5, 8, 1, 9),
    (1, 15): (10, 5, 6, 9, 1, 10),
}
M2D_LAYOUT = (12, 5, 6, 9, 1, 10, 12)  # the mapping record (1, 15), then the pair at 10: stride 12


def test_record_layout_is_the_parents(hipcc, tmp_path):
    """rec_sums (csrc/gsr_launch.h), the one statement of the instance record's layout, gives for every
    (need, dual) launch_render_bwd accepts and for the M2D form what the three statements it replaced gave
    (bwd_nv, bwd_tile's O_C1 / NA / NB and bwd_rec_layout's run-time arithmetic, all in the parent's
    gsr_backward.hip), and BwdShape of every named variant keeps its sums, record stride and LDS bytes (the
    program's static_asserts)."""
    src, exe = tmp_path / "layout_main.hip", tmp_path / "layout_main"
    src.write_text(LAYOUT_MAIN)
    r = _run([hipcc, *build.flags(), "--cuda-host-only", str(src), "-o", str(exe)])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run([str(exe)])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    rec = {(int(w[1]), int(w[2])): tuple(int(x) for x in w[3:]) for w in rows if w[0] == "rec"}
    assert set(rec) == set(REC_LAYOUTS)
    for key, (stride, o_op, o_c1, o_c2, n_c2, nv) in REC_LAYOUTS.items():
        assert rec[key] == (stride, o_op, o_c1, o_c2, n_c2, -1, nv), key
    m2d = [tuple(int(x) for x in w[3:]) for w in rows if w[0] == "m2d"]
    assert m2d == [M2D_LAYOUT]
    assert [w[1:] for w in rows if w[0] == "const"] == [["10", "12"]]
    assert max(v[0] for v in REC_LAYOUTS.values()) == M2D_LAYOUT[0] == 12


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
