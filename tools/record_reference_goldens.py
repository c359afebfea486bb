"""Records tests/golden/ref_raster/<case>.npz from the reference's own kernels on the GPU
(oracle/reference.py; needs oracle/_ref/libref_raster.so and a GPU, run once):

    python tools/record_reference_goldens.py [--out DIR]

For every case of tests/reference_cases.GOLDEN_CASES: the inputs, the reference's colour, depth image,
radii, tiles_touched, n_contrib, final T, ranges and point_list, and per power (1 and 2, random-sign seed)
every gradient tensor of one backward run plus the relative L2 spread between two runs (its float atomics
make the backward non-deterministic).  tests/test_reference_goldens_cpu.py compares both oracle builds
with these files on machines that have neither the library nor a GPU.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import reference_cases as rc  # noqa: E402
from oracle import harness, reference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ref_raster"))
    a = ap.parse_args()
    if not reference.available():
        sys.exit("reference library: " + reference.why_unavailable())
    os.makedirs(a.out, exist_ok=True)
    for name in rc.GOLDEN_CASES:
        case = rc.BY_NAME[name]
        scene, kw = case.scene(), case.kwargs()
        fr, _ = harness.run_reference(scene, backward=False, **kw)
        rec = rc.scene_inputs(scene, kw)
        rec.update({k: v for k, v in rc.frame_dict(fr).items()})
        for power, seed in sorted({(p, s) for n, p, s in rc.GOLDEN_RUNS if n == name}):
            d = rc.dpix(scene, seed)
            runs = [reference.backward(fr, d, power=power) for _ in range(2)]
            rec[f"dpix_p{power}"] = d
            for k in harness.GRAD_KEYS:
                rec[f"g_p{power}_{k}"] = runs[0][k]
                rec[f"spread_p{power}_{k}"] = np.float64(harness.rel_l2(runs[1][k], runs[0][k]))
        path = os.path.join(a.out, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: num_rendered {fr.num_rendered}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
