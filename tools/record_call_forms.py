"""Record tests/golden/py_call_forms.json: the libgsr.so calls every Python wrapper form makes, as
tests/test_gpu_call_forms.py notes them (its CASES through its recorder).  Run it at the commit whose call forms are
the reference -- a refactor of the binding layer must then pass the test without running this again.

    python tools/record_call_forms.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import pytest
    import torch

    import test_gpu_call_forms as cf
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=cf.GOLDEN)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for name in sorted(cf.CASES):
        with pytest.MonkeyPatch.context() as mp:
            out[name] = cf.record(name, dev, mp)
        print(f"{name}: {len(out[name])} calls")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        cases = [f" {json.dumps(k)}: [\n" + ",\n".join("  " + json.dumps(c, sort_keys=True) for c in out[k]) + "\n ]"
                 for k in sorted(out)]  # one call per line
        f.write("{\n" + ",\n".join(cases) + "\n}\n")


if __name__ == "__main__":
    main()
