"""Device-code identity check for a refactor of the kernels: python tools/device_asm_diff.py REV

Compiles every translation unit of build.SOURCES from the working tree and from git revision REV with the
library's own flags plus --cuda-device-only -S, drops the lines naming the per-compilation __hip_cuid_ symbol,
and compares the two texts function by function: a function's body and, for a kernel, its .amdhsa_kernel
descriptor block (registers, LDS, scratch, kernarg size).  Labels carry the function's index in its file
(.LBB<i>_<n>, .Lfunc_end<i>, `BB<i>_<n>` in the loop comments), which moves when a function is added ahead of it, so the index is dropped before
comparing.  Prints per file `identical` or the functions whose text differs, and the functions only one side has
(`added` / `removed`); exits non-zero when a function both sides have differs or one was removed.  With functions
added, the text outside any function (the metadata listing every kernel) differs by construction and is not
compared; without, it is.  Needs hipcc, no GPU.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatam_amd import build  # noqa: E402


def device_asm(src, csrc, include, out):
    cmd = [build.hipcc(), *build.flags(csrc, include), "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    return [ln for ln in open(out).read().splitlines() if "__hip_cuid_" not in ln]


_LABEL = re.compile(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\.LJTI|\.LCPI|\bBB)\d+(?=_\d|\b)")


def functions(lines):
    """{function name: its lines} (a body runs from its .type directive to .Lfunc_end, plus a kernel's
    .amdhsa_kernel block), function indices dropped from the labels; the rest under ''."""
    out, cur = {"": []}, ""
    for ln in lines:
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", ln) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
        # (the label's width sets the padding ahead of its comment: one space)
        out.setdefault(cur, []).append(re.sub(r"\s+;", " ;", _LABEL.sub(r"\1", ln)) if cur else ln)
        if ln.startswith(".Lfunc_end") or ln.strip() == ".end_amdhsa_kernel":
            cur = ""
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    work = tempfile.mkdtemp(prefix="gsr_asm_")
    try:
        trees = {"new": (build.CSRC, build.INCLUDE), "old": build.export_rev(rev, work)}
        jobs = [(src, side) for src in build.SOURCES for side in trees]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            asm = dict(zip(jobs, ex.map(
                lambda j: device_asm(j[0], *trees[j[1]], os.path.join(work, f"{j[1]}_{j[0]}.s")), jobs)))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    bad = 0
    for src in build.SOURCES:
        old, new = functions(asm[src, "old"]), functions(asm[src, "new"])
        added, removed = sorted(new.keys() - old.keys()), sorted(old.keys() - new.keys())
        both = [f for f in old.keys() & new.keys() if f or not (added or removed)]
        diff = sorted(f or "(outside any function)" for f in both if old[f] != new[f])
        bad += bool(diff or removed)
        text = "differs in " + ", ".join(diff) if diff else f"identical ({len(both)} functions)"
        for what, names in (("added", added), ("removed", removed)):
            if names:
                text += f"; {what}: " + ", ".join(names)
        print(f"{src}: {text}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
