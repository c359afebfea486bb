"""Device-code identity check for a refactor of the kernels: python tools/device_asm_diff.py REV

Compiles every translation unit of build.SOURCES from the working tree and from git revision REV with the
library's own flags plus --cuda-device-only -S, drops the lines naming the per-compilation __hip_cuid_ symbol,
and compares the two texts function by function: a function's body and, for a kernel, its .amdhsa_kernel
descriptor block (registers, LDS, scratch, kernarg size).  Labels carry the function's index in its file
(.LBB<i>_<n>, .Lfunc_end<i>, `BB<i>_<n>` in the loop comments), which moves when a function is added ahead of it, so the index is dropped before
comparing.  Prints per file `identical` or the functions whose text differs, and the functions only one side has
(`added` / `removed`); a function one file lost and another file gained is looked up by name across all files of
the other side and printed under its new file as `moved from X to Y: identical` or `differs`.  Exits non-zero when
a function both sides have differs, in place or moved, or one was removed.  With functions added, removed or moved,
the file's text outside any function (the metadata listing every kernel) differs by construction and is not
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
    funcs = {(src, side): functions(asm[src, side]) for src in build.SOURCES for side in trees}
    # a function one file lost and another gained has moved: looked up by name across the other side's files
    home = {side: {f: src for src in build.SOURCES for f in funcs[src, side] if f} for side in trees}
    bad = 0
    for src in build.SOURCES:
        old, new = funcs[src, "old"], funcs[src, "new"]
        gained, lost = sorted(new.keys() - old.keys()), sorted(old.keys() - new.keys())
        moved_in = [f for f in gained if home["old"].get(f, src) != src]
        moved_out = [f for f in lost if home["new"].get(f, src) != src]
        added, removed = sorted(set(gained) - set(moved_in)), sorted(set(lost) - set(moved_out))
        both = [f for f in old.keys() & new.keys() if f or not (gained or lost)]
        diff = sorted(f or "(outside any function)" for f in both if old[f] != new[f])
        bad += bool(diff or removed)
        text = "differs in " + ", ".join(diff) if diff else f"identical ({len(both)} functions)"
        for what, names in (("added", added), ("removed", removed)):
            if names:
                text += f"; {what}: " + ", ".join(names)
        print(f"{src}: {text}")
        for f in moved_in:
            same = funcs[home["old"][f], "old"][f] == new[f]
            bad += not same
            print(f"  {f} moved from {home['old'][f]} to {src}: {'identical' if same else 'differs'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
