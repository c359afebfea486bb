"""Device-code identity check for a refactor of the kernels:
    python tools/device_asm_diff.py REV [--removed NAME ...]

Compiles the translation units of the working tree (build.SOURCES) and those of git revision REV (the SOURCES
of its own build.py) with the library's own flags plus --cuda-device-only -S, drops the lines naming the
per-compilation __hip_cuid_ symbol, and compares the two texts function by function: a function's body and,
for a kernel, its .amdhsa_kernel descriptor block (registers, LDS, scratch, kernarg size).  A source only one
side has -- a file the change adds, deletes or renames -- contributes no functions on the other, so a split or
a merge shows as functions that moved.

Labels carry the function's index in its file (.LBB<i>_<n>, .Lfunc_end<i>, `BB<i>_<n>` in the loop comments),
which moves when a function is added ahead of it, so the index is dropped before comparing.

Prints per file `identical` or the functions whose text differs, and the functions only one side has (`added` /
`removed`).  A function one file lost and another gained is looked up by name across all files of the other
side and printed under its new file as `moved from X to Y: identical` or `differs`.  --removed names the
functions (mangled) the change deletes on purpose; each is printed as `removed: NAME (expected)`.

Exits non-zero when a function both sides have differs, in place or moved; when one was removed that --removed
does not name; or when a --removed name was not removed (mistyped, or still there).  With functions added,
removed or moved, a file's text outside any function (the metadata listing every kernel) differs by
construction and is not compared; without, it is.  Needs hipcc, no GPU.
"""
import argparse
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("--removed", nargs="*", default=[], metavar="NAME",
                    help="functions (mangled names) the change removes on purpose")
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="gsr_asm_")
    try:
        trees = {"new": (build.CSRC, build.INCLUDE), "old": build.export_rev(args.rev, work)}
        mine = {"new": build.SOURCES, "old": build.rev_sources(args.rev)}
        sources = build.SOURCES + [s for s in mine["old"] if s not in build.SOURCES]
        # a source one side does not have contributes no functions there
        jobs = [(src, side) for src in sources for side in trees if src in mine[side]]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            asm = dict(zip(jobs, ex.map(
                lambda j: device_asm(j[0], *trees[j[1]], os.path.join(work, f"{j[1]}_{j[0]}.s")), jobs)))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    funcs = {(src, side): functions(asm[src, side]) if (src, side) in asm else {} for src in sources for side in trees}
    # a function one file lost and another gained has moved: looked up by name across the other side's files
    home = {side: {f: src for src in sources for f in funcs[src, side] if f} for side in trees}
    expected, bad, gone = set(args.removed), 0, set()
    for src in sources:
        old, new = funcs[src, "old"], funcs[src, "new"]
        gained, lost = sorted(new.keys() - old.keys() - {""}), sorted(old.keys() - new.keys() - {""})
        moved_in = [f for f in gained if home["old"].get(f, src) != src]
        moved_out = [f for f in lost if home["new"].get(f, src) != src]
        added, removed = sorted(set(gained) - set(moved_in)), sorted(set(lost) - set(moved_out))
        both = [f for f in old.keys() & new.keys() if f or not (gained or lost)]
        diff = sorted(f or "(outside any function)" for f in both if old[f] != new[f])
        bad += bool(diff or set(removed) - expected)
        gone |= set(removed)
        if not new:
            text = "only in " + args.rev
        elif not old:
            text = "new file"
        else:
            text = "differs in " + ", ".join(diff) if diff else f"identical ({len(both)} functions)"
        for what, names in (("added", added), ("removed", removed)):
            if names:
                text += f"; {what}: " + ", ".join(f + " (expected)" if what == "removed" and f in expected else f
                                                  for f in names)
        print(f"{src}: {text}")
        for f in moved_in:
            same = funcs[home["old"][f], "old"][f] == new[f]
            bad += not same
            print(f"  {f} moved from {home['old'][f]} to {src}: {'identical' if same else 'differs'}")
    if expected - gone:
        print("--removed names that were not removed: " + ", ".join(sorted(expected - gone)))
    return 1 if bad or expected - gone else 0


if __name__ == "__main__":
    sys.exit(main())
