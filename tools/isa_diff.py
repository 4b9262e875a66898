"""Device assembly of every library source in this tree against another checkout: a plain text diff, nothing else.

    python tools/isa_diff.py <other-tree>
    python tools/isa_diff.py --bodies <other-tree>

Every entry of noisediff_amd.build.SOURCES is compiled from both trees with that module's own flags plus
`--cuda-device-only -S` (needs hipcc; no GPU).  Comment lines, `.ident`, `.file` and lines naming the per-file
`__hip_cuid_<hash>` symbol are dropped, the rest is compared line by line.  Prints `identical` or the number of
differing lines per unit; exit status 1 on any difference.

`--bodies`: for the units that differ, function by function instead.  A function added in the middle of a unit renumbers every later basic-block
label (`.LBB<function>_<block>`), and a new template parameter renames every instance, so the line diff of such a unit is all noise.  This mode cuts each
unit into its functions' instruction streams (label to `.Lfunc_end`), drops trailing comments and the function index of the block labels, and counts the
functions of the OTHER tree whose stream is found unchanged in this tree under any name; the rest are listed by name, as are this tree's additional streams.
"""
from __future__ import annotations

import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from noisediff_amd.build import FLAGS, SOURCES, SPECIAL, _hipcc  # noqa: E402


def device_asm(tree: str, name: str) -> list:
    srcname, flags = SPECIAL.get(name, (name, FLAGS))
    src = os.path.join(tree, "noisediff_amd", "csrc", srcname + ".hip")
    r = subprocess.run([_hipcc(), *flags, "--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}\n{r.stderr}")
    return [ln for ln in r.stdout.splitlines()
            if not ln.lstrip().startswith((";", ".ident", ".file")) and "__hip_cuid_" not in ln]


def bodies(asm: list) -> dict:
    """function name -> its instruction stream, block labels without their function index, trailing comments dropped"""
    out, cur = {}, None
    for ln in asm:
        m = re.match(r"^(\w+):", ln)
        if m and not ln.startswith(".L"):
            cur = out.setdefault(m.group(1), [])
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur.append(re.sub(r"\s*;.*$", "", re.sub(r"\.LBB\d+_", ".LBB_", ln)))
    return {k: [ln.replace(k, "<this function>") for ln in v] for k, v in out.items()}


def main(argv) -> int:
    by_body = "--bodies" in argv
    argv = [a for a in argv if a != "--bodies"]
    if len(argv) != 1:
        print(__doc__, file=sys.stderr)
        return 2
    trees = {"this": ROOT, "other": os.path.abspath(argv[0])}
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        asm = {(t, n): ex.submit(device_asm, trees[t], n) for n in SOURCES for t in trees}
        asm = {k: f.result() for k, f in asm.items()}
    differing = 0
    for n in SOURCES:
        a, b = asm["this", n], asm["other", n]
        d = sum(1 for ln in difflib.unified_diff(b, a, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---")) if a != b else 0
        differing += d > 0
        print(f"{n:16s} {len(a):8d} lines  " + ("identical" if d == 0 else f"{d} lines differ"))
        if d and by_body:
            mine, theirs = bodies(a), bodies(b)
            have = {tuple(v) for v in mine.values()}
            gone = [k for k, v in theirs.items() if tuple(v) not in have]
            kept = {tuple(v) for v in theirs.values()}
            print(f"    {len(theirs) - len(gone)} of the other tree's {len(theirs)} functions have their instruction stream unchanged in this tree")
            for k in gone:
                print(f"    changed or gone: {k}")
            for k, v in mine.items():
                if tuple(v) not in kept:
                    print(f"    only in this tree: {k}")
    print(f"{len(SOURCES) - differing} of {len(SOURCES)} units identical")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
