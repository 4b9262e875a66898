"""Device assembly of every library source in this tree against another checkout: a plain text diff, nothing else.

    python tools/isa_diff.py <other-tree>

Every entry of noisediff_amd.build.SOURCES is compiled from both trees with that module's own flags plus
`--cuda-device-only -S` (needs hipcc; no GPU).  Comment lines, `.ident`, `.file` and lines naming the per-file
`__hip_cuid_<hash>` symbol are dropped, the rest is compared line by line.  Prints `identical` or the number of
differing lines per unit; exit status 1 on any difference.
"""
from __future__ import annotations

import difflib
import os
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


def main(argv) -> int:
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
    print(f"{len(SOURCES) - differing} of {len(SOURCES)} units identical")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
