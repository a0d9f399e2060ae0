#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE [--only GLOB] [--dropped NAME ...] [--jobs N]

Every hierarchicalgnn_amd/csrc/*.hip of both trees is compiled to device assembly with the flags of
hierarchicalgnn_amd/build.py.  Per kernel symbol three things are compared: the instruction text, the
.amdhsa_kernel descriptor block, and the kernel's entry under amdhsa.kernels (register counts, LDS, private
segment, spill counts).  Only what depends on the order of the kernels in the file or on the path of the source
is normalised: the function index of .LBB<n>_<m> labels and the __hip_cuid_<hash> symbol.

A host-side refactor passes when every kernel of NEW_TREE exists in OLD_TREE and is identical to it, and the only
kernels of OLD_TREE that are gone are the (mangled) names given with --dropped.  Exit status 1 otherwise.
"""
import argparse
import fnmatch
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC"]  # hierarchicalgnn_amd/build.py
CSRC = os.path.join("hierarchicalgnn_amd", "csrc")


def compile_to_asm(src, out):
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", src, "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def normalise(text):
    text = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", text)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)


def kernels(asm):
    """{kernel symbol: (instructions, descriptor block, metadata entry)}"""
    lines = [ln.split(";")[0].rstrip() for ln in normalise(asm).splitlines()]
    lines = [ln for ln in lines if ln.strip()]
    meta = {}
    if "amdhsa.kernels:" in lines:
        entry = None
        for ln in lines[lines.index("amdhsa.kernels:") + 1:]:
            if not ln.startswith("  "):
                break
            if ln.startswith("  - "):
                entry = []
            entry.append(ln)
            m = re.match(r"\s+\.name:\s+(\S+)", ln)
            if m:
                meta[m.group(1)] = entry
    found = {}
    for name in meta:
        start = lines.index(name + ":") + 1
        desc = lines.index("\t.amdhsa_kernel " + name, start)
        found[name] = (lines[start:desc], lines[desc:lines.index("\t.end_amdhsa_kernel", desc) + 1], meta[name])
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--only", default="*.hip", help="file name pattern under csrc/ (default: every .hip)")
    ap.add_argument("--dropped", nargs="*", default=[], help="mangled kernels expected in OLD_TREE only")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()

    def files(tree):
        return {os.path.basename(p): p for p in glob.glob(os.path.join(tree, CSRC, "*.hip"))
                if fnmatch.fnmatch(os.path.basename(p), args.only)}
    old, new = files(args.old_tree), files(args.new_tree)
    bad = sorted(set(old) ^ set(new))
    for name in bad:
        print(f"{name}: in {'OLD' if name in old else 'NEW'} tree only")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max(1, min(args.jobs, 16))) as pool:
        jobs = {(side, name): pool.submit(compile_to_asm, path, os.path.join(tmp, f"{side}_{name}.s"))
                for side, tree in (("old", old), ("new", new)) for name, path in tree.items()}
        asm = {k: kernels(j.result()) for k, j in jobs.items()}
    unexpected = len(bad)
    dropped = []
    for name in sorted(set(old) & set(new)):
        a, b = asm[("old", name)], asm[("new", name)]
        same = [k for k in b if k in a and a[k] == b[k]]
        differ = [k for k in b if k in a and a[k] != b[k]]
        added = [k for k in b if k not in a]
        gone = [k for k in a if k not in b]
        print(f"{name}: {len(a)} kernels before, {len(b)} after: {len(same)} identical, {len(differ)} differ, "
              f"{len(added)} new, {len(gone)} gone")
        for k in differ:
            parts = [w for w, x, y in zip(("instructions", "descriptor", "metadata"), a[k], b[k]) if x != y]
            print(f"  DIFFERS ({', '.join(parts)}): {k}")
        for k in added:
            print(f"  NEW: {k}")
        for k in gone:
            print(f"  GONE{'' if k in args.dropped else ' (not expected)'}: {k}")
        dropped += [k for k in gone if k in args.dropped]
        unexpected += len(differ) + len(added) + sum(k not in args.dropped for k in gone)
    missing = sorted(set(args.dropped) - set(dropped))
    for k in missing:
        print(f"expected to be dropped, but not found in the old tree or still present: {k}")
    unexpected += len(missing)
    print(f"dropped as expected: {len(dropped)}")
    print("IDENTICAL device code" if not unexpected else f"{unexpected} unexpected difference(s)")
    return 1 if unexpected else 0


if __name__ == "__main__":
    sys.exit(main())
