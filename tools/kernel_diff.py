"""Compares the kernels of one source file as the working tree builds them with those of a git revision (CPU container: hipcc
cross-compiles): per kernel, whether the instruction stream is identical - otherwise both instruction counts - and VGPRs, SGPRs,
spills, LDS and scratch of both builds. Each side is compiled with its own headers, in a temporary directory.
usage: python tools/kernel_diff.py mg.hip [revision, default HEAD] [name filter]"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libfluid_amd import build as B  # noqa: E402

KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(tree, src):
    """{demangled kernel name: (instructions, resources)} of libfluid_amd/csrc/<src> in the source tree `tree`."""
    csrc = os.path.join(tree, "libfluid_amd", "csrc")
    subprocess.run([B._hipcc(), *B.FLAGS, "-c", os.path.join(csrc, src), "-o", os.path.join(csrc, "x.o"), "--save-temps=obj"],
                   check=True, capture_output=True, cwd=csrc)
    asm = open(next(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith("gfx950.s"))).read()
    meta = {}
    for blk in asm.split("  - .agpr_count:")[1:]:
        get = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        meta[get("name")] = tuple(int(get(k)) for k in KEYS)
    names = list(meta)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for name, nice in zip(names, plain):
        body = asm[re.search(r"^" + re.escape(name) + r":", asm, re.M).start():]
        body = body[:body.index("\n.Lfunc_end")]
        # instructions only: no labels, directives or comments; block labels do not carry the function's number
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in body.split("\n")[1:]]
        ins = [i for i in ins if i and not i.startswith(".") and not i.endswith(":")]
        nice = nice.replace("(anonymous namespace)::", "").removeprefix("void ")
        out[nice.split("(")[0]] = (ins, meta[name])  # (no two kernels of a file differ in their parameter lists alone)
    return out


def main():
    src = sys.argv[1]
    rev = sys.argv[2] if len(sys.argv) > 2 else "HEAD"
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    with tempfile.TemporaryDirectory() as d:
        old, new = os.path.join(d, "old"), os.path.join(d, "new")
        os.makedirs(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "libfluid_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        os.makedirs(os.path.join(new, "libfluid_amd", "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(new, "include"))
        for f in os.listdir(B.CSRC):
            if f.endswith(".h") or f == src:
                shutil.copy(os.path.join(B.CSRC, f), os.path.join(new, "libfluid_amd", "csrc", f))
        a, b = kernels(old, src), kernels(new, src)
    same = 0
    print(f"{src}: {rev} -> working tree    (vgpr sgpr spill lds scratch)")
    for name in sorted(set(a) | set(b)):
        if flt not in name:
            continue
        if name not in a or name not in b:
            print(f"{name:52s} only in {'the working tree' if name in b else rev}")
            continue
        (ia, ra), (ib, rb) = a[name], b[name]
        same += ia == ib
        res = " ".join(str(x) if x == y else f"{x}->{y}" for x, y in zip(ra, rb))
        print(f"{name:52s} {'identical' if ia == ib else f'{len(ia)} -> {len(ib)} instructions':32s} {res}")
    print(f"{same} of {len(set(a) | set(b))} kernels instruction-identical")


if __name__ == "__main__":
    main()
