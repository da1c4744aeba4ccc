"""Static instruction counts of one kernel per source-line range: VALU (v_*), LDS (ds_*), memory (global_/flat_/buffer_/scratch_/
s_load) and everything else, from the device assembly of one source file compiled with the project's flags and line tables
(CPU container: hipcc cross-compiles; nothing runs).  An instruction counts for the line of the nearest .loc before it - the
innermost inlined frame, so a helper's instructions are found at the helper's own lines.
usage: python tools/asm_by_line.py particles.hip 'k_correct_fine<5632, false>' 730-800 [860-905 ...] [-DXYZ ...]
Without ranges: one row per source line of the kernel that has instructions."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libfluid_amd import build as B  # noqa: E402

CLASSES = ("valu", "lds", "mem", "other")


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return "mem"
    return "other"


def kernel_lines(asm, want):
    """{(file, line): Counter(class -> instructions)} of the first kernel whose demangled name contains `want`."""
    names = sorted(set(re.findall(r"^(_Z\w+):", asm, re.M)))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    hit = [n for n, d in zip(names, dem) if want in d]
    if not hit:
        raise SystemExit("no kernel matches %r; kernels: %s" % (want, ", ".join(d for d in dem if "(" in d)[:2000]))
    body = asm[asm.index("\n" + hit[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    files = {int(m.group(1)): m.group(2) for m in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]+)"', asm, re.M)}
    out = collections.defaultdict(collections.Counter)
    cur = (None, 0)
    for ln in body.split("\n"):
        ln = ln.split(";")[0].strip()
        if not ln or ln.endswith(":"):
            continue
        if ln.startswith(".loc"):
            f = ln.split()
            cur = (os.path.basename(files.get(int(f[1]), "?")), int(f[2]))
            continue
        if ln.startswith("."):
            continue
        out[cur][classify(ln.split()[0])] += 1
    return hit[0], out


def main(argv):
    src, want = argv[0], argv[1]
    ranges = [tuple(int(x) for x in a.split("-")) for a in argv[2:] if re.fullmatch(r"\d+-\d+", a)]
    defs = [a for a in argv[2:] if a.startswith("-")]
    with tempfile.TemporaryDirectory() as d:
        s = os.path.join(d, "x.s")
        subprocess.run([B._hipcc(), *B.FLAGS, *defs, "-gline-tables-only", "--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", s],
                       check=True, capture_output=True)
        name, per = kernel_lines(open(s).read(), want)
    print("#", name)
    print("# %-22s %7s %7s %7s %7s" % (("lines of " + src)[:22], *CLASSES))
    here = {ln: c for (f, ln), c in per.items() if f == os.path.basename(src)}
    rows = [("%d-%d" % r, [c for ln, c in here.items() if r[0] <= ln <= r[1]]) for r in ranges] if ranges else \
           [(str(ln), [here[ln]]) for ln in sorted(here)]
    rows.append(("other files", [c for (f, ln), c in per.items() if f != os.path.basename(src)]))
    rows.append(("whole kernel", list(per.values())))
    for label, cs in rows:
        tot = sum(cs, collections.Counter())
        print("  %-22s %7d %7d %7d %7d" % (label, *(tot[k] for k in CLASSES)))


if __name__ == "__main__":
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    main(sys.argv[1:])
