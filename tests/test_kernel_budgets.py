"""The register, scratch and LDS budgets of k_correct_fine, read from the compiler's own metadata (tools/kernel_resources.py compiles
particles.hip for gfx950; nothing runs on a device). The kernel asks for 4 waves per SIMD, that is 128 VGPRs, and sits at 127 / 128:
beyond that the compiler spills to scratch without a word, and the first pass must stay at two workgroups per CU (LDS)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = {"k_correct_fine<5632, false>": 81920, "k_correct_fine<12288, true>": 163840}  # static LDS, bytes


def test_k_correct_fine_stays_within_its_vgpr_scratch_and_lds_budgets():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "particles.hip", "k_correct_fine"],
                         capture_output=True, text=True, check=True).stdout
    print(out)
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(k_correct_fine<[^>]*>)\s+vgpr\s+(\d+) sgpr\s+(\d+) spill\s+(\d+) lds\s+(\d+) scratch\s+(\d+)", line)
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert set(seen) == set(BUDGETS), out
    for name, (vgpr, sgpr, spill, lds, scratch) in seen.items():
        assert vgpr <= 128 and spill == 0 and scratch == 0 and lds <= BUDGETS[name], (name, vgpr, spill, lds, scratch)
