"""Generates tests/golden/binning.npz from the REAL reference (oracle/_ref/libref.so): update_and_hash_particles on the clouds
tests/binning_cases.GOLDEN (one_tile_prime and its twin, the scan_tiles grids, scan_recursion). Build container only. Per case only
the counts (particles, occupied cells, largest count, cells) and the SHA-256 digests of the reference's raw index per particle, its
count per cell and its _fluid_cells are stored (binning_cases.summary), as three arrays with one row per case: no results, a few
kilobytes. The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import loader as orc  # noqa: E402
from tests import binning_cases as bc  # noqa: E402
from tests.golden.make_golden_voxelizer_edges import save  # noqa: E402

if __name__ == "__main__":
    orc.build()
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built: the reference sources are needed to generate the golden vectors")
    names, all_counts, all_sha = [], [], []
    for name in bc.GOLDEN:
        counts, sha = bc.summary(*bc.run_cpu(bc.build(name), "ref"))
        names.append(name)
        all_counts.append(counts)
        all_sha.append(sha)
        print(name, counts.tolist(), bytes(sha[0][:4]).hex(), bytes(sha[1][:4]).hex(), bytes(sha[2][:4]).hex())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binning.npz")
    save(path, dict(ids=np.array(names), counts=np.stack(all_counts), sha=np.stack(all_sha)))
    print(path, os.path.getsize(path), "bytes")
