"""Generates tests/golden/mesher_edges.npz from the REAL reference mesher (oracle/_ref/libref.so) on the inputs of
tests/mesher_edge_cases.py. Build container only. Per case only the counts (points, NaN points, vertices, indices) and the SHA-256
digests of the reference's value, position and index bytes are stored (mesher_edge_cases.summary), as three arrays with one row
per case: no results, a few kilobytes.
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import loader as orc  # noqa: E402
from tests import mesher_edge_cases as ec  # noqa: E402
from tests.golden.make_golden_voxelizer_edges import save  # noqa: E402

if __name__ == "__main__":
    orc.build()
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built: the reference sources are needed to generate the golden vectors")
    names, all_counts, all_sha = [], [], []
    for prefix, cases, is_field in (("cloud", ec.CLOUD_IDS, False), ("field", ec.FIELD_IDS, True)):
        for cid in list(cases):
            counts, sha = ec.summary(*ec.results(cid, "ref", is_field))
            names.append(f"{prefix}:{cid}")
            all_counts.append(counts)
            all_sha.append(sha)
            print(prefix, cid, counts.tolist(), bytes(sha[0][:4]).hex(), bytes(sha[1][:4]).hex(), bytes(sha[2][:4]).hex())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesher_edges.npz")
    save(path, dict(ids=np.array(names),counts=np.stack(all_counts), sha=np.stack(all_sha)))
    print(path, os.path.getsize(path), "bytes")
