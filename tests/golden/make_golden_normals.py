"""Generates tests/golden/mesher_normals.npz from the REAL reference (oracle/_ref/libref.so): mesh::generate_normals() of the
meshes in tests/golden/mesher.npz and of the extra fields of tests/mesher_normals_cases.py, whose values, positions and indices
(the real reference mesher's) are stored too. Needs oracle/_ref/libref.so (oracle.loader.build()). Data only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import loader as orc  # noqa: E402
from tests import mesher_normals_cases as nc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    orc.build()
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built")
    with np.load(os.path.join(HERE, "mesher.npz")) as z:
        g = {k: z[k] for k in z.files}
    out = {}
    for name in nc.GOLDEN_MESHES:
        out[f"{name}_normals"] = orc.ref_mesh_obj(g[f"{name}_pos"], g[f"{name}_idx"], normals=True)[1]
        print(name, out[f"{name}_normals"].shape)
    for name in nc.EXTRA_FIELDS:
        v, size = nc.extra_field(name)
        pos, idx = orc.mesher_mesh(None, size, values=v, kind="ref", **nc.FIELD_GRID)
        nrm = orc.ref_mesh_obj(pos, idx, normals=True)[1]
        out.update({f"{name}_values": v, f"{name}_pos": pos, f"{name}_idx": idx, f"{name}_normals": nrm})
        print(name, pos.shape, idx.shape, nc.fallbacks_and_nans(pos, idx))
    parts, vo, io = [], 0, 0
    for nv, ni in g["cases_counts"]:
        pos, idx = g["cases_pos"][vo:vo + nv], g["cases_idx"][io:io + ni]
        parts.append(orc.ref_mesh_obj(pos, idx, normals=True)[1] if nv else np.zeros((0, 3)))
        vo, io = vo + nv, io + ni
    out["cases_normals"] = np.concatenate(parts)
    path = os.path.join(HERE, "mesher_normals.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")
