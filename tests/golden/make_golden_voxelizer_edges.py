"""Generates tests/golden/voxelizer_edges.npz from the REAL reference voxelizer (oracle/_ref/libref.so) on the inputs of
tests/voxel_edge_cases.py. Build container only. Mesh cases are stored like voxelizer.npz (inputs, grid placement, types,
the two VoxelizerNode lists); grid cases as the types before (`_in`) and after (`_out`) voxelizer::mark_exterior.
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import loader as orc  # noqa: E402
from tests import voxel_edge_cases as vec  # noqa: E402


def save(path, arrays):
    """np.savez_compressed with the zip members in sorted order and dated 1980-01-01."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    orc.build()
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built: the reference sources are needed to generate the golden vectors")
    out = {}
    for name in vec.MESH_NAMES:
        pos, idx, cs, off, rs = vec.make(name)
        gmin, goff, types = orc.voxelize(pos, idx, cs, off, kind="ref")
        cells = orc.ref_voxel_cells(pos, idx, cs, off, True, False, rs)      # cells_ref, interior only
        cells_all = orc.ref_voxel_cells(pos, idx, cs, off, True, True, None)  # cells, interior + surface
        out.update({f"{name}_pos": pos, f"{name}_idx": idx, f"{name}_cs": np.float64(cs), f"{name}_off": np.asarray(off),
                    f"{name}_ref_size": np.asarray(rs, dtype=np.int64), f"{name}_grid_min": gmin, f"{name}_grid_off": goff,
                    f"{name}_types": types, f"{name}_cells_ref_interior": cells, f"{name}_cells_all": cells_all})
        print(name, types.shape, {k: int((types == k).sum()) for k in range(3)}, len(cells), len(cells_all))
    for name in vec.GRID_NAMES:
        t = vec.grid(name)
        res = orc.voxel_mark_exterior(t, kind="ref")
        out.update({f"{name}_in": t, f"{name}_out": res})
        print(name, t.shape, {k: int((t == k).sum()) for k in range(3)}, "->", {k: int((res == k).sum()) for k in range(3)})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "voxelizer_edges.npz")
    save(path, out)
    print(path, os.path.getsize(path), "bytes")
