"""Generates tests/golden/stencil_stages.npz from the REAL reference (oracle/_ref/libref.so) on the cell fields of
tests/stencil_cases.py: per case the unknown list (`fluid_cells`), the matrix bits (`abits`), and the solve's iteration count
(`iters`) and pressure (`p`). Build container only.
The archive is written with fixed time stamps: a second run reproduces it byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import loader as orc  # noqa: E402
from tests import stencil_cases as sc  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stencil_stages.npz")
FIELDS = ("fluid_cells", "abits", "iters", "p")


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


def arrays():
    out = {}
    for name in sc.NAMES:
        st = sc.staged(name, "ref")
        for f in FIELDS:
            out[f"{name}.{f}"] = st[f]
    return out


if __name__ == "__main__":
    orc.build()
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built: the reference sources are needed to generate the golden vectors")
    out = arrays()
    for name in sc.NAMES:
        print(name, len(out[f"{name}.p"]), "unknowns,", int(out[f"{name}.iters"]), "iterations")
    save(PATH, out)
    print(PATH, os.path.getsize(PATH), "bytes")
