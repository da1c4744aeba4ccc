"""Inputs of the vertex-normal tests (tests/test_mesher_normals.py, tests/golden/make_golden_normals.py) beyond the meshes of
tests/golden/mesher.npz, and the plain in-order restatement of mesh::generate_normals the fixtures are checked against."""
import numpy as np

from tests import mesher_cases as mc

GOLDEN_MESHES = ["block", "edges", "fine", "field1", "field2", "field3"]  # non-empty meshes of tests/golden/mesher.npz
FIELD_SIZES = {"field1": (7, 6, 5), "field2": (1, 9, 1), "field3": (12, 1, 3)}
FIELD_GRID = dict(grid_offset=(0.25, -1.5, 3.0), cell_size=0.7)

# name -> (vertices, triangles, vertices that take the (1, 0, 0) fallback, vertices with a NaN normal, vertices whose normal is
# exactly (1, 0, 0) by either branch): what the inputs below must keep exercising
EXTRA_FIELDS = {"zeros15": (2289, 3798, 6, 0, 23), "zeros30": (2116, 3183, 14, 0, 51), "nan": (867, 1322, 0, 167, 7)}


def extra_field(name):
    """(values float64[nz+1, ny+1, nx+1], size). Exact zeros at grid points collapse vertices onto corners (degenerate triangles,
    zero sums: the (1, 0, 0) fallback); NaN samples give NaN vertices and NaN normals around them."""
    if name == "zeros15":
        size = (14, 11, 9)
        v = mc.random_field(11, size)
        v[np.random.default_rng(111).random(v.shape) < 0.15] = 0.0
    elif name == "zeros30":
        size = (14, 11, 9)
        v = mc.random_field(12, size)
        v[np.random.default_rng(112).random(v.shape) < 0.3] = 0.0
    elif name == "nan":
        size = (9, 7, 8)
        v = mc.random_field(13, size)
        m = np.random.default_rng(113).random(v.shape)
        v[m < 0.1] = 0.0
        v[(m >= 0.1) & (m < 0.14)] = np.nan
    else:
        raise KeyError(name)
    return v, size


def in_order_normals(positions, indices, with_fallback_mask=False):
    """mesh::generate_normals (include/fluid/data_structures/mesh.h:38-53, NormalT = double) restated: zero, add every
    triangle's cross product to its three corners in index-list order, then normalise or fall back to (1, 0, 0). Plain fp64,
    one operation at a time, in the reference's operand order."""
    pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    with np.errstate(all="ignore"):
        e1, e2 = pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]]
        face = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                         e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        n = np.zeros_like(pos)
        for t in range(len(tri)):  # the order of the additions is the contract
            for v in tri[t]:
                n[v] += face[t]
        sq = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        small = sq <= 1e-6 * 1e-6  # false for NaN: a NaN sum is divided and stays NaN
        out = n / np.sqrt(sq)[:, None]
    out[small] = (1.0, 0.0, 0.0)
    return (out, small) if with_fallback_mask else out


def fallbacks_and_nans(positions, indices):
    """(vertices that take the (1, 0, 0) fallback, vertices with a NaN normal) in the in-order restatement."""
    n, small = in_order_normals(positions, indices, with_fallback_mask=True)
    return int(small.sum()), int(np.isnan(n).any(axis=1).sum())
