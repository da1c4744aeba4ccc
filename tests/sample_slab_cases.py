"""Decompositions, the ownership model and the particles for the velocity sampling on slabs (lfa_sample_velocity_collective,
lfa_mesher_vertex_velocities_collective; libfluid_amd/csrc/sample.hip). No GPU here.

Grid and points are those of tests/sample_cases.py, unchanged: 40 x 24 x 17 cells, three tile layers, the last holding ONE cell
layer. Offset and cell size are no binary fractions, so of the lattice points built for cell z = 8 some divide back into cell 7: on
that slab face the fp64 division alone decides the owner.

owner(points, bounds)   : the rank whose tile layers hold trunc(fi_z) >> 3, -1 for an outside point.
stitch(cells, bounds)   : the ranks' lfa_download_cells stitched by owned z-range (tests/test_gpu_slabs.py: run_slabs).
reads_ghost(...)        : which owned points have a 3 x 3 x 3 block that reaches the ghost layer below / above.
slab_particles()        : sparse_particles() plus blobs that leave fluid cells on both sides of z = 8 and z = 16."""
import numpy as np

from libfluid_amd import CELL_DTYPE, PARTICLE_DTYPE
from tests import sample_cases as sc

BOUNDS = ([0, 1, 3], [0, 2, 3], [0, 1, 2, 3])  # tile layers; a rank that owns the last layer alone owns a single cell layer
N_TILE_LAYERS = -(-sc.SIZE[2] // 8)
FACES = (8, 16)  # the cell layers a slab face can lie on


def owner(points, bounds):
    """int64[n]: the rank that answers each point, -1 for the points outside the grid."""
    fi, inside = sc.classify(points)
    out = np.full(len(fi), -1, dtype=np.int64)
    layer = sc.cells_of(fi[inside])[:, 2] >> 3
    out[inside] = np.searchsorted(np.asarray(bounds), layer, side="right") - 1
    return out


def stitch(cells_per_rank, bounds):
    """One grid from the ranks' downloads: rank r contributes the cell layers [8 bounds[r], min(8 bounds[r + 1], nz))."""
    nx, ny, nz = sc.SIZE
    out = np.zeros(nx * ny * nz, dtype=CELL_DTYPE)
    for r, cells in enumerate(cells_per_rank):
        z0, z1 = 8 * bounds[r], min(8 * bounds[r + 1], nz)
        out.reshape(nz, ny, nx)[z0:z1] = np.asarray(cells, dtype=CELL_DTYPE).reshape(nz, ny, nx)[z0:z1]
    return out


def reads_ghost(points, bounds):
    """(below bool[n], above bool[n]): the point is inside and the block around its cell reaches the cell layer under its owner's
    first layer / over its owner's last one (where there is a neighbour rank)."""
    fi, inside = sc.classify(points)
    own = owner(points, bounds)
    cz = np.zeros(len(fi), dtype=np.int64)
    cz[inside] = sc.cells_of(fi[inside])[:, 2]
    b = np.asarray(bounds)
    lo, hi = 8 * b[np.maximum(own, 0)], 8 * b[np.maximum(own, 0) + 1]
    below = inside & (own > 0) & (cz == lo)
    above = inside & (own < len(bounds) - 2) & (cz == hi - 1)
    return below, above


def slab_particles():
    """sparse_particles() and two blobs of 600 particles across the faces z = 8 and z = 16 (cells [6, 10) and [14, 17) in z), both
    in the tile columns x = 3, 4 that sparse_particles() has dilated already: the tiles x = 0, 1 with y = 2 or z = 2 stay implicit."""
    rng = np.random.default_rng(sc.SEED + 4)
    base = sc.sparse_particles()
    a = np.array([26.0, 9.0, 6.0]) + np.array([5.0, 5.0, 4.0]) * rng.random((600, 3))
    b = np.array([30.0, 14.0, 14.0]) + np.array([5.0, 5.0, 2.999]) * rng.random((600, 3))
    extra = np.zeros(len(a) + len(b), dtype=PARTICLE_DTYPE)
    extra["pos"] = np.array(sc.OFFSET) + np.concatenate([a, b]) * sc.H
    extra["old_pos"] = extra["pos"]
    extra["vel"] = rng.normal(size=(len(extra), 3)) * 0.5
    return np.concatenate([base, extra])


# state (d) of the device test: a collective seed_box inside tile (0, 2, 1), which is implicit until then - the binning after it flags
# tiles of all three layers that the grid of the last P2G does not hold
SEED_BOX = (np.array(sc.OFFSET) + np.array([1.2, 18.2, 9.2]) * sc.H, np.array([3.5, 3.5, 3.5]) * sc.H)
SEED_TILE = (0, 2, 1)


def window(bounds, r):
    """The cell layers of rank r: (8 lo, min(8 hi, nz))."""
    return 8 * bounds[r], min(8 * bounds[r + 1], sc.SIZE[2])


def reach(bounds, r, nz):
    """The cell layers rank r can answer with fresh ghost layers: [max(0, 8 lo - 7), min(nz, 8 hi + 7))."""
    lo = 8 * bounds[r] - 7 if r > 0 else 0
    hi = 8 * bounds[r + 1] + 7 if r + 2 < len(bounds) else nz
    return max(lo, 0), min(hi, nz)
