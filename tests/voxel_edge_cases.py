"""Adversarial inputs for the voxelizer (libfluid_amd/csrc/voxelizer.hip), beside the well-behaved meshes of voxel_cases.py.

Mesh cases, `make(name)` -> (positions, indices, cell_size, ref_offset, ref_size) like voxel_cases.make:
  tower           one triangle whose bounding box is longer than one LDS chunk of cell centres (128) on ALL three axes:
                  the z-chunk loop of k_voxelize_triangles, the `zc` carry and the three loops combined. Cell size 0.1 and
                  odd offsets: every running sum rounds. Its 132 x 132 x 134 grid is also more than 1024 compaction blocks.
  lattice_05      an axis-aligned box whose faces lie on cell boundaries, dyadic: every separating-axis comparison of the
                  touching cells is `>` against an equal value, and the sums are exact.
  lattice_01      the same box at cell size 0.1 (sums round): the corner voxel of the fitted grid comes out SURFACE, so
                  mark_exterior returns at once and nothing is exterior.
  degenerate      five triangles (n_tri % 4 == 1): a point, two vertices at one position, a proper triangle, three collinear
  degenerate_037  vertices, a repeated index; on unit cells and on cells of 0.37 at an odd offset.
  seven           seven triangles (n_tri % 4 == 3): a tetrahedron that encloses interior cells, one triangle inside a single
                  cell of that interior, and the same small triangle twice outside.

Grid cases, `grid(name)` -> uint8[nz, ny, nx], the types before mark_exterior:
  maze            a one-cell serpentine corridor through an all-SURFACE 41 x 27 x 5 grid (no size a multiple of 8): the
                  front crosses block faces hundreds of times. INTERIOR pockets in the walls must stay interior: sealed
                  ones, and ones that touch the corridor only across an edge or only across a corner (6- against
                  18- / 26-connectivity).
  column_x/y/z    grids one cell thick in two directions, a wall part-way along.
  sheet           9 x 17 x 1 with a staggered wall: the cell behind the step is reachable only diagonally.
  stale_*         grids that hold EXTERIOR cells on entry. The reference walks from the corner through cells that are
                  INTERIOR when visited (src/voxelizer.cpp:94-100), so an EXTERIOR cell is a wall and never a seed.
"""
import numpy as np

from libfluid_amd import scenes

INTERIOR, EXTERIOR, SURFACE = 0, 1, 2

MESH_NAMES = ["tower", "lattice_05", "lattice_01", "degenerate", "degenerate_037", "seven"]
GRID_NAMES = ["maze", "column_x", "column_y", "column_z", "sheet", "stale_line", "stale_corner_surface", "stale_reopened",
              "stale_cavity"]
STALE_NAMES = [n for n in GRID_NAMES if n.startswith("stale_")]


def _degenerate():
    pos = np.array([[2.3, 3.1, 1.7],                                        # 0: the point
                    [5.5, 2.25, 4.0], [5.5, 2.25, 4.0], [7.2, 6.1, 4.9],    # 1, 2 at one position
                    [1.2, 6.7, 2.2], [6.9, 7.4, 1.1], [3.3, 1.4, 6.8],      # a proper triangle
                    [1.0, 1.0, 1.0], [3.0, 2.5, 4.0], [5.0, 4.0, 7.0]],     # exactly collinear: steps of (2, 1.5, 3)
                   dtype=np.float64)
    idx = np.array([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 4, 6, 4], dtype=np.uint64)
    return pos, idx


def make(name):
    if name == "tower":
        pos = np.array([[0.31, 0.52, 0.77], [13.13, 13.41, 0.93], [0.95, 1.6, 13.9]], dtype=np.float64)
        return pos, np.array([0, 1, 2], dtype=np.uint64), 0.1, (0.013, -0.027, 0.05), (128, 131, 130)
    if name == "lattice_05":
        pos, idx = scenes.box_mesh((1.0, 1.5, 2.0), (4.0, 3.5, 5.5))
        return pos, idx, 0.5, (0.0, 0.0, 0.0), (7, 8, 10)
    if name == "lattice_01":
        pos, idx = scenes.box_mesh((1.0, 1.5, 2.0), (4.0, 3.5, 5.5))
        return pos, idx, 0.1, (0.0, 0.0, 0.0), (35, 30, 50)
    if name == "degenerate":
        pos, idx = _degenerate()
        return pos, idx, 1.0, (0.0, 0.0, 0.0), (7, 7, 7)
    if name == "degenerate_037":
        pos, idx = _degenerate()
        return pos, idx, 0.37, (-0.4, 0.11, 0.2), (18, 20, 17)
    if name == "seven":
        pos = np.array([[1.0, 1.0, 1.0], [3.0, 1.2, 1.1], [1.9, 3.0, 1.3], [2.0, 1.8, 3.0],   # the tetrahedron
                        [1.93, 1.68, 1.57], [1.98, 1.70, 1.60], [1.95, 1.73, 1.62],           # inside one cell, inside it
                        [3.34, 3.42, 3.30], [3.42, 3.44, 3.35], [3.36, 3.52, 3.40]],          # outside, used twice
                       dtype=np.float64)
        idx = np.array([0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2, 4, 5, 6, 7, 8, 9, 7, 8, 9], dtype=np.uint64)
        return pos, idx, 0.25, (0.05, -0.1, 0.0), (11, 12, 10)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------ grid cases
MAZE_SIZE = (41, 27, 5)   # nx, ny, nz
MAZE_OPEN_X = 39          # the corridor uses x < 39; the columns x = 39, 40 are wall, two cells thick, and hold pockets
# (x, y, z) -> how the pocket meets the corridor
MAZE_POCKETS = {
    (40, 20, 4): "sealed", (40, 15, 2): "sealed", (40, 16, 2): "sealed",
    (20, 13, 3): "edge",    # in the wall between two layers, above and below a wall row: (20, 12, 2) is open, across an edge
    (39, 6, 1): "edge",     # (38, 6, 0) is open
    (39, 7, 0): "edge",     # (38, 6, 0) and (38, 8, 0) are open
    (39, 3, 1): "corner",   # only (38, 2, 0), (38, 4, 0), (38, 2, 2), (38, 4, 2) are open: all three coordinates differ
}


def _maze():
    nx, ny, nz = MAZE_SIZE
    t = np.full((nz, ny, nx), SURFACE, dtype=np.uint8)
    for z in range(0, nz, 2):
        for y in range(ny):
            if y % 2 == 0:
                t[z, y, :MAZE_OPEN_X] = INTERIOR
            else:  # the connectors alternate between the two ends of the rows
                t[z, y, MAZE_OPEN_X - 1 if (y // 2) % 2 == 0 else 0] = INTERIOR
    # a layer ends at (0, ny - 1) when it is entered at (0, 0) and the other way round: 14 rows, an even number of turns
    for z in range(1, nz, 2):
        t[z, ny - 1 if (z // 2) % 2 == 0 else 0, 0] = INTERIOR
    for (x, y, z) in MAZE_POCKETS:
        assert t[z, y, x] == SURFACE
        t[z, y, x] = INTERIOR
    return t


def _shell(shape, lo, hi):
    """EXTERIOR outside, a one-cell SURFACE shell on the box lo..hi (inclusive, per axis in z, y, x order), INTERIOR inside:
    what mark_exterior leaves of a closed box."""
    t = np.full(shape, EXTERIOR, dtype=np.uint8)
    t[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = SURFACE
    t[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = INTERIOR
    return t


def grid(name):
    if name == "maze":
        return _maze()
    if name in ("column_x", "column_y", "column_z"):
        shape = {"column_x": (1, 1, 50), "column_y": (1, 50, 1), "column_z": (50, 1, 1)}[name]
        t = np.zeros(50, dtype=np.uint8)
        t[30] = SURFACE
        return t.reshape(shape)
    if name == "sheet":  # the wall steps from y = 11 to y = 12 at x = 8: (7, 12) is a diagonal neighbour of the open (8, 11)
        t = np.zeros((1, 17, 9), dtype=np.uint8)
        t[0, 11, :8] = SURFACE
        t[0, 12, 8] = SURFACE
        return t
    if name == "stale_line":
        return np.array([1, 1, 0, 0, 0, 0], dtype=np.uint8).reshape(1, 1, 6)
    if name == "stale_corner_surface":
        t = np.zeros((3, 5, 7), dtype=np.uint8)
        t[0, 0, 0] = SURFACE
        t[1, 2, 4] = EXTERIOR
        return t
    if name == "stale_reopened":  # a flooded closed box on 20 x 19 x 18 (x, y, z), then a 2 x 2 hole in its x-low wall
        t = _shell((18, 19, 20), (3, 4, 5), (13, 14, 15))
        t[7:9, 9:11, 5] = INTERIOR
        return t
    if name == "stale_cavity":  # an unflooded closed box with one EXTERIOR cell in its cavity
        t = _shell((10, 11, 12), (2, 2, 3), (7, 8, 9))
        t[t == EXTERIOR] = INTERIOR
        t[4, 5, 6] = EXTERIOR
        return t
    raise KeyError(name)


def spread_rule(types):
    """The rule that is NOT the reference's: seed the corner unless it is SURFACE, then let every EXTERIOR cell, wherever it
    is, turn its INTERIOR face neighbours EXTERIOR until nothing changes. Returns (types, number of sweeps that changed
    something) - from a grid with no EXTERIOR cell the sweeps are the longest shortest path from the corner."""
    t = np.array(types, dtype=np.uint8, copy=True)
    if t.flat[0] != SURFACE:
        t.flat[0] = EXTERIOR
    sweeps = 0
    while True:
        e = np.pad(t == EXTERIOR, 1)
        near = (e[:-2, 1:-1, 1:-1] | e[2:, 1:-1, 1:-1] | e[1:-1, :-2, 1:-1] | e[1:-1, 2:, 1:-1] | e[1:-1, 1:-1, :-2] |
                e[1:-1, 1:-1, 2:])
        new = near & (t == INTERIOR)
        if not new.any():
            return t, sweeps
        t[new] = EXTERIOR
        sweeps += 1
