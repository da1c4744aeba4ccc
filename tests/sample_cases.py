"""Inputs and the model for the velocity sampling (lfa_sample_velocity, libfluid_amd/csrc/sample.hip). No GPU here.

The grid is 40 x 24 x 17: 5 x 3 x 3 tiles of 8^3, ragged in y and z, the last z tile holding one layer. Cell size 0.3 and offset
(0.69, -0.35, 15.3) are no binary fractions, so a face off + c h can divide back to just under c: only the fp64 division decides a
point's cell, and the model below is that rule in numpy.

The points (POINTS, seeded):
  lattice : per axis the cells {0, 1, n - 2, n - 1} and both sides of every tile face - 12 x 8 x 6 cells; each cell with the 8
            diagonal fraction triples of FRACTIONS and 8 random triples from the same set. These sit where the kernel's one-tile path
            and its general path meet, and where samples are clamped.
  random  : 4 096 uniform points in the box.
  outside : the block OUTSIDE_BLOCK (one of them lands INSIDE: the far face on z alone, 5.1 / 0.3 rounds below 17).
  corners : the offset corner itself, and one and two ulps below the far corner.

model(cells, points): the classification, then the oracle's (or the compiled reference's) PIC grid-to-particle transfer on the
inside points. Outside points: velocity +0, type 0, counted."""
import numpy as np

from libfluid_amd import CELL_DTYPE, PARTICLE_DTYPE
from oracle import loader as orc

SIZE = (40, 24, 17)
H = 0.3
OFFSET = (0.69, -0.35, 15.3)
SEED = 20261019
FRACTIONS = np.array([0.0, 2.0 ** -30, 0.25, np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 0.75, 1.0 - 2.0 ** -30])
N_RANDOM = 4096
GRAVITY = (0.3, -981.0, 0.1)  # of the sparse and the stepped states
DT = 0.01

_N = np.array(SIZE, dtype=np.float64)
_OFF = np.array(OFFSET, dtype=np.float64)


def axis_cells(n):
    """{0, 1, n - 2, n - 1} and both sides of every tile face."""
    cells = {0, 1, n - 2, n - 1}
    for face in range(8, n, 8):
        cells |= {face - 1, face}
    return sorted(cells)


def lattice():
    """(points float64[m, 3], cells int64[m, 3] the cell each point was BUILT for, fraction indices int64[m, 3])."""
    rng = np.random.default_rng(SEED)
    ax = [axis_cells(n) for n in SIZE]
    cells = np.array([(x, y, z) for z in ax[2] for y in ax[1] for x in ax[0]], dtype=np.int64)
    diag = np.repeat(np.arange(8)[:, None], 3, axis=1)
    which = np.concatenate([np.concatenate([diag, rng.integers(0, 8, size=(8, 3))]) for _ in range(len(cells))])
    built = np.repeat(cells, 16, axis=0)
    pts = _OFF + (built.astype(np.float64) + FRACTIONS[which]) * H
    return pts, built, which


def random_points():
    rng = np.random.default_rng(SEED + 1)
    return _OFF + rng.random((N_RANDOM, 3)) * (_N * H)


def outside_block():
    """The 11 points of the outside block; the others' coordinates of a point that leaves on one axis are well inside."""
    mid = _OFF + np.array([13.37, 9.21, 5.63]) * H
    far = _OFF + _N * H
    rows = [np.nextafter(_OFF, -np.inf),            # one ulp below the offset corner
            [_OFF[0] - H, mid[1], mid[2]],          # one cell below on x
            far,                                    # the far corner
            [far[0], mid[1], mid[2]], [mid[0], far[1], mid[2]], [mid[0], mid[1], far[2]],  # the far faces, each alone
            [np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]], [mid[0], mid[1], -np.inf],
            [1e300, -1e300, 1e300],
            [mid[0], mid[1], mid[2] + 1e19]]
    return np.array(rows, dtype=np.float64)


def corner_checks():
    far = _OFF + _N * H
    one = np.nextafter(far, -np.inf)
    return np.array([_OFF, one, np.nextafter(one, -np.inf)], dtype=np.float64)


def points():
    """Every point, in the order lattice | random | outside block | corner checks."""
    return np.ascontiguousarray(np.concatenate([lattice()[0], random_points(), outside_block(), corner_checks()]))


def classify(pts):
    """(fi float64[n, 3], inside bool[n]): fi = (x - offset) / h, a true fp64 division; inside iff fi >= 0 && fi < n on all three
    axes, decided on the doubles - no cast comes before it, and a NaN compares false."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        fi = (pts - _OFF) / H
        inside = ((fi >= 0.0) & (fi < _N)).all(axis=1)
    return fi, inside


def cells_of(fi):
    """trunc(fi) of INSIDE points (particle::compute_cell_index_and_position)."""
    return np.trunc(fi).astype(np.int64)


def raw_index(c):
    return c[:, 0] + SIZE[0] * (c[:, 1] + SIZE[1] * c[:, 2])


def model(cells, pts, kind="oracle"):
    """(velocity float64[n, 3], types uint8[n], n_outside) on the grid `cells` (CELL_DTYPE[nx ny nz], x fastest)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
    fi, inside = classify(pts)
    vel = np.zeros((len(pts), 3), dtype=np.float64)
    types = np.zeros(len(pts), dtype=np.uint8)
    if inside.any():
        sim = orc.CpuSim(SIZE, cell_size=H, offset=OFFSET, method=orc.PIC, kind=kind)
        sim.set_cells(cells)
        parts = np.zeros(int(inside.sum()), dtype=PARTICLE_DTYPE)
        parts["pos"] = pts[inside]
        sim.set_particles(parts)
        sim.g2p()
        vel[inside] = sim.particles()["vel"]
        sim.close()
        types[inside] = cells["type"][raw_index(cells_of(fi[inside]))]
    return vel, types, int((~inside).sum())


def random_field(seed=SEED + 2):
    """A grid of fp32-representable velocities and random types (air, fluid, solid)."""
    rng = np.random.default_rng(seed)
    n = SIZE[0] * SIZE[1] * SIZE[2]
    cells = np.zeros(n, dtype=CELL_DTYPE)
    cells["vel"] = (rng.normal(size=(n, 3)) * 3.0).astype(np.float32).astype(np.float64)
    cells["type"] = rng.choice(np.array([orc.AIR, orc.FLUID, orc.SOLID], dtype=np.uint8), size=n)
    return cells


def sparse_particles():
    """About 4 000 particles in the cells [2, 6)^3 and a second blob inside tile (3, 1, 1): most tiles of the grid stay implicit."""
    rng = np.random.default_rng(SEED + 3)
    a = 2.0 + 4.0 * rng.random((3500, 3))
    b = np.array([25.0, 9.0, 9.0]) + 5.0 * rng.random((500, 3))
    parts = np.zeros(len(a) + len(b), dtype=PARTICLE_DTYPE)
    parts["pos"] = _OFF + np.concatenate([a, b]) * H
    parts["old_pos"] = parts["pos"]
    parts["vel"] = rng.normal(size=(len(parts), 3)) * 0.5
    return parts


def neighbourhood_stats(pts):
    """For the inside points: on how many axes the 3 x 3 x 3 block crosses a tile face, and on how many a sample is clamped (an
    index below 0 or at or above n - 1)."""
    fi, inside = classify(pts)
    c = cells_of(fi[inside])
    n = np.array(SIZE, dtype=np.int64)
    lo, hi = np.maximum(c - 1, 0), np.minimum(c + 1, n - 1)
    crosses = (lo >> 3) != (hi >> 3)
    clamped = (c - 1 < 0) | (c + 1 >= n - 1)
    return crosses.sum(axis=1), clamped.sum(axis=1)
