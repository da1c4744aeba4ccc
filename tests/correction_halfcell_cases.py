"""Clouds for the position correction's HALF-WIDTH fine cells along x (particles.hip: FTX = 22 half cells of 8/22 cells per tile,
a block row of 26 - the last two of the x-1 tile, the own 22, the first two of the x+1 tile -, a particle walks the five half cells
[hx - 2, hx + 2] of nine rows). Built with the helpers of tests/correction_cases.py on grids of 17 x 9 x 9 and 24 x 17 x 17 cells
(three tiles per axis at most; the last tile of a 17-cell axis is one cell wide). Start coordinates are multiples of 2^-20 cells
(2^-16 but for the partners of the reach pairs), h = 1, no offset: a cell and a fraction below 1 with 20 bits are exact in fp32.

half_coord() and layout() restate the new index and block in numpy. Two half cells are one whole fine cell exactly
((l + t) * 2.75f = 2 ((l + t) * 1.375f) in fp32), so a part stages the same particles as before.

  reach      24 x 17 x 17. Isolated pairs along x, y and z equal. The first particle on the left edge, the right edge and in the middle
             of a half cell - hx = 8 in tile 0 and hx = 9 in tile 1: both parities -, the partner to the right and to the left of it at
             re - 1.1e-6 (kind reach_in: a partner, two half cells away at the most) and at re + 0.8e-6 (reach_out: none) - what the
             lattice of 2^-20 has next to re -/+ 1e-6. At the edge of reach the spring is all but zero, so kind near2 puts a pair's
             particles on the two faces of ONE half cell between them, 0.364 cells apart: each finds the other exactly two half
             cells away, worth thousands of bars.
  faces      17 x 9 x 9. The same pairs across the tile faces x = 8 and x = 16 (the last tile is one cell, three half cells, wide):
             the first particle in the last two half cells of the left tile or the first two of the right one, the partner in the
             neighbour's.
  edges      24 x 17 x 17. rounding: particles whose (l + t) * 2.75f is integral - exactly (l + t = 0 and 4) and by fp32 rounding
             (lattice points just below a half cell's face that the product rounds onto it) - each with a partner 0.364 + cells to
             either side. max_face: a particle ON the grid's max face of x, t == 1 in cell 7 of the last tile (half cell 21), with a
             partner behind it. sparse: a block row of tile (1, 1, 1) whose only record lies in ONE outer half cell (bx = 0, 1, 24,
             25), the partner of an own particle in the neighbouring fine row of y.
  crowded    24 x 17 x 17, jittered sub-lattices confined to fine rows of tile (0, 0, 0) in its fine layers 4, 5 and 6: part 0 stages
             more than FINE_CAP_BIG (the gather kernel takes it), part 1 more than FINE_CAP (the second pass).
"""
import functools
from fractions import Fraction

import numpy as np

from tests import correction_cases as cc
from tests import correction_row_cases as rc
from tests.correction_cases import FB, FINE_CAP, FINE_CAP_BIG, FT, FT_PL, Q, U, above, below, qd  # noqa: F401

FTX, FBX = 2 * FT, 2 * FT + 4
W = Fraction(8, FTX)                               # a half cell, in cells
RE = float(np.sqrt(cc.RE2))
D_IN, D_OUT = int(np.rint((RE - 1e-6) * Q)), int(np.rint((RE + 1e-6) * Q))  # lattice units of 2^-20 cells
OWN_LAYERS = (FT_PL, FT - FT_PL)


# ---------------------------------------------------------------------------------------------------- the new layout
def half_coord(l, t):
    """fine_coord_x() of particles.hip: (int)(((float)l + t) * 2.75f), the last half cell takes the tile's max face."""
    x = (np.asarray(l).astype(np.float32) + np.asarray(t).astype(np.float32)) * np.float32(2.75)
    return np.minimum(x.astype(np.int64), FTX - 1)


def fine_coords(q, size):
    """Global fine coordinates of lattice positions q: (FTX * tile + half cell, FT * tile + fine cell, the same), int64[n, 3]."""
    q = np.asarray(q, dtype=np.int64)
    g = cc.fine_coords(q, size)
    cell = np.minimum(q[:, 0] // Q, size[0] - 1)
    g[:, 0] = FTX * (cell // 8) + half_coord(cell % 8, (q[:, 0] - cell * Q) / Q)
    return g


def layout(cloud):
    """{(tile, part): int64[rows, 26]} for every tile that holds particles: records per block cell, rows r = by + 13 bz."""
    size, parts, solid, meta = cloud
    g = fine_coords(meta["q"], size)
    per_tile = np.array([FTX, FT, FT])
    out = {}
    for t in np.unique(g // per_tile, axis=0):
        for part in (0, 1):
            nzb = OWN_LAYERS[part] + 2
            b = g - per_tile * t + np.array([2, 1, 1])
            b[:, 2] -= part * FT_PL
            b = b[((b >= 0) & (b < np.array([FBX, FB, nzb]))).all(axis=1)]
            counts = np.zeros((FB * nzb, FBX), dtype=np.int64)
            np.add.at(counts, (b[:, 1] + FB * b[:, 2], b[:, 0]), 1)
            out[(tuple(int(c) for c in t), part)] = counts
    return out


def prediction(cloud):
    """(parts handed to the second pass, parts handed to the gather kernel)."""
    staged = {k: int(v.sum()) for k, v in layout(cloud).items()}
    return {k for k, s in staged.items() if s > FINE_CAP}, {k for k, s in staged.items() if s > FINE_CAP_BIG}


def candidates(cloud):
    """Pair candidates per particle: the records of the five half cells [hx - 2, hx + 2] of the nine fine rows around it (itself
    included), and of the three whole fine cells the parent walked - (new, old), int64[n] each."""
    size, parts, solid, meta = cloud
    new, old = fine_coords(meta["q"], size), cc.fine_coords(meta["q"], size)
    out = []
    for g, reach in ((new, 2), (old, 1)):
        d = np.abs(g[:, None, :] - g[None, :, :])
        out.append(((d[:, :, 0] <= reach) & (d[:, :, 1] <= 1) & (d[:, :, 2] <= 1)).sum(axis=1))
    return out


# ---------------------------------------------------------------------------------------------------- spots and pairs
def half_face(tile, k):
    """The left face of half cell k of tile `tile` (x), in cells (a Fraction)."""
    return Fraction(8 * tile) + k * W


def spot(tile, k, where):
    """A lattice point (2^-16) of half cell k: the first one beyond its left face, the last one below its right face, its middle."""
    if where == "left":
        return above(half_face(tile, k))
    if where == "right":
        return below(half_face(tile, k + 1))
    return qd(float(half_face(tile, k) + W / 2))


def _pair(dx, dy=0, dz=0):
    return np.array([[0, 0, 0], [dx, dy, dz]], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- reach
REACH_HALF = ((0, 8), (1, 9))  # (tile, half cell): both parities


def reach(seed=61):
    size = (24, 17, 17)
    pl = cc._Placer(size, np.random.default_rng(seed), wall=1.0)
    for tile, k in REACH_HALF:
        for where in ("left", "right", "mid"):
            for sign in (1, -1):
                for kind, d in (("reach_in", D_IN), ("reach_out", D_OUT)):
                    pl.place(_pair(sign * d), [[spot(tile, k, where)], None, None], kind=kind, where=where, sign=sign, half=k,
                             partners=kind == "reach_in")
        # the two faces of half cell k + 1: the last point of k and the first of k + 2
        pl.place(_pair(spot(tile, k + 2, "left") - spot(tile, k, "right")), [[spot(tile, k, "right")], None, None], kind="near2", half=k)
    return cc._finish(size, pl.pts, None, q_bits=20, groups=pl.groups)


# ---------------------------------------------------------------------------------------------------- tile faces
FACE_SPOTS = (1.53, 4.47, 7.51)  # y and z of the groups of a face: 3 x 3, more than two cells apart, off every fine-row face


def faces():
    size = (17, 9, 9)
    pl = cc._Placer(size, np.random.default_rng(67), wall=0.25)
    for face_tile in (1, 2):  # the face x = 8 * face_tile: half cells 20, 21 of the tile before it, 0, 1 of this one
        left = face_tile - 1
        todo = [(spot(left, 21, "right"), 1), (spot(left, 20, "mid"), 1), (spot(face_tile, 0, "left"), -1), (spot(face_tile, 1, "mid"), -1)]
        groups = [(_pair(sign * d), x, dict(kind=kind, sign=sign, partners=kind == "reach_in")) for x, sign in todo
                  for kind, d in (("reach_in", D_IN), ("reach_out", D_OUT))]
        a, b = (20, 0) if face_tile == 1 else (21, 1)  # one half cell between the two: 21 of the left tile, 0 of the right one
        x = spot(left, a, "right")
        groups.append((_pair(spot(face_tile, b, "left") - x), x, dict(kind="near2")))
        for n, (rel, x, info) in enumerate(groups):
            pl.place(rel, [[x], [qd(FACE_SPOTS[n % 3])], [qd(FACE_SPOTS[n // 3])]], face=face_tile, **info)
    return cc._finish(size, pl.pts, None, q_bits=20, groups=pl.groups)


# ---------------------------------------------------------------------------------------------------- edges
def rounded_onto_faces(tile=1, count=3):
    """Lattice points (2^-20) of tile `tile` strictly below a half cell's left face whose fp32 product (l + t) * 2.75f is that
    face's integer all the same: [(lattice x, k)], the first `count` found from k = 21 down."""
    out = []
    for k in range(FTX - 1, 0, -1):
        f = half_face(0, k) * Q
        x = f.numerator // f.denominator  # the last lattice point below the face, relative to the tile (4 k / 11 is no lattice point)
        l, t = x // Q, (x % Q) / Q
        if (np.float32(l) + np.float32(t)) * np.float32(2.75) == np.float32(k):
            out.append((8 * tile * Q + x, k))
    return out[:count]


SPARSE_BX = (0, 1, FBX - 2, FBX - 1)
SPARSE_TILE = (1, 1, 1)


def edges(seed=71):
    size = (24, 17, 17)
    pl = cc._Placer(size, np.random.default_rng(seed), wall=0.0)
    d = qd(0.37)  # a little more than a half cell: the partners of a particle ON a face lie two half cells away on one side
    trio = np.array([[0, 0, 0], [-d, 0, 0], [d + qd(0.05), 0, 0]], dtype=np.int64)
    pl.place(trio, [[8 * Q], None, None], kind="rounding", exact=True, half=0)             # l + t = 0: on the tile face
    pl.place(trio, [[12 * Q], None, None], kind="rounding", exact=True, half=11)           # l + t = 4: 4 * 2.75 = 11
    for x, k in rounded_onto_faces():
        pl.place(trio, [[x], None, None], kind="rounding", exact=False, half=k)
    # t == 1 in cell 7 of tile 2: x = 24 = the grid's max face
    # (y and z fractions clear of the skin: on the face itself the oracle and the reference treat a particle that is also within
    # the skin of a cell face of y or z differently, which is no business of the correction)
    ys = [qd(v) + 5 * U for v in np.arange(2.5, 15.0, 0.65)]
    pl.place(_pair(-d), [[24 * Q], ys, ys], kind="max_face")
    # a row of tile (1, 1, 1)'s block with ONE record, in an outer half cell: A there, its partner B - an own particle of the tile -
    # two half cells further in and across a fine-row face of y (8 + 8 * 3 / 11 and 8 + 8 * 9 / 11 in turn); own rows of a part
    tx, ty, tz = SPARSE_TILE
    for n, bx in enumerate(SPARSE_BX):
        yface = Fraction(8 * ty) + Fraction(8 * (3, 9)[n % 2], FT)
        dy = (above(yface) + qd(0.04)) - (below(yface) - qd(0.04))
        k = bx - 2  # own-tile half cell of A: -2, -1 (the x-1 tile's 20, 21), 22, 23 (the x+1 tile's 0, 1)
        inward = 1 if k < 0 else -1
        xa = spot(tx + (k // FTX), k % FTX, "right" if k < 0 else "left")  # the two faces of the half cell between them
        xb = spot(tx, k + 2 * inward, "left" if k < 0 else "right")
        z = rc._fine_mid(tz, 2 + 2 * n)
        pl.place(_pair(xb - xa, dy), [[xa], [below(yface) - qd(0.04)], [z]], kind="sparse", bx=bx)
    return cc._finish(size, pl.pts, None, q_bits=20, groups=pl.groups)


# ---------------------------------------------------------------------------------------------------- crowded
CROWD_TILE = (0, 0, 0)
CROWD_ROWS = ([(fy, 4) for fy in (0, 2, 4, 6, 8, 10)] + [(fy, 3) for fy in (1, 3, 5, 7, 9)]           # part 0 alone
              + [(fy, FT_PL - 1) for fy in (1, 3, 5, 7, 9)] + [(fy, FT_PL) for fy in (0, 2, 4, 6, 8)])  # both parts' blocks


def crowded(seed=73):
    size = (24, 17, 17)
    rng = np.random.default_rng(seed)
    q = rc._row_fill(rng, size, CROWD_TILE, CROWD_ROWS, range(0, 8), (6, 5, 5), 0.04)
    return cc._finish(size, q[rng.permutation(len(q))], None, min_dist=1.0 / 6.0 - 0.08 - 2.0 ** -15)


# ---------------------------------------------------------------------------------------------------- the cases
CASES = {"reach": reach, "faces": faces, "edges": edges, "crowded": crowded}
NAMES = tuple(CASES)
ISOLATED = ("reach", "faces", "edges")


@functools.lru_cache(maxsize=None)
def build(name):
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


@functools.lru_cache(maxsize=None)
def oracle(name):
    """cc.run_cpu(case) on the live oracle, computed once and shared; read-only."""
    return cc._frozen(cc.run_cpu(build(name)))


def groups_of(name, kind):
    return [g for g in build(name)[3]["groups"] if g["kind"] == kind]
