"""Clouds for the STAGING of the position correction (k_correct_fine: the block's fine rows, a slot's row found from the rows'
first slots, the per-row descriptors) and for its epilogue's short cut (an interior tile in open water skips the clamp to the box
and the walls' push-out). Built with the helpers of tests/correction_cases.py; every cloud is dyadic (start coordinates multiples
of 2^-16 cells, h = 1, no offset), at most 24 x 24 x 24 cells and about 12 000 particles.

The block of a work item (tile, part): rows r = by + 13 bz, by = 0 .. 12 the fine rows (y) of the tile and one on each side,
bz = 0 .. own layers + 1 the part's own fine layers (z; 6 for part 0, 5 for part 1) and one on each side; a row's staged slots are
its three segments one after the other - the last fine cell of the x-1 tile, the eleven of the own x tile, the first of the x+1
tile. layout() restates that in numpy.

  sparse_rows       ragged 21 x 13 x 24. Around tile (1, 0, 1): per fine layer three dumbbells ACROSS a fine-row face in y (one
                    record in each of two neighbouring rows), the layers taking turns between the x-1 segment, the own run and the
                    x+1 segment: 48 (part 0) and 42 (part 1) non-empty rows of one record, runs of three empty rows between them -
                    a wave's 64 slots span the whole block. A lone dumbbell in tile (0, 1, 2): a block of one row. Junctions of
                    three in the corner tiles (0, 0, 0) and (2, 1, 2).
  sparse_rows_ends  24^3. Part 1 of tile (1, 1, 1) stages its block's first row (by = 0, bz = 0) and its last row and nothing in
                    between: 89 empty rows.
  long_rows         24^3, jittered sub-lattices confined to single fine rows. In tile (2, 2, 2) one row of more than 192 records -
                    whole waves lie inside it - between an empty row and a row of one record. In tile (0, 0, 0) twelve such rows:
                    part 0 stages more than FINE_CAP (second pass, its own particles still listed), with more than 20 empty rows.
  wall_reach_x, _y  17 x 9 x 9 and 9 x 17 x 9: the last tile of the long axis is ONE cell wide, so the middle tile [8, 16) is not in
                    the outer tile layer and still within reach of the wall. A junction of four in the middle tile: three partners
                    2^-4 cells behind P (cell 15, fraction 0.97) push it by 0.98 cells into cell 16, beyond 1 - skin: the wall
                    pushes it back by more than 0.03 cells. (Two partners push by 2 corr = 0.71 cells at most: from cell 15 a junction
                    of three cannot reach a fraction of 0.9 in cell 16.) Controls: the same junction in tile 0 and in the middle
                    of the middle tile, as far from every wall of the long axis as these grids allow.
  wall_reach_thin_x, _y, _z  17 x 24 x 24, 24 x 17 x 24, 24 x 24 x 17: the same junction in tile (1, 1, 1). Three tiles per axis: the
                    tile is "not in the outer tile layer" on ANY axis and lies in open water, so a short cut decided by tiles
                    would take it and skip the wall's push-out; by cells (c + 7 <= n - 2) it is not interior. In the 17 x 9 x 9
                    grids above no rule calls the tile interior (the 9-cell axes have outer tiles only): those show the reach,
                    these catch the wrong rule.
  wall_reach_low    24^3, tile (1, 1, 1) - the one interior tile, starting at cell 8. The mirror image: P in cell 8 pushed by 0.98
                    cells (less than 7) towards the low wall of x, of y, of z, into cell 7 - nowhere near cell 0, no wall acts. A
                    control in the middle of the tile.
"""
import functools
from fractions import Fraction

import numpy as np

from tests import correction_cases as cc
from tests.correction_cases import FB, FINE_CAP, FINE_CAP_BIG, FT, FT_PL, Q, U, above, below, qd  # noqa: F401

LIST_MAX_BIG = 2 * 2048  # own particles the second pass lists (twice its count array of 2048 words)
OWN_LAYERS = (FT_PL, FT - FT_PL)


# ---------------------------------------------------------------------------------------------------- the block layout
def layout(cloud):
    """{(tile, part): int64[rows, 3]} for every tile that holds particles: records per row r = by + 13 bz and segment (x-1 tile,
    own x tile, x+1 tile) of the part's block."""
    size, parts, solid, meta = cloud
    g = cc.fine_coords(meta["q"], size)
    out = {}
    for t in np.unique(g // FT, axis=0):
        for part in (0, 1):
            nzb = OWN_LAYERS[part] + 2
            b = g - FT * t + 1
            b[:, 2] -= part * FT_PL
            inside = ((b >= 0) & (b < np.array([FB, FB, nzb]))).all(axis=1)
            b = b[inside]
            seg = np.where(b[:, 0] == 0, 0, np.where(b[:, 0] == FB - 1, 2, 1))
            counts = np.zeros((FB * nzb, 3), dtype=np.int64)
            np.add.at(counts, (b[:, 1] + FB * b[:, 2], seg), 1)
            out[(tuple(int(c) for c in t), part)] = counts
    return out


def own_count(counts, part):
    """Own particles of a part: the own-x segment of the rows by = 1 .. 11, bz = 1 .. own layers."""
    rows = counts[:, 1].reshape(-1, FB)
    return int(rows[1:1 + OWN_LAYERS[part], 1:1 + FT].sum())


def wave_spans(counts):
    """Per aligned group of 64 staged slots (a wave of one staging round): (row of its first slot, row of its last slot)."""
    per_row = counts.sum(axis=1)
    row_of_slot = np.repeat(np.arange(len(per_row)), per_row)
    return [(int(row_of_slot[lo]), int(row_of_slot[min(lo + 63, len(row_of_slot) - 1)])) for lo in range(0, len(row_of_slot), 64)]


def empty_runs(counts):
    """Lengths of the runs of consecutive empty rows BETWEEN non-empty rows."""
    full = np.flatnonzero(counts.sum(axis=1) > 0)
    return [int(b - a - 1) for a, b in zip(full[:-1], full[1:]) if b - a > 1]


def prediction(cloud):
    """(parts handed to the second pass, parts handed to the gather kernel), as tests/test_correction_cases.cap_edge_prediction."""
    staged = {k: int(v.sum()) for k, v in layout(cloud).items()}
    return {k for k, s in staged.items() if s > FINE_CAP}, {k for k, s in staged.items() if s > FINE_CAP_BIG}


# ---------------------------------------------------------------------------------------------------- groups
def _fine_face(tile, k):
    """The face between fine cells k - 1 and k of a tile axis, in cells (a Fraction)."""
    return Fraction(8 * tile) + Fraction(8 * k, FT)


def _fine_mid(tile, k):
    """The middle of fine cell k of a tile axis (k = -1: the last one of the tile before, 11: the first of the next), on the lattice."""
    return qd(float(Fraction(8 * tile) + Fraction(8 * (2 * k + 1), 2 * FT)))


def _x_dumbbell(d=0.25):
    return np.array([[0, 0, 0], [qd(d), 0, 0]], dtype=np.int64)


def _junction3(rng):
    """Three particles around the anchor, 0.06 .. 0.15 cells from it on every axis, in three different octants."""
    signs = [(-1, -1, -1), (1, 1, -1), (1, -1, 1)]
    return np.array([[s * int(rng.integers(int(0.06 * 65536), int(0.15 * 65536))) * U for s in sg] for sg in signs], dtype=np.int64)


def _pushed(axis, sign):
    """P at the anchor and three partners 2^-4 cells behind it, 18 degrees off the axis and 120 degrees apart around it: they push
    P by 3 corr k(2^-4) cos 18 = 0.98 cells along sign * axis (and each other sideways)."""
    d, th = 2.0 ** -4, np.deg2rad(18.0)
    o = [b for b in range(3) if b != axis]
    rel = np.zeros((4, 3), dtype=np.int64)
    for k in range(3):
        ph = np.deg2rad(20.0 + 120.0 * k)
        rel[1 + k, axis] = -sign * qd(d * np.cos(th))
        rel[1 + k, o[0]] = qd(d * np.sin(th) * np.cos(ph))
        rel[1 + k, o[1]] = qd(d * np.sin(th) * np.sin(ph))
    return rel


# ---------------------------------------------------------------------------------------------------- sparse rows
SPARSE_TILE = (1, 0, 1)
SPARSE_FACES = (2, 6, 10)   # fine-row faces (y) a dumbbell lies across: rows by = k, k + 1 of its layer hold one record each


def sparse_rows(seed=31):
    size = (21, 13, 24)
    rng = np.random.default_rng(seed)
    pl = cc._Placer(size, rng, wall=1.0)
    tx, ty, tz = SPARSE_TILE
    m = qd(0.26)
    xs = (qd(8 * tx - 0.4), qd(8 * tx + 4.0), qd(8 * tx + 8.4))  # the x-1 tile's last fine cell, the own run, the x+1 tile's first
    for gz in range(-1, FT + 1):
        for k in SPARSE_FACES:
            b = _fine_face(ty, k)
            rel = np.array([[0, below(b) - m, 0], [0, above(b) + m, 0]], dtype=np.int64)
            pl.place(rel, [[xs[(gz + 1) % 3]], [0], [_fine_mid(tz, gz)]], kind="rows", layer=gz, face=k, seg=(gz + 1) % 3)
    pl.place(_x_dumbbell(), [[qd(3.0)], [qd(11.0)], [qd(21.0)]], kind="one_row")
    pl.place(_junction3(rng), [[qd(1.5)], [qd(1.5)], [qd(1.5)]], kind="corner_low")
    pl.place(_junction3(rng), [[qd(19.5)], [qd(11.5)], [qd(22.5)]], kind="corner_high")
    return cc._finish(size, pl.pts, None, groups=pl.groups)


def sparse_rows_ends():
    size = (24, 24, 24)
    pl = cc._Placer(size, np.random.default_rng(37), wall=1.0)
    x = [qd(12.0)]
    pl.place(_x_dumbbell(), [x, [_fine_mid(1, -1)], [_fine_mid(1, FT_PL - 1)]], kind="first_row")   # by = 0, bz = 0 of part 1
    pl.place(_x_dumbbell(), [x, [_fine_mid(1, FT)], [_fine_mid(1, FT)]], kind="last_row")            # by = 12, bz = 6
    pl.place(_x_dumbbell(), [x, [qd(12.0)], [_fine_mid(1, 1)]], kind="own")                          # makes the tile a work item
    return cc._finish(size, pl.pts, None, groups=pl.groups)


# ---------------------------------------------------------------------------------------------------- long rows
def _row_fill(rng, size, tile, rows, xcells, sub, jitter):
    """cc._fill over the cells the fine rows `rows` = [(fy, fz), ..] of `tile` pass through (x cells `xcells` of the tile), cut
    down to the particles whose fine (y, z) is one of the rows."""
    span = lambda k: range((8 * k) // FT, (8 * (k + 1) - 1) // FT + 1)  # noqa: E731  cells (in the tile) fine cell k overlaps
    cells = sorted({(8 * tile[0] + cx, 8 * tile[1] + cy, 8 * tile[2] + cz) for fy, fz in rows for cx in xcells for cy in span(fy)
                    for cz in span(fz)})
    q = cc._fill(rng, cells, sub, jitter)
    g = cc.fine_coords(q, size) - FT * np.asarray(tile)
    keep = np.zeros(len(q), dtype=bool)
    for fy, fz in rows:
        keep |= (g[:, 1] == fy) & (g[:, 2] == fz)
    return q[keep]


LONG_SMALL, LONG_BIG = (2, 2, 2), (0, 0, 0)
LONG_BIG_ROWS = ([(fy, 2) for fy in (2, 4, 6, 8)] + [(fy, 4) for fy in (2, 4, 6)]      # own rows of part 0
                 + [(fy, FT_PL) for fy in (2, 4, 6, 8, 10)])                            # part 0's top halo layer, own to part 1


def long_rows(seed=41):
    size = (24, 24, 24)
    rng = np.random.default_rng(seed)
    small = _row_fill(rng, size, LONG_SMALL, [(3, 3)], range(0, 7), (4, 4, 4), 0.05)
    one = np.array([[8 * 2 + 3, 0, 0]], dtype=np.int64) * Q + np.array([[qd(0.5), _fine_mid(2, 4), _fine_mid(2, 3)]])
    big = _row_fill(rng, size, LONG_BIG, LONG_BIG_ROWS, range(1, 8), (6, 5, 5), 0.04)
    q = np.concatenate([small, one, big])
    return cc._finish(size, q[rng.permutation(len(q))], None, min_dist=1.0 / 6.0 - 0.08 - 2.0 ** -15)


# ---------------------------------------------------------------------------------------------------- wall reach
def _wall_reach(axis):
    size = [9, 9, 9]
    size[axis] = 17
    pl = cc._Placer(size, np.random.default_rng(43 + axis), wall=0.5)
    mid = [[qd(4.5)]] * 3

    def at(v):
        a = list(mid)
        a[axis] = [qd(v)]
        return a

    pl.place(_pushed(axis, +1), at(15.97), kind="into_last_cell", axis=axis)
    pl.place(_pushed(axis, +1), at(1.97), kind="control", axis=axis)
    pl.place(_pushed(axis, -1), at(12.03), kind="control", axis=axis)
    return cc._finish(size, pl.pts, None, groups=pl.groups)


def _wall_reach_thin(axis):
    """The junction of _wall_reach in tile (1, 1, 1) of a grid with 17 cells along `axis` and 24 along the other two: three tiles
    per axis, so "not in the outer tile layer" calls the tile interior on all three axes, while its cell 15 is one cell from the
    last cell of `axis`."""
    size = [24, 24, 24]
    size[axis] = 17
    pl = cc._Placer(size, np.random.default_rng(53 + axis), wall=0.5)

    def at(v, w):
        a = [[qd(w)]] * 3
        a[axis] = [qd(v)]
        return a

    pl.place(_pushed(axis, +1), at(15.97, 12.0), kind="into_last_cell", axis=axis)
    pl.place(_pushed(axis, -1), at(12.03, 9.5), kind="control", axis=axis)
    pl.place(_pushed(axis, +1), at(9.97, 14.5), kind="control", axis=axis)
    return cc._finish(size, pl.pts, None, groups=pl.groups)


def tile_rules(size, tile):
    """(the naive rule "not in the outer tile layer on any axis", the kernel's rule "every cell c of the tile has c - 7 >= 1 and
    c + 7 <= n - 2 on every axis" = t >= 1 and 8 t + 16 <= n) for a tile."""
    naive = all(1 <= t < -(-n // 8) - 1 for t, n in zip(tile, size))
    return naive, all(t >= 1 and 8 * t + 16 <= n for t, n in zip(tile, size))


def wall_reach_low():
    size = (24, 24, 24)
    pl = cc._Placer(size, np.random.default_rng(47), wall=0.5)
    for axis in range(3):
        a = [[qd(10.5 + 2.5 * ((axis + 1) % 3 == b))] for b in range(3)]
        a[axis] = [qd(8.03)]
        pl.place(_pushed(axis, -1), a, kind="towards_low_wall", axis=axis)
    pl.place(_pushed(0, +1), [[qd(12.0)], [qd(14.5)], [qd(14.5)]], kind="control", axis=0)
    return cc._finish(size, pl.pts, None, groups=pl.groups)


# ---------------------------------------------------------------------------------------------------- the cases
CASES = {
    "sparse_rows": sparse_rows,
    "sparse_rows_ends": sparse_rows_ends,
    "long_rows": long_rows,
    "wall_reach_x": lambda: _wall_reach(0),
    "wall_reach_y": lambda: _wall_reach(1),
    "wall_reach_low": wall_reach_low,
    "wall_reach_thin_x": lambda: _wall_reach_thin(0),
    "wall_reach_thin_y": lambda: _wall_reach_thin(1),
    "wall_reach_thin_z": lambda: _wall_reach_thin(2),
}
NAMES = tuple(CASES)
ISOLATED = tuple(n for n in NAMES if n != "long_rows")


@functools.lru_cache(maxsize=None)
def build(name):
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


@functools.lru_cache(maxsize=None)
def oracle(name):
    """cc.run_cpu(case) on the live oracle, computed once and shared; read-only."""
    return cc._frozen(cc.run_cpu(build(name)))


def run_cpu_time_step(cloud, kind="oracle"):
    """One simulation::time_step(DT) from the case's state: positions by id (FLIP carries C, and the id in it, through)."""
    from oracle import loader as orc
    size, parts, solid, meta = cloud
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=cc.METHOD, blending=cc.BLEND, kind=kind)
    s.set_particles(parts)
    s.L.time_step(s.h, cc.DT, None, None)
    after = s.particles()
    s.close()
    ids = np.rint(after["cx"][:, 0]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(len(parts)))
    return cc._by_id(after["pos"], ids)


@functools.lru_cache(maxsize=None)
def oracle_time_step(name):
    return cc._frozen(run_cpu_time_step(build(name)))


def groups_of(name, kind):
    return [g for g in build(name)[3]["groups"] if g["kind"] == kind]
