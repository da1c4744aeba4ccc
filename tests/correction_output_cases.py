"""Clouds for the set-up and the result stores of the position correction's pair kernel (particles.hip, k_correct_fine): the first
staged slot of a block cell comes from the source tiles' fine_start minus the base of the row's run, only the rows' three run
lengths are scanned, and the two parts of a tile run as work items eight apart. Built with the helpers of tests/correction_cases.py
and tests/correction_halfcell_cases.py on grids of at most 24 x 17 x 17 cells (the last tile of a 17-cell axis is one cell wide);
start coordinates are multiples of 2^-16 cells, h = 1, no offset.

  empty_part    tile (1, 0, 0) holds particles in its cells z = 0 .. 3 only, fine layers 0 .. 5: part 1 owns no particle (it still
                stages fine layer 5) and every own row of it is empty.
  window        tile (0, 0, 0) with exactly WINDOW = 3 FINE_CAP / 4 = 4 224 particles and tile (2, 1, 1) with WINDOW + 1; every part
                stages less than FINE_CAP. (The sizes at which a tile's results would or would not fit the positions' LDS: the
                kernel stores every result directly, so both tiles take the one route there is.)
  second_pass   tile (0, 0, 0) with 18 particles per cell, next to tile (1, 0, 0) with 8: a part of the crowded tile stages more
                than FINE_CAP and at most FINE_CAP_BIG (the second pass), no part of the normal one does.
  second_pass_spread  second_pass plus a pair in the middle of eight more tiles: ten particle tiles, so the first eight run in the
                paired order of work items and the last two in the plain one, and the flags of the crowded tile's parts have to
                mean the same part to the first pass, the second pass and the gather kernel.
  last_tile     17 x 17 x 17. Pairs inside the last tile of x, one cell wide: one particle ON the grid's max face x = 17 (t == 1 in
                cell 0 of that tile), its partner behind it; and pairs across the face x = 16 into it.
  lone_tile     tile (1, 1, 1) alone, 8 per cell: the source tiles on all six sides (and the 20 others) have no particles - the
                outer runs of every row have length 0, and the rows by = 0, 12 and bz = 0, nzb - 1 are empty in a row.
  single        two tiles of one particle each, partners across the face x = 8, and a third tile whose one particle has none.
"""
import functools

import numpy as np

from tests import correction_cases as cc
from tests import correction_halfcell_cases as hc
from tests.correction_cases import FINE_CAP, FINE_CAP_BIG, FT, FT_PL, Q, U, qd  # noqa: F401

WINDOW = 3 * FINE_CAP // 4
WINDOW_TILES = ((0, 0, 0), (2, 1, 1))
EMPTY_PART_TILE = (1, 0, 0)
CROWD_TILE, NORMAL_TILE = (0, 0, 0), (1, 0, 0)
LONE_TILE = (1, 1, 1)


def tile_of(cloud):
    """Tile coordinates per particle, int64[n, 3]."""
    size, parts, solid, meta = cloud
    return np.minimum(meta["q"] // Q, np.asarray(size) - 1) // 8


def tile_counts(cloud):
    t, n = np.unique(tile_of(cloud), axis=0, return_counts=True)
    return {tuple(int(c) for c in k): int(v) for k, v in zip(t, n)}


def own_counts(cloud):
    """{(tile, part): own particles}: part 0 owns the fine layers 0 .. FT_PL - 1 of its tile, part 1 the rest."""
    size, parts, solid, meta = cloud
    g = hc.fine_coords(meta["q"], size)
    part = (g[:, 2] % FT) // FT_PL
    out = {}
    for t, p in zip(tile_of(cloud), part):
        k = (tuple(int(c) for c in t), int(p))
        out[k] = out.get(k, 0) + 1
    return out


def staged(cloud):
    return {k: int(v.sum()) for k, v in hc.layout(cloud).items()}


def _shuffled(rng, q):
    return q[rng.permutation(len(q))]


def empty_part(seed=81):
    rng = np.random.default_rng(seed)
    cells = cc._tile_cells(EMPTY_PART_TILE)
    q = cc._fill(rng, cells[cells[:, 2] < 4], (2, 2, 2), 0.1)
    return cc._finish((24, 17, 17), _shuffled(rng, q), None)


def window(seed=83):
    rng = np.random.default_rng(seed)
    out = []
    for t, n in zip(WINDOW_TILES, (WINDOW, WINDOW + 1)):
        cells = cc._tile_cells(t)
        nine = n - 8 * len(cells)  # cells with 9 particles (3 x 3 x 1), the others hold 8 (2 x 2 x 2)
        out += [cc._fill(rng, cells[:nine], (3, 3, 1), 0.05), cc._fill(rng, cells[nine:], (2, 2, 2), 0.05)]
    return cc._finish((24, 17, 17), _shuffled(rng, np.concatenate(out)), None)


def second_pass(seed=85):
    rng = np.random.default_rng(seed)
    q = np.concatenate([cc._fill(rng, cc._tile_cells(CROWD_TILE), (3, 3, 2), 0.04), cc._fill(rng, cc._tile_cells(NORMAL_TILE), (2, 2, 2), 0.04)])
    return cc._finish((24, 17, 17), _shuffled(rng, q), None)


SPREAD_TILES = ((2, 0, 0), (0, 1, 0), (1, 1, 0), (2, 1, 0), (0, 0, 1), (1, 0, 1), (2, 0, 1), (0, 1, 1))


def second_pass_spread():
    """second_pass and a pair in the middle of eight more tiles: ten tiles with particles - the first eight take the paired order
    of work items (part 0 of eight tiles, then their part 1), the last two the plain one -, the crowded tile among the first."""
    size, parts, solid, meta = second_pass()
    d = qd(0.37)
    extra = [[(8 * t[0] + 4) * Q + 3 * U + k * d, (8 * t[1] + 4) * Q + 5 * U, (8 * t[2] + 4) * Q + 7 * U] for t in SPREAD_TILES for k in (0, 1)]
    return cc._finish(size, np.concatenate([meta["q"], np.array(extra, dtype=np.int64)]), None)


def last_tile(seed=87):
    size = (17, 17, 17)
    pl = cc._Placer(size, np.random.default_rng(seed), wall=0.0)
    d = qd(0.37)
    # (y and z clear of the skin of a cell face: see tests/correction_halfcell_cases.py, edges)
    ys = [qd(v) + 5 * U for v in np.arange(2.5, 15.0, 0.65)]
    pl.place(hc._pair(-d), [[17 * Q], ys, ys], kind="max_face")
    pl.place(hc._pair(d), [[16 * Q + qd(0.3)], ys, ys], kind="inside")
    pl.place(hc._pair(d), [[16 * Q - qd(0.2)], ys, ys], kind="across")
    pl.place(hc._pair(-d), [[16 * Q + qd(0.1)], ys, ys], kind="across")
    return cc._finish(size, pl.pts, None, groups=pl.groups)


def lone_tile(seed=89):
    rng = np.random.default_rng(seed)
    q = cc._fill(rng, cc._tile_cells(LONE_TILE), (2, 2, 2), 0.1)
    return cc._finish((24, 17, 17), _shuffled(rng, q), None)


def single():
    y, z = qd(4.3) + 3 * U, qd(3.6) + 5 * U
    q = np.array([[8 * Q - qd(0.15), y, z], [8 * Q + qd(0.2), y, z],   # tiles (0, 0, 0) and (1, 0, 0): 0.35 cells apart
                  [qd(20.4) + U, qd(12.3) + U, qd(11.7) + U]])           # tile (2, 1, 1): alone
    groups = [dict(ids=(0, 1), kind="pair"), dict(ids=(2,), kind="alone")]
    return cc._finish((24, 17, 17), q, None, groups=groups)


CASES = {"empty_part": empty_part, "window": window, "second_pass": second_pass, "second_pass_spread": second_pass_spread,
         "last_tile": last_tile, "lone_tile": lone_tile, "single": single}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def build(name):
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


@functools.lru_cache(maxsize=None)
def oracle(name):
    """cc.run_cpu(case) on the live oracle, computed once and shared; read-only."""
    return cc._frozen(cc.run_cpu(build(name)))
