"""Designed clouds for the kernels that only stream particles (k_advect_collide, k_advect_collide_count, k_tile_scatter,
k_cell_count, k_build_fine_index, k_g2p): all but the scatter issue all of a thread's loads up front - indices past the end
clamped, invalid slots loaded and dropped - and their stores last, so what can go wrong sits at the tails: a last wave, chunk or loop round
that is partly filled, and lanes of one wave that take different paths. Pure numpy, deterministic from a seed; every builder
returns (size, parts, solid, meta) in the form of tests/move_cases.py (dyadic starts and moves, parts["cx"][:, 0] = the id) or of
tests/transfer_cases.py (g2p_tiles, stale_leavers).

  lattice(n)      n particles on a lattice of pitch 1.5 cells in a ragged 24 x 17 x 17 grid, in shuffled order, moves of at most 0.3
                  cells (some change cells, some tiles): at least 0.86 > re = 0.7071 cells apart before and after, so the
                  position correction of a time step moves none. The padding of the ragged tiles counts as solid: only the tiles (tx, 0, 0) are "clear", every wave mixes
                  lanes of both paths. n in COUNTS: 1, 63, 64, 65, 511, 512, 513 and 64 AC_CHUNKS k +- 1. The largest one also
                  runs on two z-slab ranks split at z = 8 (SLAB_BOUNDS): to each rank the other's particles are holes, key
                  0xFFFFFFFF, lane by lane in every chunk of every wave
  mixed()         32 x 24 x 24 with a plate at x = 30, pitch 2.5: in one wave lanes in open water, lanes in the plate's skin and
                  lanes that run into it, particles that move exactly 7 cells out of a clear tile (the short cut asks for less than 7)
                  and particles ON the max face of the grid (fraction 1 in the last cell)
  mixed_source()  a coercing source over the cells of mixed() with x >= 10 and x + y + z even
  g2p_tiles()     one tile each of 1, 255, 256, 257 and 4 097 particles beside empty ones (transfer_cases.tile_counts)
  stale_leavers() three particle tiles whose particles move after the binning: more than G2P_LV_CAP leave the first, exactly
                  G2P_LV_CAP the second, none the third
"""
import functools
import os
import re

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from tests import move_cases as mc
from tests import transfer_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, M = mc.Q, mc.M


def _define(source, name):
    text = open(os.path.join(ROOT, "libfluid_amd", "csrc", source)).read()
    return int(re.search(r"^#define %s (\d+)" % name, text, re.M).group(1))


AC_CHUNKS = _define("particles.hip", "AC_CHUNKS")    # particles per lane of k_advect_collide_count
G2P_LV_CAP = _define("grid_ops.hip", "G2P_LV_CAP")   # leavers a tile of k_g2p lists in LDS
G2P_THREADS = _define("grid_ops.hip", "G2P_THREADS")
WAVE = 64 * AC_CHUNKS
COUNTS = (1, 63, 64, 65, 511, 512, 513) + tuple(WAVE * k + d for k in (1, 2) for d in (-1, 1) if WAVE * k + d not in (511, 513))
LATTICE_SIZE = (24, 17, 17)
SLAB_N, SLAB_BOUNDS = max(COUNTS), (0, 1, 3)  # two z-slab ranks over the largest lattice, split at tile layer 1 (z = 8)
RE = 0.70710678  # the reach of the position correction in cells


def _finish(size, q16, m12, solid, order, **meta):
    """move_cases._finish at h = 1, dt = 1, without its bar on multiples of 512, in upload order `order`."""
    q16, m12 = np.asarray(q16, dtype=np.int64)[order], np.asarray(m12, dtype=np.int64)[order]
    n = len(q16)
    assert len(np.unique(q16, axis=0)) == n
    parts = np.zeros(n, dtype=PARTICLE_DTYPE)
    parts["pos"] = q16 / Q
    parts["old_pos"] = parts["pos"]
    parts["vel"] = m12 / M
    parts["cx"][:, 0] = np.arange(n)
    if solid is not None:
        solid = np.unique(np.asarray(solid, dtype=np.int32).reshape(-1, 3), axis=0)
        c = np.minimum(q16 // Q, np.asarray(size) - 1)
        assert not mc.solid_mask(size, solid)[c[:, 0], c[:, 1], c[:, 2]].any()
    return (tuple(int(s) for s in size), parts, solid,
            dict(h=1.0, off=(0.0, 0.0, 0.0), dt=1.0, skin=mc.SKIN_WORLD, q16=q16, m12=m12, **meta))


def _spots(counts, first, pitch):
    ijk = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), axis=-1).reshape(-1, 3)
    return ijk, first + pitch * ijk


def lattice(n, seed=808):
    rng = np.random.default_rng(seed)
    ijk, spot = _spots((16, 11, 11), 0.75, 1.5)
    pick = rng.permutation(len(spot))[:n]
    assert len(pick) == n
    q16 = np.rint(spot[pick] * Q).astype(np.int64) + (rng.integers(-650, 650, size=(n, 3)) * 2 + 1)  # odd: never on a face
    m12 = rng.integers(-int(0.3 * M), int(0.3 * M) + 1, size=(n, 3))
    return _finish(LATTICE_SIZE, q16, m12, None, np.arange(n), isolated=True)


MIXED_SIZE = (32, 24, 24)
PLATE_X = 30


def mixed(seed=909):
    rng = np.random.default_rng(seed)
    ijk, spot = _spots((12, 9, 9), 1.25, 2.5)
    n = len(spot)
    q16 = np.rint(spot * Q).astype(np.int64) + (rng.integers(-650, 650, size=(n, 3)) * 2 + 1)
    m12 = rng.integers(-int(0.2 * M), int(0.2 * M) + 1, size=(n, 3))
    kind = np.full(n, "plain", dtype=object)
    i, j, k = ijk.T
    # the last lattice layer before the plate: in its skin (cell 29, fraction above 1 - skin) at rest along x, or a cell in
    # front of it and moving one cell: the march stops it
    skin = (i == 11) & ((j + k) % 2 == 0)
    q16[skin, 0] = PLATE_X * Q - rng.integers(1, int(0.08 * Q) // 2, size=skin.sum()) * 2 + 1
    m12[skin, 0] = 0
    kind[skin] = "skin"
    hit = (i == 11) & ((j + k) % 2 == 1)
    q16[hit, 0] = np.rint(29.5 * Q).astype(np.int64) + 1
    m12[hit, 0] = M
    kind[hit] = "hit"
    # exactly 7 cells along x out of tile 0 (clear); the lattice spot they land beside (i = 3, 8.75) stays empty in their rows
    seven = (i == 0) & ((j + k) % 3 == 0)
    m12[seven] = (7 * M, 0, 0)
    kind[seven] = "seven"
    keep = ~((i == 3) & ((j + k) % 3 == 0))
    # on the max face of y (fraction 1 in the last cell), at rest: in clear tiles (x < 16) and beside the plate's tiles
    face = (j == 8) & (k % 2 == 0) & (kind == "plain")
    q16[face, 1] = MIXED_SIZE[1] * Q
    m12[face, 1] = 0
    kind[face] = "max_face"
    order = rng.permutation(np.flatnonzero(keep))
    plate = [(PLATE_X, y, z) for y in range(MIXED_SIZE[1]) for z in range(MIXED_SIZE[2])]
    return _finish(MIXED_SIZE, q16, m12, plate, order, isolated=True, kind=tuple(kind[order]))


def mixed_source():
    """((cells, velocity) of the coercing source, the cloud): the particles whose cell the source covers take its velocity."""
    nx, ny, nz = MIXED_SIZE
    cells = [(x, y, z) for x in range(10, nx) for y in range(ny) for z in range(nz) if (x + y + z) % 2 == 0 and x != PLATE_X]
    return (np.array(cells, dtype=np.int32), (0.125, -0.0625, 0.1875)), build("mixed")


G2P_TILE_COUNTS = (1, 255, 256, 257, 4097)


def g2p_tiles():
    return tc.tile_counts(counts=G2P_TILE_COUNTS, seed=111)


STALE_SIZE = (40, 16, 16)
STALE_TILES = (((0, 0, 0), G2P_LV_CAP + 44, 100), ((2, 0, 0), G2P_LV_CAP, 60), ((4, 1, 1), 0, 5))  # (tile, leavers, stayers)


def stale_leavers(seed=1010):
    """Leavers start 0.05 .. 0.25 cells short of their tile's +x face and move 0.5 cells along x (velocity = move: dt = 1), the
    others start in the tile's x = 1 .. 6 and move 0.25: whatever fp32 makes of the positions, who leaves is not in doubt. The
    neighbour tile they enter holds no particle of its own; it is processed as a neighbour of a particle tile."""
    rng = np.random.default_rng(seed)
    pos, vel, leaves = [], [], []
    for (tx, ty, tz), n_leave, n_stay in STALE_TILES:
        corner = 8.0 * np.array([tx, ty, tz])
        yz = lambda n: rng.uniform(0.5, 7.5, size=(n, 2))
        pos.append(corner + np.column_stack([rng.uniform(7.75, 7.95, size=n_leave), yz(n_leave)]))
        pos.append(corner + np.column_stack([rng.uniform(1.0, 6.0, size=n_stay), yz(n_stay)]))
        vel += [np.tile([0.5, 0.0, 0.0], (n_leave, 1)), np.tile([0.25, 0.0, 0.0], (n_stay, 1))]
        leaves += [np.ones(n_leave, dtype=bool), np.zeros(n_stay, dtype=bool)]
    order = rng.permutation(sum(len(p) for p in pos))
    size, parts, solid, meta = tc._finish(STALE_SIZE, np.concatenate(pos)[order], rng, vel=3.0)
    parts["vel"] = np.concatenate(vel)[order]
    return size, parts, solid, dict(meta, dt=1.0, leaves=np.concatenate(leaves)[order])


CASES = {f"lattice_n{n}": functools.partial(lattice, n) for n in COUNTS}
CASES.update({"mixed": mixed, "g2p_tiles": g2p_tiles, "stale_leavers": stale_leavers})
LATTICES = tuple(n for n in CASES if n.startswith("lattice"))


@functools.lru_cache(maxsize=None)
def build(name):
    """(size, parts, solid, meta) of a case; cached and read-only - callers copy `parts` before they change it."""
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


def tile_of(size, pos):
    """The 8^3 tile of each position (in cells, clamped like a binning clamps), as a tuple-able int64[n, 3]."""
    return np.minimum(np.floor(np.asarray(pos)).astype(np.int64), np.asarray(size) - 1) // 8


# ---------------------------------------------------------------------------------------------------- the oracle's results
def _by_id(arr, ids):
    out = np.empty_like(arr)
    out[ids] = arr
    return out


def _hashed(s, n):
    """What a hash() of the oracle leaves, by particle id: (positions, raw cell index), cell counts, fluid cells."""
    s.hash()
    after = s.particles()
    ids = np.rint(after["cx"][:, 0]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(n))
    return dict(pos=_by_id(after["pos"], ids), raw=_by_id(after["raw"], ids), counts=s.space_hash()[1].astype(np.uint32),
                fluid_cells=s.fluid_cells())


@functools.lru_cache(maxsize=None)
def oracle_moves(name):
    """The oracle on a move case: {"move": hash, advect, detect_collisions, hash; "step": one time_step, then a hash}; each as
    _hashed() gives it. Computed once and shared; read-only."""
    from oracle import loader as orc
    size, parts, solid, meta = build(name)
    out = {}
    for what in ("move", "step"):
        s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=mc.METHOD, blending=mc.BLEND)
        if solid is not None:
            s.set_solid_cells(solid)
        s.set_particles(parts)
        if what == "move":
            s.hash()
            s.L.advect(s.h, meta["dt"])
            s.L.detect_collisions(s.h)
        else:
            s.L.time_step(s.h, meta["dt"], None, None)
        out[what] = _hashed(s, len(parts))
        s.close()
        for v in out[what].values():
            v.setflags(write=False)
    return out
