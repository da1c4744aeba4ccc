"""Clouds for the 16-byte position record {key, t[3]} (libfluid_amd/csrc/common.h, PosRec): besides the ones it borrows from
tests/streaming_tail_cases.py and tests/correction_output_cases.py, one of its own.

  residues()   24 x 17 x 17, the tiles 0 .. 7 (tile id = tx + 3 (ty + 3 tz)) hold 1, 2, 3, 5, 1, 2, 3, 5 particles at rest, in
               shuffled upload order: tile_start is 0, 1, 3, 6, 11, 12, 14, 17 - every residue mod 4 twice -, so the binned records
               of a tile start at every 16-byte phase of a 64-byte sector, and the 4-byte key array beside them at every dword.
               Dyadic positions (multiples of 2^-16 cells, h = 1, no offset), at least 1.5 cells apart.
"""
import functools

import numpy as np

from tests import binning_cases as bc
from tests import streaming_tail_cases as sc

ROUND_TRIP_COUNTS = (1, 3, 4, 5, 255, 257)  # around one, four and 256 records: the tails of a 16-byte access
RESIDUE_SIZE = (24, 17, 17)
RESIDUE_COUNTS = (1, 2, 3, 5, 1, 2, 3, 5)


def residues(seed=1212):
    rng = np.random.default_rng(seed)
    nt = bc.tiles_of(RESIDUE_SIZE)
    q16 = []
    for tile, count in enumerate(RESIDUE_COUNTS):
        corner = 8 * np.array([tile % nt[0], (tile // nt[0]) % nt[1], tile // (nt[0] * nt[1])])
        for k in range(count):  # along x, 1.5 cells apart; y inside the one cell layer that the last tiles of the 17-cell axis have
            spot = corner + np.array([0.75 + 1.5 * k, 0.40, 2.75])
            q16.append(np.rint(spot * sc.Q).astype(np.int64) + (rng.integers(-650, 650, size=3) * 2 + 1))
    q16 = np.array(q16)
    assert (q16 > 0).all() and (q16 < np.asarray(RESIDUE_SIZE) * sc.Q).all()
    return sc._finish(RESIDUE_SIZE, q16, np.zeros_like(q16), None, rng.permutation(len(q16)), isolated=True)


@functools.lru_cache(maxsize=None)
def build(name):
    size, parts, solid, meta = {"residues": residues}[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


def tile_ids(size, pos):
    """Tile id (x fastest) of each position."""
    nt = bc.tiles_of(size)
    t = sc.tile_of(size, pos)
    return t[:, 0] + nt[0] * (t[:, 1] + nt[1] * t[:, 2])


def tile_starts(size, pos):
    """tile_start of a binning, restated: the exclusive scan of the particles per tile, for the tiles that hold any."""
    ids = tile_ids(size, pos)
    count = np.bincount(ids, minlength=int(np.prod(bc.tiles_of(size))))
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    return start[count > 0], count[count > 0]


@functools.lru_cache(maxsize=None)
def oracle_hash(name):
    """What a hash() of the oracle leaves on a cloud of this module, as streaming_tail_cases._hashed gives it; read-only."""
    from oracle import loader as orc
    from tests import move_cases as mc
    size, parts, solid, meta = build(name)
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=mc.METHOD, blending=mc.BLEND)
    s.set_particles(parts)
    out = sc._hashed(s, len(parts))
    s.close()
    for v in out.values():
        v.setflags(write=False)
    return out
