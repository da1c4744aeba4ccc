"""The scenes of the source-seeding tests (lfa_update_sources_rng): shared by tests/test_source_model.py (model against the
compiled reference and its recorded particles), tests/golden/make_golden_sources.py and tests/test_gpu_source_rng.py (device
against the model). A case: grid (the keywords of Sim / CpuSim), parts (resident 152-byte records, or None), sources
[(cells, velocity, root, active)], ltr."""
import functools

import numpy as np

from libfluid_amd import scenes
from tests import seed_model as sm
from tests import source_model as srcm

UNIT16 = dict(size=(16, 16, 16), cell_size=1.0, offset=(0.0, 0.0, 0.0))
WIDE = dict(size=(24, 16, 16), cell_size=1.0, offset=(0.0, 0.0, 0.0))
ODD_H05 = dict(size=(12, 10, 9), cell_size=0.5, offset=(-3.3, 0.7, 1e-3))
ODD_H17 = dict(size=(12, 10, 9), cell_size=1.7, offset=(-3.3, 0.7, 1e-3))


def _box(lo, hi):
    return [(x, y, z) for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])]


def _ragged():
    """B: a 24 x 16 x 4 block thinned by a fixed mask - cells hold 0 to 8 particles, and the cells of raw index 100-179 and
    1250-1329 stay full (runs of need = 0 in the middle of both sources) - under two sources of 400 cells each: 800 entries, so the
    scan of the needs crosses waves and 256-entry workgroups."""
    parts = scenes.seed_block((0, 0, 0), (24, 16, 4))
    cell =np.floor(parts["pos"]).astype(np.int64)
    raw = cell[:, 0] + 24 * (cell[:, 1] + 16 * cell[:, 2])
    rng = np.random.default_rng(5)
    keep = rng.random(len(parts)) < 0.55
    keep |= ((raw >= 100) & (raw < 180)) | ((raw >= 1250) & (raw < 1330))
    keep &= ~((raw >= 30) & (raw < 40))  # and a few empty cells inside the block
    parts = parts[keep]
    parts["vel"] = rng.normal(size=(len(parts), 3))
    parts["cx"] = rng.normal(size=(len(parts), 3))
    plane = lambda z: _box((0, 0, z), (24, 16, z + 1))  # noqa: E731
    a = plane(0) + plane(1)[:16]   # raw 0..399
    b = plane(3) + plane(4)[:16]   # raw 1152..1535 (thinned) and 16 dry cells above the block
    return parts, [(a, (0.5, -1.0, 0.25), 2, True), (b, (-2.0, 0.0, 1.5), 2, True)]


def _order():
    """C: the sequential semantics. (3,3,3): root 2, then root 3 (8, then 19 more). (5,5,5): root 3, then root 2 (27, nothing, the
    count LOWERED to 8), then root 3 again (19 more: the reference's over-seeding). An inactive source in between. (8,8,8) twice
    in one source. (2,2,2) holds 12 > 8 particles: nothing, the count lowered to 8, then root 3 adds 19."""
    rng = np.random.default_rng(7)
    parts = np.zeros(12 + 3, dtype=scenes.PARTICLE_DTYPE)
    parts["pos"][:12] = np.array([2.0, 2.0, 2.0]) + rng.random((12, 3))
    parts["pos"][12:] = np.array([9.0, 9.0, 9.0]) + rng.random((3, 3))  # (9,9,9) holds 3: topped up by 5
    parts["old_pos"] = parts["pos"]
    parts["vel"] = rng.normal(size=(len(parts), 3))
    sources = [([(3, 3, 3), (9, 9, 9)], (1.0, 0.0, 0.0), 2, True),
               ([(3, 3, 3), (5, 5, 5)], (0.0, 2.0, 0.0), 3, True),
               ([(7, 7, 7), (3, 3, 3)], (9.0, 9.0, 9.0), 3, False),
               ([(5, 5, 5), (8, 8, 8), (8, 8, 8), (2, 2, 2)], (0.0, 0.0, 3.0), 2, True),
               ([(2, 2, 2), (5, 5, 5)], (-1.0, -1.0, -1.0), 3, True)]
    return parts, sources


def _corners(grid):
    """D: cells (0,0,0) and (nx-1, ny-1, nz-1) and a few between, on a grid whose offset and cell size are no binary fractions."""
    nx, ny, nz = grid["size"]
    cells = [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx - 1, 0, 3), (0, ny - 1, nz - 1)] + _box((4, 3, 2), (9, 6, 4))
    return None, [(cells, (0.1, -0.2, 0.3), 2, True), ([(nx - 1, ny - 1, nz - 1), (6, 6, 6)], (1e-3, 1e3, -7.0), 3, True)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(grid, parts or None, sources, ltr)"""
    if name == "A":      # an empty grid, one source of 4 x 4 x 4 cells: 512 particles
        return UNIT16, None, [(_box((6, 10, 6), (10, 14, 10)), (0.0, -3.0, 0.0), 2, True)], False
    if name == "B":
        return (WIDE, *_ragged(), False)
    if name == "C":
        return (UNIT16, *_order(), False)
    if name == "D_h05":
        return (ODD_H05, *_corners(ODD_H05), False)
    if name == "D_h17":
        return (ODD_H17, *_corners(ODD_H17), False)
    if name == "E_root16":  # 4096 particles, 24 576 draws, from one entry
        return UNIT16, None, [([(7, 8, 9)], (0.0, 0.0, 0.0), 16, True)], False
    if name == "E_root1":   # one particle per cell over 300 cells
        return UNIT16, None, [(_box((0, 0, 0), (16, 16, 2))[100:400], (1.0, 2.0, 3.0), 1, True)], False
    if name == "F_ltr_h05":  # LFA_SEED_DRAW_LTR
        return (ODD_H05, *_corners(ODD_H05), True)
    if name == "F_ltr_B":
        return (WIDE, *_ragged(), True)
    raise KeyError(name)


RTL = ["A", "B", "C", "D_h05", "D_h17", "E_root16", "E_root1"]  # what a g++-built reference can produce
ALL = RTL + ["F_ltr_h05", "F_ltr_B"]


@functools.lru_cache(maxsize=None)
def expected(name, state=None):
    """The model's (positions, source_cells, velocities, state afterwards) of a case, from the state of a fresh simulation's
    generator; computed once and shared (read-only)."""
    grid, parts, sources, ltr = case(name)
    pre = np.zeros((0, 3)) if parts is None else parts["pos"]
    counts = srcm.cell_counts(grid["size"], grid["cell_size"], grid["offset"], pre)
    out = srcm.update_sources(grid["size"], grid["cell_size"], grid["offset"], counts, sources,
                              sm.initial_state() if state is None else state, ltr=ltr)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def sorted_rows(pos, *more):
    """Rows of float64[n, 3] sorted lexicographically (the reference's sort by cell is unstable), and `more` in the same order."""
    o = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))
    return (pos[o], *[m[o] for m in more])


def raw_index(grid, cells):
    nx, ny, _ = grid["size"]
    return (cells[:, 0] + nx * (cells[:, 1] + ny * cells[:, 2])).astype(np.uint64)


# ---- the counter-based default of lfa_update_sources (tests/source_model.py: counter_update_sources)
COUNTER_GRID = dict(size=(16, 16, 16), cell_size=0.25, offset=(-1.3, 0.7, 1e-3))
# (3,3,3) under root 2, then root 3: 6, then 19 - and 19 again in every later call; an inactive source in between
COUNTER_SOURCES = [([(3, 3, 3), (5, 9, 12)], (1.0, 0.1, -0.5), 2, True),
                   ([(7, 7, 7), (3, 3, 3)], (9.0, 9.0, 9.0), 3, False),
                   ([(3, 3, 3), (12, 2, 8), (4, 4, 6)], (0.0, 2.5, 0.3), 3, True)]


def counter_parts():
    """Three resident particles at cell centres: two in the source cell (3,3,3), one in (12,2,8)."""
    parts = np.zeros(3, dtype=scenes.PARTICLE_DTYPE)
    cells = np.array([(3, 3, 3), (12, 2, 8), (3, 3, 3)], dtype=np.float64)
    parts["pos"] = np.asarray(COUNTER_GRID["offset"]) + (cells + 0.5) * COUNTER_GRID["cell_size"]
    parts["old_pos"] = parts["pos"]
    parts["vel"] = [(0.5, -1.0, 2.0), (0.0, 0.25, 0.0), (-3.0, 0.0, 1.0)]
    return parts


def counter_expected(n_calls, ranks_z=(None,)):
    """Per call: per rank (records, ids) of counter_update_sources, ids continuing in rank order from the resident particles'."""
    g = COUNTER_GRID
    counts = srcm.cell_counts(g["size"], g["cell_size"], g["offset"], counter_parts()["pos"])
    next_id, calls = 3, []
    for epoch in range(1, n_calls + 1):
        per_rank = []
        for zr in ranks_z:
            rec, ids = srcm.counter_update_sources(g["size"], g["cell_size"], g["offset"], counts, COUNTER_SOURCES, epoch, next_id, zr)
            next_id += len(rec)
            per_rank.append((rec, ids))
        for rec, _ in per_rank:
            counts = counts + np.bincount(rec["raw"].astype(np.int64), minlength=counts.size)
        calls.append(per_rank)
    return calls
