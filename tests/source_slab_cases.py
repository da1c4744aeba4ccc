"""The scenes of tests/test_gpu_source_rng_slabs.py (lfa_update_sources_rng with LFA_SEED_COLLECTIVE on slab decompositions) and
what tests/source_model.py - pinned to the compiled reference by tests/test_source_model.py - says about them: which rank owns
which new particle. Shared by the GPU tests and by tests/test_source_slab_cases.py, which checks on the CPU that the scenes do
what they are there for. A case: (grid, parts or None, sources, ltr) as in tests/source_cases.py, plus the tile-layer bounds to
run it on."""
import functools

import numpy as np

from tests import seed_model as sm
from tests import seed_slab_cases as ssc
from tests import source_cases as sc
from tests import source_model as srcm

TALL = dict(size=(16, 16, 24), cell_size=1.0, offset=(0.0, 0.0, 0.0))
# one ulp of z is 2^-7 up there: about 1 in 256 positions rounds onto the far z face of its source cell
FAR = dict(size=(16, 16, 24), cell_size=1.0, offset=(0.0, 0.0, float(2 ** 45)))
X_FACE_CELLS = [(3, 4, 7), (9, 2, 15), (5, 5, 8), (6, 6, 23), (3, 4, 6)]

# C interleaves the ranks' entries inside and across sources; in B rank 1 keeps nothing; E_root16: 24 576 draws in one entry
REUSED = ("A", "B", "C", "E_root16", "F_ltr_B", "D_h05")
BOUNDS = {name: ([0, 1, 2],) for name in REUSED}
BOUNDS["I_interleave"] = ([0, 1, 2, 3], [0, 1, 3], [0, 2, 3])
BOUNDS["X_face"] = ([0, 1, 2, 3],)
ALL = list(BOUNDS)
PAIRS = [(name, b) for name in ALL for b in BOUNDS[name]]


def _interleave():
    """315 cells that visit the three tile layers in turn - z = 3, 12, 20, 4, 13, 21, ... - so the entries of every rank are spread
    over the whole scan (which crosses 256-entry workgroups), and a second source that lies in one cell layer."""
    cells = []
    for k in range(105):
        x, y, dz = k % 16, k // 16, k % 4
        cells += [(x, y, 3 + dz), (x, y, 12 + dz), (x, y, 20 + dz)]
    plane = [(x, y, 9) for y in range(2, 6) for x in range(2, 6)]
    return [(cells, (0.0, 1.0, -2.0), 2, True), (plane, (3.0, 0.0, 0.0), 3, True)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(grid, parts or None, sources, ltr)"""
    if name in REUSED:
        return sc.case(name)
    if name == "I_interleave":
        return TALL, None, _interleave(), False
    if name == "X_face":
        return FAR, None, [(X_FACE_CELLS, (0.0, 0.0, 1.0), 16, True)], False
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's (positions in draw order, source cells, velocities, state afterwards), from the state of a fresh generator."""
    if name in REUSED:
        return sc.expected(name)
    grid, parts, sources, ltr = case(name)
    assert parts is None
    out = srcm.update_sources(grid["size"], grid["cell_size"], grid["offset"], np.zeros(int(np.prod(grid["size"]))), sources,
                              sm.initial_state(), ltr=ltr)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def owner(grid, pos, bounds):
    """Rank of every position under the tile-layer bounds: the one whose layers hold the clamped cell of the position (its key)."""
    return ssc.owner(grid, pos, bounds)


def source_owner(cells, bounds):
    """Rank whose tile layers hold the SOURCE cell of every particle (what owner() would say if no position ever left its cell)."""
    return np.searchsorted(np.asarray(bounds[1:]), np.asarray(cells)[:, 2] >> 3, side="right")
