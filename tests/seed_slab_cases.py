"""The scenes of tests/test_gpu_seed_slabs.py and what tests/seed_model.py says about them: which rank owns which particle.
Shared by the GPU tests and by tests/test_seed_slab_cases.py, which checks on the CPU that the scenes do what they are there for."""
import functools

import numpy as np

from tests import seed_model as sm

# the grids and shapes of tests/test_gpu_seed.py: 20 cells in z are 3 tile layers, the top one partial (cells 16..19)
GRID = dict(size=(16, 12, 20), cell_size=0.7, offset=(-1.3, 0.4, 2.1))
VEL = (1.5, -0.25, 3.0)
BOX = ((0.25, 1.1, 3.0), (5.3, 4.9, 6.2))       # z 3.0 .. 9.2: tile layers 0 and 1
CORNER_SPHERE = ((-0.3, 1.2, 15.1), 2.0)         # z 13.1 .. the top of the grid: a sliver of layer 1, and layer 2
TALL_BOX = ((0.25, 1.1, 3.0), (5.3, 4.9, 12.0))  # z 3.0 .. 15.0: all three layers (9 216 candidates at density 2)
LOW_BOX = ((0.25, 1.1, 3.0), (5.3, 4.9, 3.8))    # z 3.0 .. 6.8: inside tile layer 0 (which ends at z = 7.7)
BIG = dict(size=(40, 40, 24), cell_size=1.0, offset=(0.0, 0.0, 0.0))
BIG_BOX = ((0.3, 0.3, 0.3), (39.4, 39.4, 23.4))  # 307 200 candidates at density 2
BOUNDS = ([0, 1, 3], [0, 2, 3], [0, 1, 2, 3])

# test 1: (grid, calls); a call is (kind, a, b, density, ltr) as in tests/test_gpu_seed.py
PARTITION_CASES = {
    "box-d2": (GRID, (("box", *BOX, 2, False),)),
    "box-d3": (GRID, (("box", *BOX, 3, False),)),
    "corner-sphere-d2": (GRID, (("sphere", *CORNER_SPHERE, 2, False),)),
    "tall-box-d2": (GRID, (("box", *TALL_BOX, 2, False),)),
}
# test 2: the testbed's scene 2, the state carried from the sphere to the box
APPEND_CALLS = (("sphere", (4.0, 7.0, 9.0), 1.2, 2, False), ("box", GRID["offset"], (11.2, 2.5, 14.0), 2, False))
LOW_CALLS = (("box", *LOW_BOX, 2, False),)
BIG_CALLS = (("box", *BIG_BOX, 2, False),)

# tests 5 and 6: a dam next to the slab face at z = 16 (and across the one at z = 8), as in tests/test_gpu_slabs.py STEP_CASES
STEP_GRID = dict(size=(16, 16, 32), cell_size=1.0, offset=(0.0, 0.0, 0.0))
STEP_BOX = ("box", (2.0, 0.0, 2.0), (12.0, 12.0, 14.0), 2, False)
STEP_SPHERE = ("sphere", (8.0, 14.0, 16.0), 1.5, 2, False)  # in the air above the dam, across the face at z = 16
STEP_VEL = (0.0, 0.0, 25.0)  # towards the face: a quarter of a cell per step
STEP_BOUNDS = {"apic": [0, 2, 4], "flip": [0, 1, 2, 4]}


def key(grid):
    return tuple(sorted(grid.items()))


@functools.lru_cache(maxsize=None)
def model(grid_key, calls, state=None):
    """[(positions, state after, candidates)] per call, the calls run one after the other on the model."""
    g = dict(grid_key)
    state = sm.initial_state() if state is None else state
    out = []
    for call in calls:
        kind, a, b, density, ltr = call
        fn = sm.seed_box if kind == "box" else sm.seed_sphere
        before = state
        pos, state = fn(g["size"], g["cell_size"], g["offset"], a, b, density=density, state=state, ltr=ltr)
        pos.setflags(write=False)
        n_cand = n_candidates(g, call)
        assert state == sm.advance(before, 6 * n_cand)  # (the count below is the model's)
        out.append((pos, state, n_cand))
    return out


def n_candidates(grid, call):
    """Candidates of a call: the cell range of seed_func (e - s + 1 cells per axis, clamped to the grid above) times density^3."""
    kind, a, b, density, _ = call
    a = np.asarray(a, dtype=np.float64)
    lo, hi = (a, a + np.asarray(b, dtype=np.float64)) if kind == "box" else (a - np.float64(b), a + np.float64(b))
    s, e = sm.cell_unclamped(lo, grid["offset"], grid["cell_size"]), sm.cell_unclamped(hi, grid["offset"], grid["cell_size"])
    ext = [max(min(s[k] + (e[k] - s[k] + 1), int(grid["size"][k])) - s[k], 0) for k in range(3)]
    return ext[0] * ext[1] * ext[2] * int(density) ** 3


def layer(grid, pos):
    """Tile layer of the clamped cell of every position: what decides the owner."""
    g = (np.asarray(pos, dtype=np.float64)[:, 2] - np.float64(grid["offset"][2])) / np.float64(grid["cell_size"])
    cell = np.minimum(np.maximum(np.floor(g), 0), grid["size"][2] - 1).astype(np.int64)
    return cell >> 3


def owner(grid, pos, bounds):
    """Rank of every position under the tile-layer bounds."""
    return np.searchsorted(np.asarray(bounds[1:]), layer(grid, pos), side="right")
