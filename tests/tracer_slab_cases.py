"""Inputs and the ownership model for the tracers on slab decompositions (lfa_tracers_*_collective, libfluid_amd/csrc/tracers.hip).
No GPU here.

A job of N ranks holds a partition of the single domain's tracers: a tracer lives on the rank whose tile layers hold its cell layer
cz >> 3, cz = floor((z - offset_z) / h) clamped to [0, nz - 1] on the double. Every expected value is the oracle's: positions
tc.advect_collide (tests/tracer_cases.py), velocities and types sc.model (tests/sample_cases.py) on the ranks' grids stitched by
owned z-range (tests/sample_slab_cases.py: stitch).

Scene A : grid, offset, cell size and solid block of tests/tracer_cases.py - 40 x 24 x 17 cells, h and offset no binary fractions,
          three tile layers, the last ONE cell layer thick; decompositions ss.BOUNDS.
Scene B : 16 x 16 x 33 cells, five tile layers, the last one cell layer thick; a solid slab of cells that straddles the face z = 16;
          decompositions B.bounds. One step carries tracers over up to four slab faces.
Runs    : RUNS[name] = (scene, groups): the tracers of a job as named groups, so that tests/test_tracer_slab_cases.py can count what
          each group was designed to contain; tracers(name) concatenates them, in the order the job adds them."""
import functools
import math

import numpy as np

from tests import sample_cases as sc
from tests import sample_slab_cases as ss
from tests import tracer_cases as tc

DT = sc.DT
SEED = 20261021
GROUP_SIZES = (1, 63, 64, 65, 513)  # the wave and block boundaries of the ballot and scan placement


class Scene:
    def __init__(self, name, size, h, off, solid, bounds):
        self.name, self.size, self.h, self.off = name, tuple(size), float(h), tuple(float(o) for o in off)
        self.solid = np.asarray(solid, dtype=np.int32)
        self.bounds = tuple(list(b) for b in bounds)
        self.faces = tuple(range(8, self.size[2], 8))  # the cell layers a slab face can lie on

    def grid(self):
        return dict(size=self.size, cell_size=self.h, offset=self.off)

    def mask(self):
        m = np.zeros(self.size, dtype=bool)
        m[self.solid[:, 0], self.solid[:, 1], self.solid[:, 2]] = True
        return m

    def world(self, cells):
        """Grid coordinates (in cells) -> world positions."""
        return np.array(self.off) + np.asarray(cells, dtype=np.float64) * self.h


def _box(lo, hi):
    return np.array([(x, y, z) for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])], dtype=np.int32)


A = Scene("A", sc.SIZE, sc.H, sc.OFFSET, tc.block_cells(), ss.BOUNDS)
B_SLAB_LO, B_SLAB_HI = (4, 4, 15), (12, 12, 17)  # cells [lo, hi): two cell layers, one on each side of the face z = 16
B = Scene("B", (16, 16, 33), 0.3, (-1.3, 2.1, 15.3), _box(B_SLAB_LO, B_SLAB_HI), ([0, 1, 2, 3, 4, 5], [0, 2, 3, 5], [0, 1, 5]))
A_FREE = ((12.0, 38.0), (10.0, 22.0))  # x and y ranges (cells) clear of scene A's block and its skin
B_FREE = ((12.6, 15.2), (1.0, 15.0))   # ... of scene B's slab
B_OVER = ((5.0, 11.0), (5.0, 11.0))    # ... and the columns through it


# ---------------------------------------------------------------------------------------------------- the ownership model
def cell_layer(scene, pos):
    """int64[n]: cz of the rule above - floor of the true fp64 division, clamped on the double, then cast."""
    z = np.asarray(pos, dtype=np.float64).reshape(-1, 3)[:, 2]
    with np.errstate(over="ignore"):
        c = np.floor((z - scene.off[2]) / scene.h)
    return np.clip(c, 0.0, float(scene.size[2] - 1)).astype(np.int64)


def owner(scene, pos, bounds):
    """int64[n]: the rank whose tile layers hold cz >> 3; x and y play no part, and every position has an owner."""
    return np.searchsorted(np.asarray(bounds), cell_layer(scene, pos) >> 3, side="right") - 1


def frozen_rows(pos, vel, dt=DT):
    """bool[n]: x + v dt is not finite in every coordinate - the tracer keeps its position and is counted as frozen."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ~np.isfinite(np.asarray(pos) + np.asarray(vel) * dt).all(axis=1)


def starts_outside(scene, pos):
    """bool[n]: the position is not inside the grid (the test of sc.classify, on the doubles). For such a START the reference is no
    reference: its march begins in a cell that does not exist and, when the bounce leaves the tracer below the grid's corner, its
    push-out converts a negative double to size_t, which C leaves undefined (oracle.c restates that line as it stands). The device
    clamps the cell index to 0 there and documents "the first move clamps them in" (include/libfluid_amd.h). The device tests hold
    these rows to what the contract names - a single-domain handle's plain call - and every other row to the oracle."""
    fi = (np.asarray(pos, dtype=np.float64).reshape(-1, 3) - np.array(scene.off)) / scene.h
    return ~((fi >= 0.0) & (fi < np.array(scene.size, dtype=np.float64))).all(axis=1)


def expected_move(scene, pos, vel, dt=DT):
    """Positions after one move: tc.advect_collide (the oracle) for the rows that move, the old position for the frozen ones."""
    pos, vel = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    out, moves = pos.copy(), ~frozen_rows(pos, vel, dt)
    if moves.any():
        out[moves] = tc.advect_collide(scene.size, scene.h, scene.off, scene.solid, pos[moves], vel[moves], dt)["collide"]
    return out


def expected_step(scene, pos, vel, cells, dt=DT):
    """(positions, velocities, types) after one step on the grid `cells` (scene A: sc.model is its grid's): the oracle's move, then
    the oracle's PIC transfer at the new positions."""
    assert scene is A
    new = expected_move(scene, pos, vel, dt)
    v, t, _ = sc.model(cells, new)
    return new, v, t


def rounds_model(scene, before, after, bounds):
    """The job's round count: the largest distance, in ranks, between a tracer's owner before and after the move."""
    a, b = owner(scene, before, bounds), owner(scene, after, bounds)
    return int(np.abs(b - a).max()) if len(a) else 0


def migrate_model(lists, dest, rounds):
    """The placement rule on id lists: per round every rank keeps the ids it owns in their order, then takes what the rank below
    sends up, then what the rank above sends down, each in the sender's order. lists[r]: the ids rank r holds, in storage order;
    dest[id]: the owner after the move. Returns (lists after, handed down per rank, handed up per rank, received per rank)."""
    n = len(lists)
    lists = [list(l) for l in lists]
    down, up, got = [0] * n, [0] * n, [0] * n
    for _ in range(rounds):
        stay = [[i for i in l if dest[i] == r] for r, l in enumerate(lists)]
        go_dn = [[i for i in l if dest[i] < r] for r, l in enumerate(lists)]
        go_up = [[i for i in l if dest[i] > r] for r, l in enumerate(lists)]
        for r in range(n):
            from_lo = go_up[r - 1] if r > 0 else []
            from_hi = go_dn[r + 1] if r + 1 < n else []
            lists[r] = stay[r] + from_lo + from_hi
            down[r] += len(go_dn[r])
            up[r] += len(go_up[r])
            got[r] += len(from_lo) + len(from_hi)
    return lists, down, up, got


# ---------------------------------------------------------------------------------------------------- group builders
def _movers(scene, rng, n, z_from, z_to, free):
    """n tracers that start at z in z_from and aim at z in z_to (cells), x and y inside `free` with a drift of up to 0.4 cells."""
    xy0 = np.stack([rng.uniform(*free[0], n), rng.uniform(*free[1], n)], axis=1)
    xy1 = xy0 + rng.uniform(-0.4, 0.4, (n, 2))
    start = scene.world(np.column_stack([xy0, rng.uniform(*z_from, n)]))
    end = scene.world(np.column_stack([xy1, rng.uniform(*z_to, n)]))
    return start, (end - start) / DT


def face_lattice(scene, face):
    """The z of the lattice point on the face, written the two ways a host writes it: offset + face * h and (offset / h + face) * h.
    Both were BUILT for cell `face`; which cell the fp64 division gives back is the division's business alone."""
    off, h = scene.off[2], scene.h
    return [off + face * h, (off / h + face) * h]


def _lattice(scene, rng, face, free):
    """For each lattice z of the face: two tracers that arrive there from below and two from above, with a start and a velocity for
    which z0 + v dt is the lattice z exactly (searched), and two that rest there."""
    pos, vel = [], []
    for z in face_lattice(scene, face):
        for sign in (-1.0, 1.0, -1.0, 1.0):
            for _ in range(1000):
                d = sign * rng.uniform(0.05, 0.9) * scene.h
                z0, v = z - d, d / DT
                if z0 + v * DT == z:
                    break
            else:
                z0, v = z, 0.0
            x, y = rng.uniform(*free[0]), rng.uniform(*free[1])
            pos.append([scene.off[0] + x * scene.h, scene.off[1] + y * scene.h, z0])
            vel.append([0.0, 0.0, v])
        for _ in range(2):
            pos.append([scene.off[0] + rng.uniform(*free[0]) * scene.h, scene.off[1] + rng.uniform(*free[1]) * scene.h, z])
            vel.append([0.0, 0.0, 0.0])
    return np.array(pos), np.array(vel)


def _groups_a():
    rng = np.random.default_rng(SEED)
    g = {}
    top = A.size[2] - 0.4  # (the last cell layer: above the face z = 16, under the skin of the wall)
    for face in A.faces:
        below, above = (face - 2.5, face - 0.3), (face + 0.15, min(face + 0.6, top))
        for n in GROUP_SIZES:
            g[f"face{face}_up_{n}"] = _movers(A, rng, n, below, above, A_FREE)
            g[f"face{face}_down_{n}"] = _movers(A, rng, n, above, below, A_FREE)
        g[f"lattice{face}"] = _lattice(A, rng, face, A_FREE)
    g["stay"] = _movers(A, rng, 700, (9.5, 14.0), (9.5, 14.0), A_FREE)
    g["stay_low"] = _movers(A, rng, 300, (1.5, 6.0), (1.5, 6.0), A_FREE)
    g["wall_lo"] = _movers(A, rng, 40, (0.5, 2.0), (-4.0, -3.0), A_FREE)       # the clamp, then the march stops at the wall z = 0
    g["wall_hi"] = _movers(A, rng, 40, (14.0, 15.5), (20.0, 21.0), A_FREE)     # ... at z = nz, across the face z = 16
    g["hop2_up"] = _movers(A, rng, 70, (1.0, 7.0), (16.15, top), A_FREE)        # two hops on [0, 1, 2, 3]
    g["hop2_down"] = _movers(A, rng, 70, (16.15, top), (1.0, 7.0), A_FREE)
    # NaN velocities beside both faces: frozen, they keep their position and their rank whatever the other components say
    zs = [f + d for f in A.faces for d in (-0.1, 0.1)]
    pos = A.world([[20.0 + i, 15.0, z] for i, z in enumerate(zs)] * 2)
    vel = np.array([[0.0, 0.0, np.nan]] * len(zs) + [[np.nan, 3.0, 900.0]] * len(zs))
    g["frozen"] = (pos, vel)
    # added outside the grid: below and above in z, in x only, and at +-1e300 - each has an owner, the first move clamps it in
    g["outside_z_lo"] = (A.world([[15.0 + i, 12.0, -2.5] for i in range(4)]), np.tile([[0.0, 0.0, 0.0], [1.0, -2.0, 30.0]], (2, 1)))
    g["outside_z_hi"] = (A.world([[15.0 + i, 13.0, 19.0] for i in range(4)]), np.tile([[0.0, 0.0, 0.0], [1.0, -2.0, -30.0]], (2, 1)))
    g["outside_x"] = (A.world([[-3.0, 14.0, 4.0], [-3.0, 14.0, 12.0], [44.0, 14.0, 16.5], [44.0, 15.0, 7.99]]), np.zeros((4, 3)))
    far = A.world([[16.0, 16.0, 5.0]] * 4)
    far[:, 2] = [-1e300, 1e300, -1e300, 1e300]
    g["far"] = (far, np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, -1.0]]))
    return g


def _groups_b():
    rng = np.random.default_rng(SEED + 1)
    g = {}
    top = B.size[2] - 0.4
    for k in (1, 2, 3, 4):  # k faces in one step, in the same step as the stayers and the one-face movers
        hi = (8.0 * k + 0.15, min(8.0 * k + 7.5, top))
        g[f"hop{k}_up"] = _movers(B, rng, 70, (0.5, 7.5), hi, B_FREE)
        g[f"hop{k}_down"] = _movers(B, rng, 70, (32.15, top), (32.0 - 8.0 * k + 0.5, 32.0 - 8.0 * k + 7.5), B_FREE)
    g["stay"] = _movers(B, rng, 300, (17.5, 22.0), (17.5, 22.0), B_FREE)
    # the unclamped move ends across the face z = 16, the bounce at the slab leaves the tracer on the side it came from
    g["bounce_up"] = _movers(B, rng, 66, (13.0, 14.5), (17.5, 19.0), B_OVER)
    g["bounce_down"] = _movers(B, rng, 66, (17.5, 19.0), (13.0, 14.5), B_OVER)
    g["wall_hi"] = _movers(B, rng, 20, (30.0, 31.5), (36.0, 37.0), B_FREE)
    return g


def _groups_grow():
    """Scene A. 1 500 tracers of the layers z < 8 all move up across the face z = 8; ONE tracer waits in z in [8, 16): on [0, 1, 3]
    and [0, 1, 2, 3] rank 0 loses all its tracers and rank 1 grows from 1 to 1 501, past its first 1 024; on [0, 1, 2, 3] rank 2
    owns nothing at the add."""
    rng = np.random.default_rng(SEED + 2)
    return {"one": _movers(A, rng, 1, (11.0, 12.0), (11.0, 12.0), A_FREE), "crowd": _movers(A, rng, 1500, (5.0, 7.5), (8.3, 10.0), A_FREE)}


RUNS = {
    "A": (A, _groups_a),
    "A_stay": (A, lambda: {k: v for k, v in _groups_a().items() if k.startswith("stay")}),
    "B": (B, _groups_b),
    "grow": (A, _groups_grow),
}
# what the runs are designed to do, per decomposition: the rounds of the first step ...
ROUNDS = {"A": {(0, 1, 3): 1, (0, 2, 3): 1, (0, 1, 2, 3): 2}, "A_stay": {(0, 1, 3): 0, (0, 2, 3): 0, (0, 1, 2, 3): 0},
          "B": {(0, 1, 2, 3, 4, 5): 4, (0, 2, 3, 5): 2, (0, 1, 5): 1}, "grow": {(0, 1, 3): 1, (0, 2, 3): 0, (0, 1, 2, 3): 1}}
# ... and in the run "grow" the ranks that own nothing at the add, that lose everything in the step, and that grow from 1 to 1 501
GROW_RANKS = {(0, 1, 3): dict(empty=[], emptied=[0], growing=[1]), (0, 2, 3): dict(empty=[1], emptied=[], growing=[]),
              (0, 1, 2, 3): dict(empty=[2], emptied=[0], growing=[1])}


@functools.lru_cache(maxsize=None)
def groups(run):
    """{name: (first row, rows)} of the run's tracers."""
    out, at = {}, 0
    for name, (pos, _) in RUNS[run][1]().items():
        out[name] = (at, len(pos))
        at += len(pos)
    return out


@functools.lru_cache(maxsize=None)
def tracers(run):
    """(scene, pos float64[n, 3], vel float64[n, 3]) of a run, read-only, in the order the job adds them."""
    scene, build = RUNS[run]
    g = build()
    pos = np.ascontiguousarray(np.concatenate([p for p, _ in g.values()]), dtype=np.float64)
    vel = np.ascontiguousarray(np.concatenate([v for _, v in g.values()]), dtype=np.float64)
    assert pos.shape == vel.shape and math.isfinite(float(np.abs(pos).max()))
    pos.setflags(write=False)
    vel.setflags(write=False)
    return scene, pos, vel


@functools.lru_cache(maxsize=None)
def moved(run):
    """The oracle's positions after the run's first move, computed once and shared; read-only."""
    scene, pos, vel = tracers(run)
    out = expected_move(scene, pos, vel)
    out.setflags(write=False)
    return out


def rows(run, group):
    at, n = groups(run)[group]
    return slice(at, at + n)


@functools.lru_cache(maxsize=None)
def stopped(run):
    """bool[n]: the tracers a march stops in the run's first move - tc.march_model, which tests/test_tracer_slab_cases.py pins to the
    oracle on these rows. Two kinds of rows it cannot speak for: the frozen ones do not march (False), and the group "far" starts at
    +-1e300, where march_model's floor is an exact Python integer and the reference's is an int conversion out of range; such a
    march starts outside the grid, so its first crossing meets "outside" and stops it (True). The oracle gives their positions."""
    scene, pos, vel = tracers(run)
    ask = ~frozen_rows(pos, vel)
    out = np.zeros(len(pos), dtype=bool)
    if "far" in groups(run):
        ask[rows(run, "far")] = False
        out[rows(run, "far")] = True
    out[ask] = tc.march_model(scene.size, scene.mask(), scene.h, scene.off, pos[ask], vel[ask], DT)[1]
    out.setflags(write=False)
    return out
