"""Sequences of pressure systems for ONE solver handle, each step with the oracle's cold fp64 answer. Pure numpy plus the oracle.

A simulation solves a new system on the same handle every step, and the solver keeps state from one solve to the next: the
epochs that decide whether a solve starts from the previous pressure (per handle and per tile), `warm_started`, `last_rhs_zero`,
`pcg_poisoned`, `last_iters`, the multigrid hierarchy with its compacted level-0 list, the closed-tile flags. The sequences here walk
through the combinations of that state; the oracle knows no state - it solves every step from p = 0.

Everything is built from stencil_cases.build("droplets") (40 x 16 x 16 = 5 x 2 x 2 tiles). Fields are particle subsets of it:
  A  the field as it is: 20 particle tiles, 5 of them closed - (0,1,0), (0,1,1), (3,1,1), (4,1,0), (4,1,1)
  B  A without the groups `interior` and `cell7` - tile (0,1,0) leaves the particle set, 19 remain - and with 1 - 3 new particles in
     cell (29, 9, 9) (group `b_extra`): tile (3,1,1) holds 65 coupled unknowns and is no longer closed
  S  spray: A without `pool`, `straddle_x`, `straddle_y`, `straddle_z` and `tile65`: 5 tiles, every one closed - the PCG has no tile
     to iterate over
A step is Step(field, f, nan): the oracle's grid after P2G and gravity for that field, times f, rounded to fp32 - the very grid a
device is handed with upload_cells -, with one face velocity replaced by NaN where `nan` = (x, y, z) names a cell (its +x face).
The oracle is handed the same grid with set_cells and solves it from scratch. f = 0 gives a zero right-hand side.

`hot` is no sequence of uploaded grids: two passes of the whole hot path (hash, P2G, gravity, solve, apply, extrapolate, G2P) from a
field's particles, recorded stage by stage on the oracle (hot_steps).
"""
import collections
import functools

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from oracle import loader as orc
from tests import stencil_cases as sc

DT = sc.DT
P_REL = 1e-4  # the pressure bar of tests/test_gpu_parity.py (restated: that module is a GPU module)
FIELDS = ("A", "B", "S")
B_EXTRA_CELL = (29, 9, 9)
DROPPED = {"A": (), "B": ("interior", "cell7"), "S": ("pool", "straddle_x", "straddle_y", "straddle_z", "tile65")}
TILES = {"A": 20, "B": 19, "S": 5}
CLOSED_A = {(0, 1, 0), (0, 1, 1), (3, 1, 1), (4, 1, 0), (4, 1, 1)}
NAN_CELL = {"A": (20, 0, 4), "S": (26, 10, 10)}  # a pool cell inside tile (2,0,0); a cell of `tile64` inside tile (3,1,1)
NAN_TILE = {"A": (2, 0, 0), "S": (3, 1, 1)}

Step = collections.namedtuple("Step", "field f nan", defaults=(1.0, None))

SEQUENCES = {
    "repeat": [Step("A"), Step("A"), Step("A", 1.001), Step("A", -0.5)],
    "rest_A": [Step("A"), Step("A", 0.0), Step("A", 0.0), Step("A")],
    "rest_S": [Step("S"), Step("S", 0.0), Step("S", 0.0), Step("S")],
    "come_and_go": [Step("A"), Step("B"), Step("A"), Step("S"), Step("A")],
    "capped": [Step("A"), Step("A")],             # max_iterations 3, then 200
    "switch": [Step("A"), Step("A", 1.001), Step("A"), Step("A")],  # the preconditioner / dtype changes between the steps
    "nan_A": [Step("A", 1.0, NAN_CELL["A"]), Step("A")],
    "nan_S": [Step("S", 1.0, NAN_CELL["S"]), Step("S")],
}
WARM_DISCRIMINATING = ("repeat", "come_and_go", "hot_A", "hot_S")  # (hot_*: hot_steps, not SEQUENCES)


# ---------------------------------------------------------------------------------------------------- fields
@functools.lru_cache(maxsize=None)
def particles(field):
    """The field's particles (read-only)."""
    size, parts, solid, meta = sc.build("droplets")
    drop = {c for k in DROPPED[field] for c in meta["groups"][k]}
    cell = np.floor(parts["pos"]).astype(np.int64)  # (h = 1, offset 0)
    keep = np.array([tuple(int(a) for a in c) not in drop for c in cell])
    out = parts[keep].copy()
    if field == "B":
        rng = np.random.default_rng(2209)
        n = int(rng.integers(1, 4))
        extra = np.zeros(n, dtype=PARTICLE_DTYPE)
        extra["pos"] = np.asarray(B_EXTRA_CELL, dtype=np.float64)[None, :] + rng.uniform(0.1, 0.9, size=(n, 3))
        extra["old_pos"] = extra["pos"]
        extra["vel"] = rng.normal(size=(n, 3)) * 3.0
        for f in ("cx", "cy", "cz"):
            extra[f] = rng.normal(size=(n, 3)) * 0.3
        out = np.concatenate([out, extra])
    out.setflags(write=False)
    return out


def groups(field):
    """name -> cells of the droplet groups the field holds."""
    meta = sc.build("droplets")[3]
    out = {k: v for k, v in meta["groups"].items() if k not in DROPPED[field]}
    if field == "B":
        out["b_extra"] = [B_EXTRA_CELL]
    return out


def _oracle(field):
    size, _, solid, meta = sc.build("droplets")
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=sc.APIC, blending=1.0, density=meta["rho"])
    s.set_solid_cells(solid)
    s.set_particles(particles(field))
    return s


@functools.lru_cache(maxsize=None)
def _after_gravity(field):
    """(the oracle, binned, for set_cells / build_system / solve; its cells after P2G and gravity)."""
    s = _oracle(field)
    s.hash()
    s.p2g()
    s.add_gravity(DT)
    cells = s.cells()
    cells.setflags(write=False)
    return s, cells


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray) and v.ndim:
            v.setflags(write=False)
    return out


def _tiles_of(size, fluid_cells, abits):
    per = sc.unknowns_per_tile(size, fluid_cells)
    coupled = sc.couplings_across_tile_faces(size, None, fluid_cells, abits)
    return per, {t for t, k in per.items() if k <= sc.CLOSED_MAX and t not in coupled}


@functools.lru_cache(maxsize=None)
def solved(step):
    """The oracle's cold solve of a step: dict(vel, type - the grid to upload -, fluid_cells, abits, b, p, residual, iters, tiles -
    tile -> unknowns -, closed - the set of closed tiles). Shared and read-only. A NaN step is built but not solved (p is None)."""
    size = sc.build("droplets")[0]
    s, base = _after_gravity(step.field)
    nx, ny, nz = size
    cells = base.copy()
    cells["vel"] = sc.f32(base["vel"] * step.f)
    if step.nan is not None:
        x, y, z = step.nan
        cells["vel"][x + nx * (y + ny * z), 0] = np.nan
    s.set_cells(cells)
    s.build_system(DT)
    out = dict(vel=cells["vel"].copy(), type=cells["type"].copy(), fluid_cells=s.fluid_cells(), abits=s.abits(), b=s.b())
    if step.nan is None:
        p, res, it = s.solve(DT)
        out.update(p=p.copy(), residual=float(res), iters=int(it))
    else:
        out.update(p=None, residual=None, iters=None)
    out["tiles"], out["closed"] = _tiles_of(size, out["fluid_cells"], out["abits"])
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def hot_steps(field, steps=2):
    """`steps` passes of the hot path from the field's particles on the oracle, stage by stage (what CpuSim.hot_step does in one
    call: tests/test_solve_sequence_cases.py holds the two together). Per step the dict of solved() without vel / type, and
    grid_vel (after the extrapolation), parts (after the G2P, sorted by position)."""
    size = sc.build("droplets")[0]
    s = _oracle(field)
    out = []
    for _ in range(steps):
        s.hash()
        s.p2g()
        s.add_gravity(DT)
        s.build_system(DT)
        rec = dict(fluid_cells=s.fluid_cells(), abits=s.abits(), b=s.b())
        p, res, it = s.solve(DT)
        rec.update(p=p.copy(), residual=float(res), iters=int(it))
        s.apply_pressure(DT, p)
        s.extrapolate()
        s.g2p()
        rec["grid_vel"] = s.cells()["vel"].copy()
        after = s.particles()
        rec["parts"] = after[np.lexsort((after["pos"][:, 2], after["pos"][:, 1], after["pos"][:, 0]))]
        rec["tiles"], rec["closed"] = _tiles_of(size, rec["fluid_cells"], rec["abits"])
        out.append(_freeze(rec))
    s.close()
    return tuple(out)


def records(name):
    """The per-step oracle records of a sequence: SEQUENCES[name] through solved(), or hot_A / hot_S through hot_steps()."""
    if name.startswith("hot_"):
        return list(hot_steps(name[4:]))
    return [solved(st) for st in SEQUENCES[name]]


def fields_of(name):
    return [name[4:]] * 2 if name.startswith("hot_") else [st.field for st in SEQUENCES[name]]


# ---------------------------------------------------------------------------------------------------- helpers
def group_indices(field, rec):
    """name -> indices into the step's unknowns (searchsorted on its fluid_cells) of every group the field holds."""
    nx, ny, nz = sc.build("droplets")[0]
    fc = rec["fluid_cells"].astype(np.int64)
    out = {}
    for k, cells in groups(field).items():
        raw = np.array([cx + nx * (cy + ny * cz) for cx, cy, cz in cells], dtype=np.int64)
        at = np.searchsorted(fc, raw)
        assert np.array_equal(fc[at], raw), k
        out[k] = at
    return out


def tile_of_unknowns(rec):
    """int[n, 3]: the tile of every unknown of a step."""
    nx, ny, nz = sc.build("droplets")[0]
    r = rec["fluid_cells"].astype(np.int64)
    return np.stack([(r % nx) // 8, ((r // nx) % ny) // 8, (r // (nx * ny)) // 8], axis=1)


def closed_groups(field, rec):
    """The groups all of whose unknowns lie in tiles closed in this step."""
    t = tile_of_unknowns(rec)
    return {k: at for k, at in group_indices(field, rec).items() if all(tuple(int(a) for a in t[i]) in rec["closed"] for i in at)}


def wrong_warm_closed(rec, prev):
    """The fp64 pressure of step `rec` a solver returns that starts the step from the previous pressure and hands the closed tiles
    the residual b - A p_prev in place of b: p_true - p_prev on the tiles closed in this step that took part in the previous one
    (`prev`: that step's record; p_prev is 0 in a cell that was no unknown then), p_true everywhere else. p_prev is the oracle's
    answer to the previous step, not a chain of wrong ones: each step's mistake is taken on its own."""
    t = tile_of_unknowns(rec)
    hit = np.array([tuple(int(a) for a in x) in rec["closed"] and tuple(int(a) for a in x) in prev["tiles"] for x in t])
    fc, pfc = rec["fluid_cells"].astype(np.int64), prev["fluid_cells"].astype(np.int64)
    at = np.minimum(np.searchsorted(pfc, fc), len(pfc) - 1)
    p_prev = np.where(pfc[at] == fc, prev["p"][at], 0.0)
    return np.where(hit, rec["p"] - p_prev, rec["p"])
