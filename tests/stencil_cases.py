"""Adversarial cell fields for the grid stages around the pressure solve (k_abits, k_rhs, k_apply_pressure, k_extrapolate,
lfa_apply_a and the solve itself), the staged run that records every one of those stages on the oracle or the reference, and an
fp64 numpy restatement of the two velocity stages that says, face by face, which rule applied.
Pure numpy, deterministic from a seed; every builder returns (size, parts, solid, meta) with
meta = dict(h=cell size, off=grid offset, rho=density, ...). The method is APIC throughout: the stencils do not depend on it.

What goes wrong in these kernels is case analysis, not arithmetic: a face is classified by the types of two cells, read from a
10 x 10 x 10 halo in LDS; a halo cell outside the particle tiles takes its type from the solid mask; "holds particles" (an
unknown) and "is fluid" are different things for a particle inside a solid cell. What the fields are for:
  maze       a wall with a one-cell doorway, a 3-D checkerboard of solids, a solid strip on the floor, particles in a random 45 %
             of ALL cells - solid ones included: hundreds of unknowns of type SOLID, every face class side by side, ragged tiles
  maze_h17,  the same field at cell_size 1.7 / 0.5, offset != 0, density 2: inv_h, coeff = dt / (rho h), a_scale
  maze_h05
  droplets   a pool and droplets in the air above it: single cells in tile interiors and in cell 7 of a tile (closed tiles),
             pairs across a tile face in x, y and z (open tiles), on every domain wall and in the max corner cell, a tile with
             exactly LFA_CLOSED_MAX_UNKNOWNS = 64 unknowns and one with 65, droplets on and under a solid cell, a particle
             inside an isolated solid cell
  sheets     one-cell-thick sheets of fluid normal to each axis at index 7 and at index 8 (the two sides of a tile face), one-cell
             lines along each axis through several tiles, sheets in the last layer of each axis of a ragged grid
  thin_*     grids of less than a tile across (two cells in x, in y), and 8 x 8 x 8 / 9 x 8 x 8 filled wall to wall but for
             the top layer: one full tile, and one full tile beside a one-cell sliver tile
  retyped    cells that hold particles but are typed AIR when the system is built: a host that edits the grid's types after the P2G
             (the reference calls back after the transfer and after gravity, src/simulation.cpp:67-80) gets there. Such a cell is
             an unknown that no neighbour counts as fluid: "holds particles" and "is fluid" come apart on the NON-solid side too
  walls_x,   fluid flush against a solid block that exactly fills the neighbouring tile, on both of its sides; that tile holds no
  walls_y,   particle, so the halo types of its cells come from the solid mask; solid cells in a tile far from any particle
  walls_z

Every field is well-posed by construction and tests/test_stencil_cases.py asserts it: no unknown is walled in on all six sides,
and no set of coupled unknowns is sealed off from the air (the reference returns NaN there - out of scope).
"""
import functools

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from oracle import loader as orc

APIC = 2
AIR, FLUID, SOLID = 1, 2, 4
DT = 0.01
OFF_H = (0.3, -0.2, 0.1)
CLOSED_MAX = 64  # LFA_CLOSED_MAX_UNKNOWNS (libfluid_amd/csrc/pcg.h)


# ---------------------------------------------------------------------------------------------------- construction
def _cells_of(mask):
    """int[k, 3] (x, y, z) of the set cells of a bool[nz, ny, nx] mask, in raw (x fastest) order."""
    z, y, x = np.nonzero(mask)
    return np.stack([x, y, z], axis=1)


def _mask_of(size, cells):
    nx, ny, nz = size
    m = np.zeros((nz, ny, nx), dtype=bool)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    m[cells[:, 2], cells[:, 1], cells[:, 0]] = True
    return m


def _box(lo, hi):
    """All cells lo <= c <= hi (inclusive)."""
    g = np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)


def _walled_in(size, fluid, solid):
    """Non-solid cells of `fluid` whose six neighbours are all solid or outside the grid: unknowns with an empty matrix row."""
    s = np.pad(solid, 1, constant_values=True)
    shut = s[1:-1, 1:-1, :-2] & s[1:-1, 1:-1, 2:] & s[1:-1, :-2, 1:-1] & s[1:-1, 2:, 1:-1] & s[:-2, 1:-1, 1:-1] & s[2:, 1:-1, 1:-1]
    return fluid & shut


def _finish(size, fluid, solid, rng, per_cell=(1, 3), h=1.0, off=(0.0, 0.0, 0.0), rho=1.0, vel=3.0, **meta):
    """1 - 3 particles (per_cell) in every cell of the bool mask `fluid`, away from the cell's faces, random v and C of scale `vel`;
    `solid`: bool mask or None. Positions are off + h * (position in cells)."""
    size = tuple(int(s) for s in size)
    cells = _cells_of(fluid)
    cnt = rng.integers(per_cell[0], per_cell[1] + 1, size=len(cells))
    rep = np.repeat(cells, cnt, axis=0)
    n = len(rep)
    pos = rep + rng.uniform(0.1, 0.9, size=(n, 3))
    parts = np.zeros(n, dtype=PARTICLE_DTYPE)
    parts["pos"] = np.asarray(off, dtype=np.float64)[None, :] + pos * h
    parts["old_pos"] = parts["pos"]
    parts["vel"] = rng.normal(size=(n, 3)) * vel
    for f in ("cx", "cy", "cz"):
        parts[f] = rng.normal(size=(n, 3)) * vel * 0.1 / h
    assert len(np.unique(parts["pos"], axis=0)) == n
    sc = None if solid is None or not solid.any() else _cells_of(solid).astype(np.int32)
    return size, parts, sc, dict(h=float(h), off=tuple(off), rho=float(rho), **meta)


def maze(h=1.0, off=(0.0, 0.0, 0.0), rho=1.0, seed=11):
    """21 x 13 x 18, ragged in all three axes. Solids: the plane x = 8 but for the doorway (8, 6, 9); (x + y + z) odd for x >= 14;
    the strip 2 <= x <= 6 of the floor y = 0. Particles in a random 45 % of all cells, solid or not - except the non-solid cells of
    the checkerboard that are walled in on all six sides (their matrix row would be empty)."""
    size = (21, 13, 18)
    nx, ny, nz = size
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    solid = (x == 8) | ((x >= 14) & ((x + y + z) % 2 == 1)) | ((y == 0) & (x >= 2) & (x <= 6))
    solid[9, 6, 8] = False
    fluid = rng.random((nz, ny, nx)) < 0.45
    fluid &= ~_walled_in(size, fluid, solid)
    return _finish(size, fluid, solid, rng, h=h, off=off, rho=rho, doorway=(8, 6, 9))


def droplets(seed=22):
    """40 x 16 x 16 = 5 x 2 x 2 tiles: a pool two cells deep wall to wall, and in the tile layer above it the droplets listed in
    meta["groups"] (name -> cells). Tiles (tx, 1, tz): (0,1,0) singles in the interior and in cell 7 along x and z - closed;
    (1,1,0) | (2,1,0) a pair across x = 15 | 16, (1,1,0) | (1,1,1) a pair across z = 7 | 8, (3,0,0) | (3,1,0) a pair across y = 7 | 8 -
    open; (3,1,1) a 4 x 4 x 4 block = 64 unknowns - closed; (2,1,1) such a block and one more cell = 65 - not closed; droplets on
    the walls x = 0, x = 39, y = 15, z = 0, z = 15 and in the corner cell (39, 15, 15); a solid cell with a droplet on top of it
    and one under it; a solid cell on its own with a particle inside."""
    size = (40, 16, 16)
    rng = np.random.default_rng(seed)
    groups = {
        "pool": _box((0, 0, 0), (39, 1, 15)),
        "interior": np.array([(2, 10, 2), (5, 12, 5), (3, 13, 6)]),
        "cell7": np.array([(7, 10, 4), (4, 11, 7)]),
        "straddle_x": np.array([(15, 12, 5), (16, 12, 5)]),
        "straddle_y": np.array([(28, 7, 4), (28, 8, 4)]),
        "straddle_z": np.array([(12, 12, 7), (12, 12, 8)]),
        "walls": np.array([(0, 11, 11), (39, 10, 10), (35, 15, 3), (34, 10, 0), (2, 11, 15)]),
        "corner": np.array([(39, 15, 15)]),
        "tile64": _box((25, 9, 9), (28, 12, 12)),
        "tile65": np.concatenate([_box((17, 9, 9), (20, 12, 12)), np.array([(22, 14, 14)])]),
        "on_solid": np.array([(37, 12, 4), (37, 10, 4)]),
        "in_solid": np.array([(36, 12, 12)]),
    }
    solid = _mask_of(size, [(37, 11, 4), (36, 12, 12)])
    fluid = _mask_of(size, np.concatenate(list(groups.values())))
    return _finish(size, fluid, solid, rng, groups={k: [tuple(int(a) for a in c) for c in v] for k, v in groups.items()},
                   tile64=(3, 1, 1), tile65=(2, 1, 1))


def sheets(seed=33):
    """21 x 13 x 18 (3 x 2 x 3 tiles, the last one ragged in every axis). One-cell-thick sheets normal to x at x = 7 and x = 8, to y at
    y = 7 and y = 8, to z at z = 7 and z = 8 (apart from each other); sheets in the last layers x = 20, y = 12, z = 17; lines along
    x, y and z through all tiles of their axis; a solid cell before and behind a sheet of each normal."""
    size = (21, 13, 18)
    rng = np.random.default_rng(seed)
    parts = [
        _box((7, 1, 1), (7, 5, 6)), _box((8, 7, 1), (8, 11, 6)),          # normal x, the two sides of the tile face 7 | 8
        _box((10, 7, 9), (18, 7, 12)), _box((10, 8, 14), (18, 8, 16)),    # normal y
        _box((1, 1, 7), (5, 11, 7)), _box((10, 1, 8), (18, 5, 8)),        # normal z
        _box((20, 1, 1), (20, 11, 6)), _box((1, 12, 9), (6, 12, 16)), _box((8, 10, 17), (18, 12, 17)),  # the last layers
        _box((0, 3, 15), (20, 3, 15)), _box((19, 0, 12), (19, 12, 12)), _box((13, 10, 0), (13, 10, 17)),  # lines
    ]
    solid = _mask_of(size, [(8, 3, 3), (6, 4, 4), (9, 9, 3), (7, 8, 4), (12, 8, 10), (14, 6, 11), (3, 5, 8), (4, 6, 6),
                            (12, 9, 15), (15, 7, 15), (14, 3, 9), (16, 2, 7)])
    fluid = _mask_of(size, np.concatenate(parts)) & ~solid
    return _finish(size, fluid, solid, rng)


def thin(size, seed=44):
    """Grids below one tile - (2, 9, 17) and (17, 2, 9) have an axis of two cells, (5, 5, 5) fits a tile with room to spare -: a random
    60 % of the cells hold particles, three cells are solid (one of them holds particles)."""
    nx, ny, nz = size
    rng = np.random.default_rng(seed + sum(size))
    fluid = rng.random((nz, ny, nx)) < 0.6
    solid = np.zeros_like(fluid)
    pick = rng.choice(nx * ny * nz, size=3, replace=False)
    solid.reshape(-1)[pick] = True
    fluid.reshape(-1)[pick[1:]] = False
    fluid.reshape(-1)[pick[0]] = True
    fluid &= ~_walled_in(size, fluid, solid)
    return _finish(size, fluid, solid, rng)


def full(size, seed=55):
    """(8, 8, 8): one full tile; (9, 8, 8): a full tile and a one-cell sliver tile. Filled wall to wall but for the top layer, one
    air bubble (a face from an air cell up into fluid) and one solid cell."""
    nx, ny, nz = size
    rng = np.random.default_rng(seed + sum(size))
    fluid = np.ones((nz, ny, nx), dtype=bool)
    fluid[:, ny - 1, :] = False
    fluid[3, 2, 5] = False  # the bubble
    solid = _mask_of(size, [(2, 4, 4)])
    fluid &= ~solid
    return _finish(size, fluid, solid, rng)


def retyped(seed=77):
    """9 x 8 x 7: a random 60 % of the cells hold particles, three cells are solid, and eight cells that hold particles are re-typed AIR
    after gravity (meta["retype_air"], applied by staged() and by the GPU tests)."""
    size = (9, 8, 7)
    nx, ny, nz = size
    rng = np.random.default_rng(seed)
    fluid = rng.random((nz, ny, nx)) < 0.6
    solid = np.zeros_like(fluid)
    pick = rng.choice(nx * ny * nz, size=3, replace=False)
    solid.reshape(-1)[pick] = True
    fluid.reshape(-1)[pick] = False
    fluid &= ~_walled_in(size, fluid, solid)
    air = rng.choice(np.flatnonzero(fluid.reshape(-1)), size=8, replace=False)
    return _finish(size, fluid, solid, rng, retype_air=np.sort(air))


def walls(axis, seed=66):
    """40 x 9 x 10 with the axes rotated so that `axis` is the long one: tile 1 along it is solid from end to end (cells 8 .. 15, and 0 .. 7
    of the other two axes: exactly one tile; the sliver tiles beside it stay open) and holds no particle; fluid lies flush against
    it in cells 5 .. 7 and 16 .. 18, across 1 .. 8 of the next axis - up to the domain's max face, into the sliver tile - and 1 .. 6 of
    the third; a few solid cells in tile 4 along the axis, which is no neighbour of any particle tile."""
    rng = np.random.default_rng(seed + axis)
    perm = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][axis]  # role -> axis: long, next, third
    dims = (40, 9, 10)
    size = [0, 0, 0]
    for role, a in enumerate(perm):
        size[a] = dims[role]

    def place(cells):
        out = np.empty_like(cells)
        for role, a in enumerate(perm):
            out[:, a] = cells[:, role]
        return out

    block = place(_box((8, 0, 0), (15, 7, 7)))
    far = place(np.array([(34, 2, 3), (35, 2, 3), (37, 6, 5), (39, 8, 9)]))
    wet = place(np.concatenate([_box((5, 1, 1), (7, 8, 6)), _box((16, 1, 1), (18, 8, 6))]))
    solid = _mask_of(size, np.concatenate([block, far]))
    fluid = _mask_of(size, wet)
    return _finish(size, fluid, solid, rng, axis=axis, block_tile=tuple(int(t) for t in place(np.array([[1, 0, 0]]))[0]),
                   far_tile=tuple(int(t) for t in place(np.array([[4, 0, 0]]))[0]))


CASES = {
    "maze": maze,
    "maze_h17": lambda: maze(h=1.7, off=OFF_H, rho=2.0),
    "maze_h05": lambda: maze(h=0.5, off=OFF_H, rho=2.0),
    "droplets": droplets,
    "sheets": sheets,
    "thin_2_9_17": lambda: thin((2, 9, 17)),
    "thin_17_2_9": lambda: thin((17, 2, 9)),
    "thin_5_5_5": lambda: thin((5, 5, 5)),
    "thin_8_8_8": lambda: full((8, 8, 8)),
    "thin_9_8_8": lambda: full((9, 8, 8)),
    "retyped": retyped,
    "walls_x": lambda: walls(0),
    "walls_y": lambda: walls(1),
    "walls_z": lambda: walls(2),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def build(name):
    """(size, parts, solid, meta) of a case; cached - callers copy `parts` before they change it."""
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


# ---------------------------------------------------------------------------------------------------- the staged run
def probe(n):
    return np.sin(np.arange(n) * 0.37) + 0.25  # (tests/util.py: staged_cpu_run)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def cpu_sim(name, kind="oracle"):
    size, parts, solid, meta = build(name)
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=APIC, blending=1.0, density=meta["rho"], kind=kind)
    if solid is not None:
        s.set_solid_cells(solid)
    s.set_particles(parts)
    return s


def staged(name, kind="oracle", rounded=False):
    """hash, P2G, gravity; build_system (A bits, b, an apply_a probe); solve; apply_pressure; the extrapolation with 1 and with 3
    sweeps, each from the same applied grid. `rounded`: the grid after gravity and the applied grid are rounded to fp32 before the
    next stage reads them - the stages of a device that was handed exactly those grids (grav_vel and apply_vel are the rounded
    ones then: the INPUTS of the next stage)."""
    s = cpu_sim(name, kind)
    out = {}
    s.hash()
    out["fluid_cells"] = s.fluid_cells()
    out["counts"] = s.space_hash()[1].astype(np.uint32)
    s.p2g()
    s.add_gravity(DT)
    cells = s.cells()
    out["p2g_type"] = cells["type"].copy()
    if rounded:
        cells["vel"] = f32(cells["vel"])
    edit = build(name)[3].get("retype_air")
    if edit is not None:  # the host's edit between gravity and the solve
        cells["type"][edit] = AIR
    if rounded or edit is not None:
        s.set_cells(cells)
    out["grav_vel"], out["type"] = cells["vel"].copy(), cells["type"].copy()
    s.build_system(DT)
    out["abits"], out["b"] = s.abits(), s.b()
    out["Aprobe"] = s.apply_a(probe(len(out["b"])))
    p, res, it = s.solve(DT)
    out["p"], out["residual"], out["iters"] = p.copy(), np.float64(res), np.int64(it)
    s.apply_pressure(DT, p)
    cells = s.cells()
    out["apply_exact"] = cells["vel"].copy()
    if rounded:
        cells["vel"] = f32(cells["vel"])
    out["apply_vel"] = cells["vel"].copy()
    assert np.array_equal(cells["type"], out["type"])
    for sweeps in (1, 3):
        s.set_cells(cells)
        s.set_extrapolation_iterations(sweeps)
        s.extrapolate()
        after = s.cells()
        out[f"extrap{sweeps}_vel"] = after["vel"].copy()
        assert np.array_equal(after["type"], out["type"])
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_stages(name, rounded=False):
    """staged(name, "oracle", rounded), computed once and shared; the arrays are read-only."""
    out = staged(name, "oracle", rounded)
    for v in out.values():
        if isinstance(v, np.ndarray) and v.ndim:
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- fp64 restatements
def _grid(size, a):
    nx, ny, nz = size
    return np.asarray(a).reshape((nz, ny, nx) + np.asarray(a).shape[1:])


def _nb(a, d, sign, fill):
    """out[c] = a[c + sign e_d], `fill` where that cell lies outside the grid; a is [nz, ny, nx, ...], d = 0, 1, 2 for x, y, z."""
    ax = 2 - d
    out = np.full_like(a, fill)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[ax], dst[ax] = (slice(1, None), slice(0, -1)) if sign > 0 else (slice(0, -1), slice(1, None))
    out[tuple(dst)] = a[tuple(src)]
    return out


FACE_CLASSES = ("unknown-fluid", "unknown-air", "unknown-solid", "unknown-outside", "air-unknown", "solid-unknown")


def apply_pressure_faces(size, types, fluid_cells, vel_in, p, coeff):
    """pressure_solver::apply_pressure (src/pressure_solver.cpp:73-148) face by face, in fp64 with the reference's operations: the +d
    face of cell c (neighbour n = c + e_d) gets, c before n,
        c an unknown:  n not solid (in the grid) ? u -= coeff ((n fluid ? p_n : 0) - p_c) : u = 0
        n an unknown:  c air ? u -= coeff p_n : (c solid ? u = 0 : nothing)
    Returns (vel_out float64[ncells, 3], cls: class name -> bool[ncells, 3], scale float64[ncells, 3]) with
    scale = |u_in| + coeff (|p_c| + |p_n|). The classes name the first rule that fires for the face; a face in none is untouched.
    cls["computed-twice"] (no class of its own, not in FACE_CLASSES): both rules compute - c is an unknown typed AIR and n an unknown,
    which only a grid with edited types has."""
    nx, ny, nz = size
    nc = nx * ny * nz
    unk = np.zeros(nc, dtype=bool)
    unk[np.asarray(fluid_cells, dtype=np.int64)] = True
    pc = np.zeros(nc)
    pc[np.asarray(fluid_cells, dtype=np.int64)] = p
    t3, u3, p3 = _grid(size, types), _grid(size, unk), _grid(size, pc)
    out = np.array(vel_in, dtype=np.float64)
    cls = {k: np.zeros((nc, 3), dtype=bool) for k in FACE_CLASSES}
    scale = np.zeros((nc, 3))
    twice = np.zeros((nc, 3), dtype=bool)
    for d in range(3):
        tn = _nb(t3, d, +1, 0).reshape(-1)  # 0: outside the grid (solid to the stencil, src/mac_grid.cpp:26-31)
        un = _nb(u3, d, +1, False).reshape(-1)
        pn = _nb(p3, d, +1, 0.0).reshape(-1)
        tc, uc = t3.reshape(-1), u3.reshape(-1)
        val = out[:, d].copy()
        open_ = uc & (tn != SOLID) & (tn != 0)
        val = np.where(open_, val - coeff * (np.where(tn == FLUID, pn, 0.0) - pc), val)
        val = np.where(uc & ~open_, 0.0, val)
        val = np.where(un & (tc == AIR), val - coeff * pn, val)
        val = np.where(un & (tc == SOLID), 0.0, val)
        out[:, d] = val
        cls["unknown-fluid"][:, d] = uc & (tn == FLUID)
        cls["unknown-air"][:, d] = uc & (tn == AIR)
        cls["unknown-solid"][:, d] = uc & (tn == SOLID)
        cls["unknown-outside"][:, d] = uc & (tn == 0)
        cls["air-unknown"][:, d] = ~uc & un & (tc == AIR)
        cls["solid-unknown"][:, d] = ~uc & un & (tc == SOLID)
        twice[:, d] = uc & un & (tc == AIR)
        scale[:, d] = np.abs(vel_in[:, d]) + coeff * (np.abs(pc) + np.abs(pn))
    cls["computed-twice"] = twice
    return out, cls, scale


def extrapolate_sweeps(size, types, fluid_cells, vel_in, sweeps):
    """simulation::_extrapolate_velocities (src/simulation.cpp:685-754) in fp64, the neighbours added in the reference's order
    (-x, +x, -y, +y, -z, +z). Returns (vel_out, written bool[ncells, 3], count int[ncells] - valid neighbours of a cell in the sweep
    that made it valid, 0 elsewhere -, born int[ncells] - that sweep, 1-based; 0: an unknown, -1: never reached -,
    bound float64[ncells, 3] - the rounding unit of each written component: max |valid neighbour component|, plus, for a later
    sweep, the largest unit among the neighbours it averaged (their own error is passed on, at most undiminished))."""
    nx, ny, nz = size
    nc = nx * ny * nz
    valid = np.zeros(nc, dtype=bool)
    valid[np.asarray(fluid_cells, dtype=np.int64)] = True
    valid = _grid(size, valid)
    t3 = _grid(size, types)
    vel = _grid(size, np.array(vel_in, dtype=np.float64))
    written = np.zeros((nz, ny, nx, 3), dtype=bool)
    count = np.zeros((nz, ny, nx), dtype=np.int64)
    born = np.where(valid, 0, -1)
    unit = np.zeros((nz, ny, nx, 3))
    for it in range(sweeps):
        cnt = np.zeros((nz, ny, nx), dtype=np.int64)
        total = np.zeros((nz, ny, nx, 3))
        biggest = np.zeros((nz, ny, nx, 3))
        passed = np.zeros((nz, ny, nx, 3))
        tpos = np.full((nz, ny, nx, 3), SOLID)
        for d in range(3):
            for sign in (-1, +1):
                ok = _nb(valid, d, sign, False)
                v = _nb(vel, d, sign, 0.0)
                total = total + np.where(ok[..., None], v, 0.0)
                biggest = np.maximum(biggest, np.where(ok[..., None], np.abs(v), 0.0))
                passed = np.maximum(passed, np.where(ok[..., None], _nb(unit, d, sign, 0.0), 0.0))
                cnt = cnt + ok
                if sign > 0:
                    tpos[..., d] = np.where(ok, _nb(t3, d, +1, SOLID), SOLID)
        fresh = ~valid & (cnt > 0)
        write = fresh[..., None] & (t3[..., None] == tpos)
        vel = np.where(write, total / np.maximum(cnt, 1)[..., None], vel)
        unit = np.where(write, biggest + passed, unit)
        written |= write
        count = np.where(fresh, cnt, count)
        born = np.where(fresh, it + 1, born)
        valid = valid | fresh
    return vel.reshape(nc, 3), written.reshape(nc, 3), count.reshape(nc), born.reshape(nc), unit.reshape(nc, 3)


def coeff_of(meta):
    return DT / (meta["rho"] * meta["h"])  # src/pressure_solver.cpp:74


def unknowns_per_tile(size, fluid_cells):
    """tile (tx, ty, tz) -> number of unknowns in it."""
    nx, ny, nz = size
    r = np.asarray(fluid_cells, dtype=np.int64)
    t = np.stack([(r % nx) // 8, ((r // nx) % ny) // 8, (r // (nx * ny)) // 8], axis=1)
    keys, n = np.unique(t, axis=0, return_counts=True)
    return {tuple(int(a) for a in k): int(c) for k, c in zip(keys, n)}


def couplings_across_tile_faces(size, types, fluid_cells, abits):
    """Set of tiles that have an unknown coupled to an unknown of another tile (a +d bit of the matrix whose two cells lie in different
    tiles marks both)."""
    nx, ny, nz = size
    r = np.asarray(fluid_cells, dtype=np.int64)
    c = np.stack([r % nx, (r // nx) % ny, r // (nx * ny)], axis=1)
    out = set()
    for d in range(3):
        on = ((np.asarray(abits) >> (3 + d)) & 1).astype(bool) & (c[:, d] % 8 == 7)
        for cell in c[on]:
            other = cell.copy()
            other[d] += 1
            out.add(tuple(int(a) for a in cell // 8))
            out.add(tuple(int(a) for a in other // 8))
    return out
