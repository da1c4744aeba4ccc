"""Fields and right-hand sides for the multigrid V-cycle (tests/vcycle_model.py against libfluid_amd/csrc/mg.hip).

Reused, unchanged, from tests/stencil_cases.py: maze, maze_h17, maze_h05 (a_scale != 1, offset, density 2), droplets and sheets,
thin_2_9_17 and thin_8_8_8 (a single level), retyped, walls_x. The fields A, B and S of tests/solve_sequence_cases.py for set-ups in
sequence. New here:

  terraces  70 x 37 x 53 = 9 x 5 x 7 tiles, five levels (35 x 19 x 27, 18 x 10 x 14, 9 x 5 x 7, 5 x 3 x 4); ragged on level 0; odd
            dimensions on levels 0, 1 and 3, so coarse cells of three levels have children outside the finer grid. A pool wall to wall
            whose surface steps down along x (heights 25, 18, 11, 6: the Dirichlet surface moves inwards by another amount per level);
            solid pillars one and two cells wide, aligned with the coarse cells and not; a column of fluid up to the last layer y = 36;
            a solid shelf with a film ONE cell thick on it, beside the pool (its level-1 cells are AIR: the parent tile is pruned while
            the neighbouring tile is active); spray: a droplet behind a one-cell wall whose coarse cell is FLUID in an INACTIVE level-1
            tile beside an active one (`behind_wall`), a droplet in a walled box in the pool whose coarse cell is an unknown of an ACTIVE
            level-1 tile in the octant of a closed - inactive - child (`in_box`), two single-cell droplets (one in cell 7 of its tile),
            and a pair across a tile face, which stays open. Variants: terraces_shifted - the fluid moved by 8 cells along x;
            terraces_half - x >= 35 removed; terraces_half_solid - that with another solid mask
  plate     520 x 8 x 520, fluid in y = 0, 1 wall to wall, one particle per cell: the smallest field whose level 1 has more than 1 024
            active tiles (4 225 on level 0, 1 089 on level 1): the wave-per-tile coarse kernels

system(name) is the level-0 system of a field from the oracle (hash, P2G, gravity, build_system on the fp32-rounded grid; `plate`: no
solve, no P2G velocities - its particles are at rest and one to a cell) and model(name) the hierarchy built from it;
rhs(name) the right-hand sides, deterministic: a normal random vector, the case's own b, A (smooth field), and up to 24 unit
impulses at designed unknowns (label -> vector).
"""
import functools

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from oracle import loader as orc
from tests import solve_sequence_cases as ssc
from tests import stencil_cases as sc
from tests import vcycle_model as vm

DT = sc.DT
REUSED = ("maze", "maze_h17", "maze_h05", "droplets", "sheets", "thin_2_9_17", "thin_8_8_8", "retyped", "walls_x")
SEQUENCE_FIELDS = ("A", "B", "S")
FIELDS = REUSED + ("terraces",)  # the fields every comparison runs on (plate has a test of its own)
TERRACES_SIZE = (70, 37, 53)
PLATE_SIZE = (520, 8, 520)
PILLARS = {"aligned": ((10, 11), (10, 11)), "unaligned": ((33, 34), (13, 14))}  # (x0, x1), (z0, z1): two cells wide, y = 0 .. 25


# ---------------------------------------------------------------------------------------------------- terraces
def _terraces_masks():
    nx, ny, nz = TERRACES_SIZE
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    height = np.select([x < 16, x < 32, x < 48], [25, 18, 11], 6)
    fluid = y < height
    solid = np.zeros_like(fluid)
    groups = {}
    # pillars: two wide and aligned, one wide, two wide and not aligned, one by two (PILLARS names two of them for the impulses)
    for (x0, x1), (z0, z1) in (((10, 11), (10, 11)), ((21, 21), (21, 21)), ((33, 34), (13, 14)), ((40, 40), (18, 19)), ((57, 58), (44, 44))):
        solid[z0:z1 + 1, 0:26, x0:x1 + 1] = True
    # the column up to the last layer of y, four cells wide (a whole cell of level 2), in the corner
    fluid[0:4, 25:37, 0:4] = True
    # the shelf and the film on it: x 16..31, z 32..47, solid below y = 24, fluid at y = 24 alone
    solid[32:48, 0:24, 16:32] = True
    fluid[32:48, 24:, 16:32] = False
    fluid[32:48, 24, 16:32] = True
    groups["film"] = [(20, 24, 40), (31, 24, 47)]
    # behind_wall: tile (4,2,0); a wall at x = 32 and 1 x 2 x 2 fluid behind it at x = 33, y = 16, 17 - level-1 cell (16, 8, 2) is FLUID
    solid[4:6, 16:18, 32] = True
    fluid[4:6, 16:18, 33] = True
    groups["behind_wall"] = [(33, 16, 4), (33, 17, 5)]
    # in_box: tile (5,1,3) = x 40..47, y 8..15, z 24..31 emptied, a floor under it, a wall at x = 40 and 1 x 2 x 2 fluid at x = 41
    fluid[24:32, 8:16, 40:48] = False
    solid[24:32, 7, 40:48] = True
    solid[24:32, 8:11, 40] = True
    fluid[26:28, 8:10, 41] = True
    groups["in_box"] = [(41, 8, 26), (41, 9, 27)]
    # single droplets (closed tiles) and a pair across the tile face x = 55 | 56 (open)
    for name, cells in (("single", [(60, 20, 10)]), ("cell7", [(55, 20, 47)]), ("pair", [(55, 26, 20), (56, 26, 20)])):
        for cx, cy, cz in cells:
            fluid[cz, cy, cx] = True
        groups[name] = cells
    fluid &= ~solid
    return fluid, solid, groups


def terraces(variant=None, seed=88):
    rng = np.random.default_rng(seed)
    fluid, solid, groups = _terraces_masks()
    if variant == "shifted":
        moved = np.zeros_like(fluid)
        moved[:, :, 8:] = fluid[:, :, :-8]
        fluid, groups = moved & ~solid, {}
        fluid &= ~sc._walled_in(TERRACES_SIZE, fluid, solid)
    elif variant in ("half", "half_solid"):
        fluid[:, :, 35:] = False
        groups = {k: v for k, v in groups.items() if all(c[0] < 35 for c in v)}
        if variant == "half_solid":  # another solid mask: a block in the air that is left, and one pillar gone
            solid[40:42, 30:32, 60:62] = True
            solid[21, :, 21] = False
    return sc._finish(TERRACES_SIZE, fluid, solid, rng, per_cell=(1, 2), groups=groups, pillars=PILLARS)


def plate(seed=99):
    """One particle per cell, at rest at the cell's centre (the system's matrix is all the V-cycle reads)."""
    nx, ny, nz = PLATE_SIZE
    z, y, x = np.meshgrid(np.arange(nz), np.arange(2), np.arange(nx), indexing="ij")
    parts = np.zeros(x.size, dtype=PARTICLE_DTYPE)
    parts["pos"] = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1) + 0.5
    parts["old_pos"] = parts["pos"]
    return PLATE_SIZE, parts, None, dict(h=1.0, off=(0.0, 0.0, 0.0), rho=1.0)


@functools.lru_cache(maxsize=None)
def _raw(name):
    """(size, parts, solid cells, meta) of any field here, as its builder made it."""
    if name in sc.CASES:
        return sc.build(name)
    if name in SEQUENCE_FIELDS:
        size, _, solid, meta = sc.build("droplets")
        return size, ssc.particles(name), solid, dict(meta, groups=ssc.groups(name))
    out = plate() if name == "plate" else terraces(None if name == "terraces" else name[len("terraces_"):])
    out[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def build(name):
    """(size, parts, solid cells, meta) of any field here. For `terraces` and its variants meta["conditions"] holds what the field is
    built to have, counted from the model's own hierarchy (features)."""
    size, parts, solid, meta = _raw(name)
    if name.startswith("terraces"):
        meta = dict(meta, conditions=features(name))
    return size, parts, solid, meta


def solid_mask(name):
    size, _, solid, _ = _raw(name)
    return None if solid is None else sc._mask_of(size, solid)


def a_scale(name):
    meta = _raw(name)[3]
    return DT / (meta["rho"] * meta["h"] ** 2)  # src/pressure_solver.cpp:22


# ---------------------------------------------------------------------------------------------------- the level-0 system
def plate_system_of(size, fluid=None):
    """The A-byte rule (oracle/oracle.c orc_build_system) restated for a field without solid cells: every cell of `fluid` (bool[nz,
    ny, nx]; None: the plate, y = 0, 1) holds one particle and is FLUID, every other cell is AIR, outside the grid is solid: ns counts
    the neighbours inside the grid, bit 3 + d says that the +d neighbour is FLUID. tests/test_vcycle_model.py holds it to the oracle's
    hash + build_system on a small plate, tests/test_multilevel_model.py on a small plate with holes."""
    nx, ny, nz = size
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    fluid = (y < 2) if fluid is None else np.asarray(fluid, dtype=bool).reshape(nz, ny, nx)
    raw = (x + nx * (y + ny * z))
    fc = np.sort(raw[fluid]).astype(np.uint64)
    cz, cy, cx = fc.astype(np.int64) // (nx * ny), (fc.astype(np.int64) // nx) % ny, fc.astype(np.int64) % nx
    ns = (cx > 0).astype(int) + (cx < nx - 1) + (cy > 0) + (cy < ny - 1) + (cz > 0) + (cz < nz - 1)
    up = [fluid[cz, cy, np.minimum(cx + 1, nx - 1)] & (cx < nx - 1), fluid[cz, np.minimum(cy + 1, ny - 1), cx] & (cy < ny - 1),
          fluid[np.minimum(cz + 1, nz - 1), cy, cx] & (cz < nz - 1)]
    ab = ns | (up[0].astype(int) << 3) | (up[1].astype(int) << 4) | (up[2].astype(int) << 5)
    types = np.where(fluid, sc.FLUID, sc.AIR).reshape(-1).astype(np.uint8)
    return dict(size=size, fluid_cells=fc, counts=fluid.reshape(-1).astype(np.uint32), type=types, abits=ab.astype(np.uint8),
                b=None, p=None, iters=None, vel=np.zeros((nx * ny * nz, 3)))


@functools.lru_cache(maxsize=None)
def system(name):
    """dict(size, fluid_cells, counts, type, abits, b, p, iters, vel - the fp32-rounded grid after gravity, what a device is handed)."""
    if name == "plate":
        return plate_system_of(PLATE_SIZE)
    size = _raw(name)[0]
    if name in sc.CASES:
        w = sc.oracle_stages(name, True)
        return dict(size=size, fluid_cells=w["fluid_cells"], counts=w["counts"], type=w["type"], abits=w["abits"], b=w["b"], p=w["p"],
                    iters=int(w["iters"]), vel=w["grav_vel"])
    if name in SEQUENCE_FIELDS:
        w = ssc.solved(ssc.Step(name))
        counts = np.zeros(size[0] * size[1] * size[2], dtype=np.uint32)
        counts[w["fluid_cells"].astype(np.int64)] = 1  # (which cells hold particles is all the hierarchy reads)
        return dict(size=size, fluid_cells=w["fluid_cells"], counts=counts, type=w["type"], abits=w["abits"], b=w["b"], p=w["p"],
                    iters=w["iters"], vel=w["vel"])
    return staged(name, "oracle")


def staged(name, kind):
    """The stages the model reads, on the oracle or on the compiled reference."""
    size, parts, solid, meta = _raw(name)
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=sc.APIC, blending=1.0, density=meta["rho"], kind=kind)
    if solid is not None:
        s.set_solid_cells(solid)
    s.set_particles(parts)
    s.hash()
    out = dict(size=size, fluid_cells=s.fluid_cells(), counts=s.space_hash()[1].astype(np.uint32))
    s.p2g()
    s.add_gravity(DT)
    cells = s.cells()
    cells["vel"] = sc.f32(cells["vel"])
    s.set_cells(cells)
    out["type"], out["vel"] = cells["type"].copy(), cells["vel"].copy()
    s.build_system(DT)
    out["abits"], out["b"] = s.abits(), s.b()
    p, res, it = s.solve(DT)
    out["p"], out["iters"] = p.copy(), int(it)
    s.close()
    return out


def tiles_of(w):
    """(particle tiles, closed tiles): sets of (tx, ty, tz) - grid_ops.hip:47-49, 74-84 from the A bytes."""
    per = sc.unknowns_per_tile(w["size"], w["fluid_cells"])
    nx, ny, nz = w["size"]
    r = np.asarray(w["fluid_cells"], dtype=np.int64)
    c = np.stack([r % nx, (r // nx) % ny, r // (nx * ny)], axis=1)
    coupled = set()
    for d in range(3):
        on = ((np.asarray(w["abits"]) >> (3 + d)) & 1).astype(bool) & (c[:, d] % 8 == 7)
        if on.any():
            e = np.zeros(3, dtype=np.int64)
            e[d] = 1
            coupled |= {tuple(t) for t in (c[on] // 8).tolist()} | {tuple(t) for t in ((c[on] + e) // 8).tolist()}
    return set(per), {t for t, k in per.items() if k <= sc.CLOSED_MAX and t not in coupled}


def model(name, closed=True, prune=True, mutant=None):
    """The hierarchy of a field. closed=False: no tile is closed (LFA_MG_NO_CLOSED=1). Only the mutant outside_is_air has a
    hierarchy of its own."""
    return _model(name, closed, prune, mutant if mutant == "outside_is_air" else None)


@functools.lru_cache(maxsize=None)
def _model(name, closed, prune, mutant):
    w = system(name)
    ptiles, cl = tiles_of(w)
    if len(vm.level_grids(w["size"])) == 1:
        cl = set()  # mg.hip:2230: a grid of one level keeps its closed tiles in the cycle
    return vm.hierarchy(w["size"], w["fluid_cells"], w["abits"], w["type"], w["counts"], solid_mask(name), ptiles, cl if closed else set(),
                        a_scale(name), prune=prune, mutant=mutant)


# ---------------------------------------------------------------------------------------------------- right-hand sides
def _smooth(w):
    nx, ny, nz = w["size"]
    r = np.asarray(w["fluid_cells"], dtype=np.int64)
    x, y, z = r % nx, (r // nx) % ny, r // (nx * ny)
    return np.cos(np.pi * x / nx) * np.cos(np.pi * z / nz) + 0.5 * np.cos(np.pi * y / ny) + 1.5


def designed_unknowns(name):
    """label -> index of an unknown, up to 24, no unknown twice: one cell of each of the field's named droplet groups (a pair across a
    tile face among them), cells next to a pillar (aligned with the coarse cells and not) and next to any cell of the solid mask -
    each in a tile the V-cycle runs on -, a child of a level-1 unknown, tile corners and faces of level 0, cells whose parent lies
    on a coarse tile face, cells in a child of a pruned level-1 tile, cells in the last layer of each axis, cells in a closed tile.
    Where several unknowns qualify the pick is spread over them (a fixed fraction of the way through, another per label), not the
    first in raw order: the picks do not crowd into the corner at the origin."""
    w, H = system(name), model(name)
    nx, ny, nz = w["size"]
    z, y, x = H.index
    ab = np.asarray(w["abits"]).astype(np.int64)
    lx, ly, lz = x % 8, y % 8, z % 8
    edge = lambda a: (a == 0) | (a == 7)
    op = vm.open_mask(H)
    pick = {}

    def choose(label, mask, frac=0.0):
        at = np.flatnonzero(mask)
        taken = set(pick.values())
        for k in range(len(at)):
            i = int(at[(int(frac * len(at)) + k) % len(at)])
            if i not in taken:
                pick[label] = i
                return

    meta = _raw(name)[3]
    # the field's named droplet groups first (at most 8: pairs across a tile face, then the rest by name), one cell of each
    groups = {k: v for k, v in meta.get("groups", {}).items() if k != "pool"}
    for k in sorted(groups, key=lambda k: (not (k.startswith("straddle") or k == "pair"), k))[:8]:
        cx, cy, cz = groups[k][-1]
        choose(f"group_{k}", (x == cx) & (y == cy) & (z == cz))
    sm = solid_mask(name)
    if sm is not None:
        beside = np.zeros_like(sm)
        for d in range(3):
            for sign in (-1, 1):
                beside |= sc._nb(sm, d, sign, False)
        beside = beside[z, y, x] & op
        for k, ((x0, x1), (z0, z1)) in sorted(meta.get("pillars", {}).items()):  # the cells on the -x and +x sides of the pillar
            choose(f"pillar_{k}", beside & ((x == x0 - 1) | (x == x1 + 1)) & (z >= z0) & (z <= z1), 0.6)
        choose("by_solid", beside, 0.45)
    if H.last >= 1:  # a cell whose parent is an unknown of level 1: the coarse correction at its largest
        choose("coarse_unknown_child", H.levels[1].unk[z // 2, y // 2, x // 2] & H.levels[0].unk[z, y, x], 0.5)
    if len(H.levels) > 1 and H.pruned.any():
        choose("pruned_child", H.pruned[z // 16, y // 16, x // 16], 0.5)
    choose("closed", ~op, 0.0)
    c = (x, y, z)
    for d, n in enumerate("xyz"):
        choose(f"last_{n}", c[d] == (nx, ny, nz)[d] - 1, 0.4 + 0.15 * d)
    choose("corner_000", (lx == 0) & (ly == 0) & (lz == 0), 0.3)
    choose("corner_777", (lx == 7) & (ly == 7) & (lz == 7), 0.7)
    choose("corner_any", edge(lx) & edge(ly) & edge(lz), 0.55)
    for d, (l, n) in enumerate(((lx, "x"), (ly, "y"), (lz, "z"))):  # (what the cut at 24 drops is the tail of these)
        choose(f"parent_face_{n}", ((l // 2 == 0) | (l // 2 == 3)) & ((c[d] // 8) % 2 == (l // 2 == 3)), 0.35 + 0.2 * d)
        choose(f"face_{n}7", (l == 7) & (((ab >> (3 + d)) & 1) == 1), 0.8 - 0.25 * d)
        choose(f"face_{n}0", (l == 0) & (((ab >> 3) & 7) != 0), 0.2 + 0.25 * d)
    return dict(list(pick.items())[:24])


@functools.lru_cache(maxsize=None)
def rhs(name, seed=7):
    """label -> right-hand side (read-only)."""
    w, H = system(name), model(name)
    n = len(w["fluid_cells"])
    rng = np.random.default_rng(seed + n)
    out = {"random": rng.normal(size=n)}
    if w["b"] is not None:
        out["b"] = np.array(w["b"])
    out["A_smooth"] = vm.apply_a(H, _smooth(w))
    if H.last >= 1:  # A (P chi), chi = 1 on the unknowns of level 1: the right-hand side whose answer IS a coarse correction
        z, y, x = H.index
        out["A_coarse"] = vm.apply_a(H, (H.levels[1].unk[z // 2, y // 2, x // 2] & H.levels[0].unk[z, y, x]).astype(np.float64))
    if name != "plate":
        for k, i in designed_unknowns(name).items():
            e = np.zeros(n)
            e[i] = 1.0
            out[f"impulse_{k}"] = e
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_pcg(name):
    """(p, iterations) of the model PCG on the field's own right-hand side, computed once."""
    return vm.pcg(model(name), system(name)["b"])


# ---------------------------------------------------------------------------------------------------- bars
@functools.lru_cache(maxsize=None)
def reference(name, label, closed=True, prune=True):
    """(z, d32) of one right-hand side: the fp64 model and max |V_float32(r) - V_float64(r)| over the unknowns outside the closed
    tiles (those have a bar of their own: closed_bars), but no less than half an fp32 ulp of the largest of those entries of z;
    computed once and shared."""
    H = model(name, closed, prune)
    r = rhs(name)[label]
    z = vm.vcycle(H, r)
    op = vm.open_mask(H)
    d32 = 0.0
    if op.any():
        d32 = fp32_deviation(vm.vcycle(H, r, dtype=np.float32)[op], z[op])
    z.setflags(write=False)
    return z, d32


F32_BARS = 8.0     # an fp32 result is held to F32_BARS d32
F64_REL = 1e-10    # an fp64 result to F64_REL max |model|


def fp32_deviation(z32, z64):
    """d32 = max |model_float32 - model_float64|, never below half an fp32 ulp of the largest entry (reference says why). The one
    place of the rule: tests/multilevel_cases.py takes its bars from here too."""
    # A unit impulse takes a handful of roundings, and the numpy run can be lucky: on `maze`, impulse_last_z, it deviates by 8.5e-9
    # max |z|, a seventh of the HALF ULP of the largest entry, while the device - whose z is stored in fp32 like the model's - is 0.9
    # ulp away (1.19 bars of 8 d32). d32 is therefore never taken below the rounding of the result's storage, 2^-24 max |z| over
    # the V-cycle's unknowns: below that the figure measures luck, not arithmetic. (Recorded in docs/experiments.md.)
    z32, z64 = np.asarray(z32, dtype=np.float64), np.asarray(z64, dtype=np.float64)
    if not z64.size:
        return 0.0
    return max(float(np.abs(z32 - z64).max()), 2.0 ** -24 * float(np.abs(z64).max()))


def bar(name, label, f64, closed=True, prune=True):
    """The bar of the V-cycle's share of z. fp64: 1e-10 max |z|; fp32: 8 d32."""
    z, d32 = reference(name, label, closed, prune)
    return F64_REL * float(np.abs(z).max()) if f64 else F32_BARS * d32


def closed_bars(H, r, f64, tolerance=1e-6):
    """Per unknown: the bar of its closed tile's solve (0 outside the closed tiles): |A_tile^-1|_inf stop / a_scale, stop = the
    stopping value of k_mg_solve_closed (mg.hip:2989-2990, 3038): the larger of 0.05 tolerance and its rounding floor (1e-15 fp64,
    4e-7 fp32) times max |r| over the tile."""
    out = np.zeros(len(r))
    for idx, A in H.closed_blocks:
        stop = max(0.05 * tolerance, (1e-15 if f64 else 4e-7) * float(np.abs(r[idx]).max()))
        out[idx] = np.abs(np.linalg.inv(A)).sum(axis=1).max() * stop / H.a_scale
    return out


# ---------------------------------------------------------------------------------------------------- what a field can show
def features(name):
    """Counts, from the model's own hierarchy, of what the mutants need and what `terraces` is built to have."""
    H = model(name)
    Ls = H.levels
    f = {"levels": len(Ls), "last": H.last, "closed": len(H.closed)}
    f["unknowns_per_level"] = [int(L.unk.sum()) for L in Ls]
    f["pruned_with_active_child"] = int(H.pruned.sum()) if len(Ls) > 1 else 0
    cross = []
    for L in Ls[: H.last + 1]:
        n = 0
        for d in range(3):
            n += int((L.xp[d] & ~L.inner[(d, 1)] & vm._shift(L.unk, d, 1, False)).sum())
        cross.append(n)
    f["couplings_across_active_tile_faces"] = cross
    f["inactive_fluid_neighbour"], f["inactive_octants"], f["unknown_in_inactive_octant"], f["outside_children"] = 0, 0, 0, []
    f["outside_children_fluid"] = 0
    for l in range(1, len(Ls)):
        L, F = Ls[l], Ls[l - 1]
        on = vm._cells_of_tiles(L.act)
        for d in range(3):
            for s in (-1, 1):
                beside = on & ~L.inner[(d, s)] & ~vm._shift(on, d, s, False) & (vm._shift(L.mtype, d, s, vm.MT_SOLID) == vm.MT_FLUID)
                f["inactive_fluid_neighbour"] += int(beside.reshape(L.nt[2], 8, L.nt[1], 8, L.nt[0], 8).any(axis=(1, 3, 5)).sum())
        child_on = vm._padded(np.repeat(np.repeat(np.repeat(F.act, 4, axis=0), 4, axis=1), 4, axis=2), L.shape, False)
        if l == 1:
            oct_off = (on & ~child_on).reshape(L.nt[2], 8, L.nt[1], 8, L.nt[0], 8).any(axis=(1, 3, 5))
            f["inactive_octants"] = int(oct_off.sum())
        # an unknown in the octant of an inactive child tile that is coupled to an unknown in the octant of an active one
        off_unk, on_unk = L.unk & ~child_on, L.unk & child_on
        for d in range(3):
            f["unknown_in_inactive_octant"] += int((L.xp[d] & off_unk & vm._shift(on_unk, d, 1, False)).sum())
            f["unknown_in_inactive_octant"] += int((L.xp[d] & on_unk & vm._shift(off_unk, d, 1, False)).sum())
        oc = H.outside_children[l - 1]
        f["outside_children"].append(int(oc.sum()))
        f["outside_children_fluid"] += int((oc & (L.mtype[: oc.shape[0], : oc.shape[1], : oc.shape[2]] == vm.MT_FLUID)).sum())
    # unknowns of a level 1 .. last - 1 that are coupled to two or more unknowns of their level
    f["coarse_chains"] = 0
    for L in Ls[1: H.last]:
        deg = np.zeros(L.shape, dtype=np.int64)
        for d in range(3):
            up = L.xp[d] & vm._shift(L.unk, d, 1, False)
            deg += up + vm._shift(up, d, -1, False)
        f["coarse_chains"] += int((deg >= 2).sum())
    f["cell_0_and_7"] = []
    for L in Ls[:3]:
        zz, yy, xx = np.nonzero(L.unk)
        f["cell_0_and_7"].append([bool((c % 8 == k).any()) for c in (xx, yy, zz) for k in (0, 7)])
    return f


def visible(name, mutant):
    """Whether the field has the feature the mutant needs (vcycle_model.MUTANTS), from features() alone."""
    f = features(name)
    two = f["last"] >= 1
    cross = f["couplings_across_active_tile_faces"]
    return {
        "restrict_045": two,
        "omega_coarse_1": two and f["coarse_chains"] > 0,
        "post_red_first": True,
        "ring_live": sum(cross) > 0,
        "ring_uncorrected": two and sum(cross[: f["last"]]) > 0,
        "outside_is_air": two and f["outside_children_fluid"] > 0,
        "coarsest_1": two and f["unknowns_per_level"][f["last"]] > 0,
        "stale_octant": two and f["unknown_in_inactive_octant"] > 0,
        "prune_ignored_in_ring": two and f["pruned_with_active_child"] > 0,
        "closed_smoothed": f["closed"] > 0,
    }[mutant]
