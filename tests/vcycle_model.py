"""The multigrid V-cycle of libfluid_amd/csrc/mg.hip (z = M^-1 r, LFA_PRECOND_MULTIGRID) restated in plain numpy, fp64.

A stateless function of the level-0 system: hierarchy(...) builds the levels from the inputs of one set-up, vcycle(H, r) applies the
cycle. Whole level arrays indexed [z, y, x] and padded to whole tiles, no tile-major storage, no launch layout: the tagged / flags /
launch-per-phase / fused-top forms of the device are ONE operator and this is it. Written from the header comment and the device
code of mg.hip; the rules and the lines they restate (mg.hip unless another file is named):

  level grids   halve with (n + 1) / 2 until every axis is at most 8; the last level always runs        2153-2161
  fine type     outside the particle tiles solid or air by the solid mask; a SOLID-typed cell is a wall even when it
                holds particles; otherwise FLUID exactly when its count is above 0                          144-151
  coarse type   AIR if any child is air, else FLUID if any child is fluid, else SOLID; children outside the
                finer grid are SOLID                                                           192-204, 215-231
  coarse A      the 7-point operator rediscretised on those types, unscaled, for the active tiles           233-252
  level-0 A     the given A bytes; AB_FLUID (couples to the three lower neighbours) is "typed FLUID",
                AB_UNKNOWN "holds particles"                    grid_ops.hip 66-72, pcg.h 63-79, mg.hip 481-491
  active tiles  level 0: particle tiles minus closed ones (256-259); level 1: parents of active tiles that hold a
                level-1 unknown (269-281, 2255); levels >= 2: parents of active tiles. Inactive tiles hold zeros and stay
                zero: a missing neighbour reads 0 (pcg.h 58, mg.hip 651). Level 1 empty: the finest level's sweeps
                alone (2650, 2808-2819)
  smoother      red-black SOR, MG_OMEGA (50), MG_INNER_SWEEPS (46) sweeps; down red -> black from zero with a zero
                ring (529-540), up black -> red with the ring frozen at the neighbours' corrected pre-smoothed values
                x + P e (646-671); cells that are no unknown or have no non-solid neighbour stay as they are (482-490)
  restriction   half the sum of the 8 children's residuals b - A x (572-600, pcg.h 75-79); an inactive child's octant
                is 0 (1502-1508; the level arrays: 403-415)
  prolongation  the parent's value, onto unknowns only, ring cells included                                 638-656
  coarsest      MG_COARSEST_SWEEPS (2557) sweeps red -> black, then as many black -> red, from zero         675-697
  result        divided by a_scale                                                                    2806, 2881
  closed tiles  their share of z is the exact solve of the tile's block, divided by a_scale
                                                              mg.hip 2958-3027, pcg.hip 2102-2103, grid_ops.hip 47-49

dtype=np.float32 rounds every array and constant to fp32 and computes in fp32 (no fused multiply-add, numpy's summation order
within a cell): the measure of what fp32 arithmetic does to the cycle, used for the fp32 bar only.

mutant= changes exactly one rule (MUTANTS); tests/test_vcycle_model.py shows that each moves z by at least 100 fp32 bars.
"""
import numpy as np

MG_OMEGA = 1.15           # mg.hip:50
MG_INNER_SWEEPS = 2       # mg.hip:46
MG_COARSEST_SWEEPS = 2    # mg.hip:2557
MG_MAX_LEVELS = 12        # mg.hip:40
MT_SOLID, MT_FLUID, MT_AIR = 0, 1, 2  # mg.hip:139
CT_AIR, CT_FLUID, CT_SOLID = 1, 2, 4  # the cell types of the grid (libfluid_amd/csrc/common.h)

MUTANTS = {
    "restrict_045": "restriction weight 0.45 instead of 0.5. Needs: a level 1 with unknowns.",
    "omega_coarse_1": "omega 1.0 on levels 1 and up. Needs: below the last level, a coarse unknown coupled to two or more unknowns of its level "
                      "(the four sweeps of a level solve an unknown that stands alone, or a pair, to (1 - omega)^4 = 5e-4 of the "
                      "correction whatever omega is, and so do the last level's on its few unknowns).",
    "post_red_first": "post-smoothing starts with red instead of black. Needs: two coupled unknowns in an active tile.",
    "ring_live": "Gauss-Seidel across tile faces in the post-smoothing instead of a frozen ring. Needs: a coupling across a "
                 "face between two active tiles of one level.",
    "ring_uncorrected": "the ring holds x instead of x + P e. Needs: such a coupling on a level below the last one, with a "
                        "non-zero correction of the ring cell.",
    "outside_is_air": "children outside an odd grid count as AIR. Needs: a FLUID coarse cell with a child outside the finer grid.",
    "coarsest_1": "one coarsest sweep each way instead of MG_COARSEST_SWEEPS. Needs: unknowns on the last level (of two or more).",
    "stale_octant": "the octant of an inactive child keeps the value 1 as its right-hand side. Needs: an active coarse tile with an "
                    "unknown in the octant of an inactive child tile (a closed tile whose fluid fills a coarse cell) that is coupled to an "
                    "unknown in the octant of an active one.",
    "prune_ignored_in_ring": "a pruned level-1 tile's cells read as active and non-zero (their restricted right-hand side, which the "
                             "children keep writing) where level 0 prolongs from them, ring cells included. Needs: a pruned level-1 "
                             "tile with an active child tile.",
    "closed_smoothed": "closed tiles get two sweeps instead of the exact solve. Needs: a closed tile.",
}


def level_grids(size):
    """(nx, ny, nz) of every level. mg.hip:2153-2161."""
    gs = [tuple(int(n) for n in size)]
    while max(gs[-1]) > 8 and len(gs) < MG_MAX_LEVELS:
        gs.append(tuple((n + 1) // 2 for n in gs[-1]))
    return gs


def _tiles(g):
    return tuple((n + 7) // 8 for n in g)


def _padded(a, shape, fill):
    """`a` [z, y, x] in the corner of an array of `shape`, `fill` elsewhere."""
    out = np.full(shape, fill, dtype=a.dtype)
    out[: a.shape[0], : a.shape[1], : a.shape[2]] = a[: shape[0], : shape[1], : shape[2]]
    return out


def _cells_of_tiles(flag):
    """bool[ntz, nty, ntx] -> bool over the padded cells."""
    return np.repeat(np.repeat(np.repeat(flag, 8, axis=0), 8, axis=1), 8, axis=2)


def _children_any(a):
    """out[Z, Y, X] = any of the 8 children a[2Z + k, 2Y + j, 2X + i]; `a` has even dimensions."""
    z, y, x = a.shape
    return a.reshape(z // 2, 2, y // 2, 2, x // 2, 2).any(axis=(1, 3, 5))


def _shift(a, d, sign, fill=0):
    """out[c] = a[c + sign e_d] (d = 0, 1, 2 for x, y, z), `fill` outside the array."""
    ax = 2 - d
    out = np.full_like(a, fill)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[ax], dst[ax] = (slice(1, None), slice(0, -1)) if sign > 0 else (slice(0, -1), slice(1, None))
    out[tuple(dst)] = a[tuple(src)]
    return out


class Level:
    """One level: g (nx, ny, nz), nt tiles per axis, shape of the padded arrays [z, y, x]; mtype (levels >= 1); act bool per tile
    [ntz, nty, ntx]; unk, lo, xp[3] bool and ns int over the padded cells - all zero in inactive tiles."""


class Hierarchy:
    """levels, last (the coarsest level that runs), tiles (active tiles per level), closed / closed_blocks, a_scale, index (the
    padded level-0 position of every unknown), pruned (level-1 tiles pruned although a child tile is active, bool per tile)."""


def hierarchy(size, fluid_cells, abits, types, counts, solid, particle_tiles, closed, a_scale, prune=True, mutant=None):
    """size (nx, ny, nz); fluid_cells: raw index x + nx (y + ny z) of every unknown, ascending; abits: the unknowns' A bytes (bits 0-2
    non-solid neighbours, 3-5 "the +x / +y / +z neighbour is typed FLUID"); types, counts: per cell in raw order; solid: bool[nz, ny,
    nx] or None; particle_tiles, closed: sets of (tx, ty, tz). prune=False: LFA_MG_NO_PRUNE=1."""
    assert mutant is None or mutant in MUTANTS, mutant
    nx, ny, nz = (int(n) for n in size)
    gs = level_grids(size)
    H = Hierarchy()
    H.size, H.a_scale, H.mutant, H.levels = (nx, ny, nz), float(a_scale), mutant, []
    fc = np.asarray(fluid_cells, dtype=np.int64)
    ab = np.asarray(abits).astype(np.int64)
    t3 = np.asarray(types).reshape(nz, ny, nx)
    c3 = np.asarray(counts).reshape(nz, ny, nx)
    s3 = np.zeros((nz, ny, nx), dtype=bool) if solid is None else np.asarray(solid, dtype=bool).reshape(nz, ny, nx)
    # ---- level 0
    L = Level()
    L.g, L.nt = gs[0], _tiles(gs[0])
    L.shape = tuple(8 * n for n in L.nt[::-1])
    ptile = np.zeros(L.nt[::-1], dtype=bool)
    for tx, ty, tz in particle_tiles:
        ptile[tz, ty, tx] = True
    cl = np.zeros_like(ptile)
    for tx, ty, tz in closed:
        assert ptile[tz, ty, tx]
        cl[tz, ty, tx] = True
    L.act = ptile & ~cl  # mg.hip:256-259
    z, y, x = fc // (nx * ny), (fc // nx) % ny, fc % nx
    H.index = (z, y, x)
    raw = {k: np.zeros(L.shape, dtype=np.int64) for k in ("unk", "ns", "xp", "yp", "zp", "lo")}
    raw["unk"][z, y, x] = 1
    raw["ns"][z, y, x] = ab & 7
    for d, k in enumerate(("xp", "yp", "zp")):
        raw[k][z, y, x] = (ab >> (3 + d)) & 1
    raw["lo"][z, y, x] = t3[z, y, x] == CT_FLUID  # AB_FLUID, grid_ops.hip:70-72
    H.raw0 = raw  # (closed tiles included: their blocks are solved from these)
    in_p = _cells_of_tiles(ptile)[:nz, :ny, :nx]
    # fine_type, mg.hip:144-151
    ftype = np.where(in_p, np.where(t3 == CT_SOLID, MT_SOLID, np.where(c3 > 0, MT_FLUID, MT_AIR)), np.where(s3, MT_SOLID, MT_AIR))
    assert np.array_equal(np.sort(np.flatnonzero((c3 > 0).reshape(-1))), fc), "the unknowns are the cells that hold particles"
    H.levels.append(L)
    # ---- levels >= 1
    outside = MT_AIR if mutant == "outside_is_air" else MT_SOLID  # mg.hip:197, 226
    H.outside_children = []
    for l in range(1, len(gs)):
        F, L = H.levels[-1], Level()
        L.g, L.nt = gs[l], _tiles(gs[l])
        L.shape = tuple(8 * n for n in L.nt[::-1])
        cx, cy, cz = L.g
        ft = _padded(ftype, (2 * cz, 2 * cy, 2 * cx), outside)
        air, fluid = _children_any(ft == MT_AIR), _children_any(ft == MT_FLUID)
        ctype = np.where(air, MT_AIR, np.where(fluid, MT_FLUID, MT_SOLID))  # mg.hip:202, 230
        H.outside_children.append(_children_any(_padded(np.zeros_like(ftype, dtype=bool), (2 * cz, 2 * cy, 2 * cx), True)))
        L.mtype = _padded(ctype, L.shape, MT_SOLID)  # mg.hip:172 (!in_grid: SOLID)
        # active tiles: parents of active tiles; level 1: ... that hold a level-1 unknown (mg.hip:269-281, 351)
        fa = _padded(F.act, tuple(2 * n for n in L.nt[::-1]), False)
        parents = _children_any(fa)
        L.act = parents.copy()
        if l == 1:
            has = (L.mtype == MT_FLUID).reshape(L.nt[2], 8, L.nt[1], 8, L.nt[0], 8).any(axis=(1, 3, 5))  # mg.hip:204-210
            H.pruned = parents & ~has
            if prune:
                L.act &= has
        ftype = ctype
        H.levels.append(L)
    if len(gs) == 1:
        H.pruned = np.zeros((1, 1, 1), dtype=bool)
    for l, L in enumerate(H.levels):
        on = _cells_of_tiles(L.act)
        if l == 0:
            f = {k: v * on for k, v in raw.items()}
        else:
            # k_mg_abits, mg.hip:233-252: neighbours outside the grid are SOLID
            t = np.where(on, L.mtype, -1)
            unk = t == MT_FLUID
            nb = {(d, s): _shift(L.mtype, d, s, MT_SOLID) for d in range(3) for s in (-1, 1)}
            f = {"unk": unk.astype(np.int64), "lo": unk.astype(np.int64),
                 "ns": unk * sum((v != MT_SOLID).astype(np.int64) for v in nb.values())}
            for d, k in enumerate(("xp", "yp", "zp")):
                f[k] = (unk & (nb[(d, 1)] == MT_FLUID)).astype(np.int64)
        L.unk, L.lo, L.ns = f["unk"].astype(bool), f["lo"].astype(bool), f["ns"]
        L.xp = [f["xp"].astype(bool), f["yp"].astype(bool), f["zp"].astype(bool)]
        zz, yy, xx = np.meshgrid(*[np.arange(n) for n in L.shape], indexing="ij")
        L.parity = (xx + yy + zz) & 1
        L.inner = {(0, -1): xx % 8 != 0, (0, 1): xx % 8 != 7, (1, -1): yy % 8 != 0, (1, 1): yy % 8 != 7,
                   (2, -1): zz % 8 != 0, (2, 1): zz % 8 != 7}  # the neighbour lies in the same tile
    H.tiles = [int(L.act.sum()) for L in H.levels]
    # mg.hip:2650: no coarse unknown anywhere -> the finest level's sweeps alone
    H.last = 0 if (len(H.levels) > 1 and H.tiles[1] == 0) else len(H.levels) - 1
    H.closed = sorted(closed)
    H.closed_blocks = [_closed_block(H, t) for t in H.closed]
    return H


def _closed_block(H, tile):
    """(idx: positions in the unknown vector, A: the tile's block of the unscaled operator, dense). pcg.h:63-73."""
    tx, ty, tz = tile
    z, y, x = H.index
    idx = np.flatnonzero((x // 8 == tx) & (y // 8 == ty) & (z // 8 == tz))
    pos = {(int(x[i]), int(y[i]), int(z[i])): k for k, i in enumerate(idx)}
    raw = H.raw0
    A = np.zeros((len(idx), len(idx)))
    for (cx, cy, cz), k in pos.items():
        A[k, k] = raw["ns"][cz, cy, cx]
        for d, bit in enumerate(("xp", "yp", "zp")):
            e = [0, 0, 0]
            e[d] = 1
            up, dn = (cx + e[0], cy + e[1], cz + e[2]), (cx - e[0], cy - e[1], cz - e[2])
            if raw[bit][cz, cy, cx] and up in pos:
                A[k, pos[up]] -= 1.0
            if raw["lo"][cz, cy, cx] and dn in pos:
                A[k, pos[dn]] -= 1.0
    return idx, A


# ---------------------------------------------------------------------------------------------------- the cycle
def _coef(L, omega, dt):
    """(keep, gain) of gs_coef, mg.hip:481-491, and the couplings as 0 / 1 factors: (keep, gain, lo, xp[3])."""
    on = L.unk & (L.ns > 0)
    rcp = (dt(1.0) / np.maximum(L.ns, 1).astype(dt)).astype(dt)
    keep = np.where(on, dt(1.0 - omega), dt(1.0)).astype(dt)
    gain = np.where(on, dt(omega) * rcp, dt(0.0)).astype(dt)
    return keep, gain, L.lo.astype(dt), [m.astype(dt) for m in L.xp]


def _neighbours(L, x, ring):
    """The six neighbour values of every cell: from x inside the tile, from `ring` across a tile face (ring[(d, s)]: the frozen
    values already shifted; None: all from x)."""
    out = {}
    for d in range(3):
        for s in (-1, 1):
            v = _shift(x, d, s)
            if ring is not None:
                v = np.where(L.inner[(d, s)], v, ring[(d, s)])
            out[(d, s)] = v
    return out


def _colour(L, x, b, ring, colour, coef, dt):
    """gs_colour / gs_update, mg.hip:492-524: the cells with (x + y + z) & 1 == colour."""
    keep, gain, lo, xp = coef
    n = _neighbours(L, x, ring)
    s = b + lo * n[(0, -1)]
    s = s + lo * n[(1, -1)]
    s = s + lo * n[(2, -1)]
    for d in range(3):
        s = s + xp[d] * n[(d, 1)]
    new = s * gain + keep * x
    return np.where(L.parity == colour, new, x).astype(dt)


def _sweeps(L, x, b, frozen, first, count, coef, dt):
    """`frozen`: the values the ring holds during the sweeps (an array; 0: a zero ring; None: no ring - the neighbours' live values)."""
    if frozen is None:
        ring = None
    elif isinstance(frozen, int):
        ring = {k: dt(0.0) for k in L.inner}
    else:
        ring = {(d, s): _shift(frozen, d, s) for d in range(3) for s in (-1, 1)}
    for _ in range(count):
        x = _colour(L, x, b, ring, first, coef, dt)
        x = _colour(L, x, b, ring, first ^ 1, coef, dt)
    return x


def _residual(L, x, b, dt):
    """residual_cell / stencil_row, pcg.h:63-79: over the whole level (an inactive tile holds zeros)."""
    n = _neighbours(L, x, None)
    lo = L.lo.astype(dt)
    val = L.ns.astype(dt) * x
    for d in range(3):
        val = val - lo * n[(d, -1)]
    for d in range(3):
        val = val - L.xp[d].astype(dt) * n[(d, 1)]
    return np.where(L.unk, b - val, dt(0.0)).astype(dt)


def _restrict(F, C, r, weight, dt, stale):
    """restrict_column / restrict_cell, mg.hip:572-600: pairs along z, then x, then y; halved."""
    cz, cy, cx = C.shape
    r = _padded(r, (2 * cz, 2 * cy, 2 * cx), dt(0.0))
    p = r[0::2] + r[1::2]
    p = p[:, :, 0::2] + p[:, :, 1::2]
    p = p[:, 0::2] + p[:, 1::2]
    out = (dt(weight) * p).astype(dt)
    if stale:
        off = ~_padded(np.repeat(np.repeat(np.repeat(F.act, 4, axis=0), 4, axis=1), 4, axis=2), C.shape, False)
        out = np.where(off, dt(1.0), out)
    return out


def _prolong(F, e):
    """corr, mg.hip:638: the parent's value."""
    up = np.repeat(np.repeat(np.repeat(e, 2, axis=0), 2, axis=1), 2, axis=2)
    return up[: F.shape[0], : F.shape[1], : F.shape[2]]


def vcycle(H, r, dtype=np.float64, mutant=None):
    """z = M^-1 r over the unknowns. `mutant` must be the one H was built with when it changes the hierarchy (outside_is_air)."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert mutant != "outside_is_air" or H.mutant == mutant
    dt = np.float32 if dtype == np.float32 else np.float64
    r = np.asarray(r, dtype=np.float64).astype(dt)
    Ls, last = H.levels, H.last
    omega = [MG_OMEGA] + [1.0 if mutant == "omega_coarse_1" else MG_OMEGA] * (len(Ls) - 1)
    cache = H.__dict__.setdefault("_coef", {})  # (the coefficients of a level, cast once per element type and omega)
    coef = [cache.setdefault((l, dt, omega[l]), _coef(L, omega[l], dt)) if (l, dt, omega[l]) not in cache else cache[(l, dt, omega[l])]
            for l, L in enumerate(Ls)]
    b = [None] * len(Ls)
    x = [None] * len(Ls)
    b[0] = np.zeros(Ls[0].shape, dtype=dt)
    b[0][H.index] = r
    b[0] = np.where(Ls[0].unk, b[0], dt(0.0)).astype(dt)  # (closed tiles: no part of the cycle)
    zero = [np.zeros(L.shape, dtype=dt) for L in Ls]
    weight = 0.45 if mutant == "restrict_045" else 0.5
    for l in range(last):  # down, mg.hip:2830-2870
        x[l] = _sweeps(Ls[l], zero[l], b[l], 0, 0, MG_INNER_SWEEPS, coef[l], dt)
        b[l + 1] = _restrict(Ls[l], Ls[l + 1], _residual(Ls[l], x[l], b[l], dt), weight, dt, mutant == "stale_octant")
    if last == 0:  # mg.hip:2808-2819: pre- and post-smoothing of the one level
        x[0] = _sweeps(Ls[0], zero[0], b[0], 0, 0, MG_INNER_SWEEPS, coef[0], dt)
        y = None
    else:  # coarsest_tile, mg.hip:675-697
        nsw = 1 if mutant == "coarsest_1" else MG_COARSEST_SWEEPS
        y = _sweeps(Ls[last], zero[last], b[last], 0, 0, nsw, coef[last], dt)
        y = _sweeps(Ls[last], y, b[last], 0, 1, nsw, coef[last], dt)
    for l in range(min(last - 1, len(Ls) - 1), -1, -1) if last else [0]:  # up, mg.hip:2875-2892
        L = Ls[l]
        if y is None:
            corr = zero[l]
        else:
            e = y
            if mutant == "prune_ignored_in_ring" and l == 0:
                ghost = _cells_of_tiles(H.pruned) & (Ls[1].mtype != MT_SOLID)
                e = np.where(ghost, b[1], y).astype(dt)
            corr = _prolong(L, e)
        xc = (x[l] + np.where(L.unk, corr, dt(0.0))).astype(dt)  # mg.hip:646, 654
        frozen = xc
        if mutant == "ring_uncorrected":
            frozen = x[l]
        if mutant == "ring_live":
            frozen = None
        first = 0 if mutant == "post_red_first" else 1
        y = _sweeps(L, xc, b[l], frozen, first, MG_INNER_SWEEPS, coef[l], dt)
    inv = dt(1.0 / H.a_scale)
    z = (y[H.index] * inv).astype(dt)
    for (idx, A), tile in zip(H.closed_blocks, H.closed):
        if mutant == "closed_smoothed":
            z[idx] = _smoothed_block(A, r[idx].astype(np.float64), H, idx) * float(inv)
        else:
            z[idx] = (np.linalg.solve(A, r[idx].astype(np.float64)) * float(inv)).astype(dt)
    return z.astype(np.float64)


def _smoothed_block(A, rb, H, idx):
    """MG_INNER_SWEEPS red -> black SOR sweeps from zero on a dense block (the closed_smoothed mutant)."""
    z, y, x = (c[idx] for c in H.index)
    par = (x + y + z) & 1
    v = np.zeros(len(idx))
    d = np.diag(A)
    for _ in range(MG_INNER_SWEEPS):
        for colour in (0, 1):
            m = (par == colour) & (d > 0)
            gs = (rb - (A @ v - d * v)) / np.where(d > 0, d, 1.0)
            v = np.where(m, (1.0 - MG_OMEGA) * v + MG_OMEGA * gs, v)
    return v


def apply_a(H, v):
    """A v over the unknowns, scaled (pressure_solver::_apply_a): every tile, closed ones included."""
    raw = H.raw0
    x = np.zeros(H.levels[0].shape)
    x[H.index] = v
    val = raw["ns"] * x
    for d, k in enumerate(("xp", "yp", "zp")):
        val = val - raw["lo"] * _shift(x, d, -1) - raw[k] * _shift(x, d, 1)
    return H.a_scale * val[H.index]


def open_mask(H):
    """bool over the unknowns: not in a closed tile."""
    m = np.ones(len(H.index[0]), dtype=bool)
    for idx, _ in H.closed_blocks:
        m[idx] = False
    return m


def pcg(H, b, tolerance=1e-6, max_iterations=200, mutant=None):
    """The pressure solve as the device runs it under LFA_PRECOND_MULTIGRID, in fp64 with the model as preconditioner: the closed
    tiles' blocks are solved on their own, PCG with the stopping rule of pcg.hip (the SIGNED maximum of the residual below the
    tolerance, tested behind the AXPYs; the count includes the iteration that stops: pcg.h:82-84, oracle/oracle.c orc_solve) runs
    on the rest. Returns (p, iterations)."""
    b = np.asarray(b, dtype=np.float64)
    op = open_mask(H)
    p = np.zeros(len(b))
    if float(b @ b) < 1e-6:  # src/pressure_solver.cpp:33-35
        return p, 0
    for idx, A in H.closed_blocks:
        p[idx] = np.linalg.solve(A, b[idx]) / H.a_scale
    if not op.any():
        return p, 0
    r = np.where(op, b, 0.0)
    z = np.where(op, vcycle(H, r, mutant=mutant), 0.0)
    s = z.copy()
    sigma = z @ r
    it = 0
    while it < max_iterations:
        q = np.where(op, apply_a(H, s), 0.0)
        alpha = sigma / (q @ s)
        p = p + alpha * s
        r = r - alpha * q
        it += 1
        if r[op].max() < tolerance:
            break
        z = np.where(op, vcycle(H, r, mutant=mutant), 0.0)
        sigma_new = z @ r
        s = z + (sigma_new / sigma) * s
        sigma = sigma_new
    return p, it
