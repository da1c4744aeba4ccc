"""Adversarial particle clouds for the transfer kernels (k_p2g_binned, k_p2g_atomic, k_p2g_finalize, k_g2p, k_g2p_leavers) and an
fp64 weight sum per face. Pure numpy, deterministic from a seed; every builder returns (size, parts, solid, meta) with
meta = dict(h=cell size, off=grid offset, methods=the transfer methods the cloud is meant for, ...).

What the clouds are for (the kernels' own line numbers drift; the mechanisms do not):
  tile_counts   particle tiles that hold exactly P2G_THREADS +- 1, 2 P2G_THREADS +- 1, G2P_THREADS +- 1, ... particles: the guards of
                the scatter's two-rounds-ahead software pipeline and of the G2P's strided loop
  contrast      cells with 0, 1, 2, 8, 33 and 64 particles side by side on ragged grids: lane rotation, LDS atomic contention, sums
                of hundreds of terms per face
  lattice       every coordinate a multiple of 1/2: fraction 0 (on a face), exactly 1/2 (the branch between the two staggered cells)
                and 1 (the max face), in the corner cells of an interior tile, of the ragged last tile and of a tile without neighbours
  lone_hats     isolated particles whose far-corner weight on one face is 2e-6, 5e-6 (kept) or 5e-7, 2e-7 (zeroed): both sides of the
                reference's `sum w > 1e-6` (src/simulation.cpp:324,383)
  fast          velocities (and APIC affine terms) up to a given maximum: the range of the scatter's fixed-point accumulators
  thin          grids of less than a tile, down to two cells across
"""
import functools
import itertools

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from oracle import loader as orc

PIC, FLIP, APIC = 0, 1, 2
ALL_METHODS = (PIC, FLIP, APIC)
W_MIN = 1e-6          # the reference's threshold on a face's weight sum
BAND = 1e-3           # no face of any case may lie within this relative distance of it (test_transfer_cases.py)
TILE_COUNTS = (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537)
OFF_H17 = (0.3, -0.2, 0.1)


def _finish(size, cell_pos, rng, h=1.0, off=(0.0, 0.0, 0.0), vel=3.0, methods=ALL_METHODS, **meta):
    """Particles at grid positions `cell_pos` (in cells), random v and C (world units), positions pairwise different."""
    cell_pos = np.asarray(cell_pos, dtype=np.float64).reshape(-1, 3)
    n = len(cell_pos)
    parts = np.zeros(n, dtype=PARTICLE_DTYPE)
    parts["pos"] = np.asarray(off, dtype=np.float64)[None, :] + cell_pos * h
    parts["old_pos"] = parts["pos"]
    parts["vel"] = rng.normal(size=(n, 3)) * vel
    for f in ("cx", "cy", "cz"):
        parts[f] = rng.normal(size=(n, 3)) * vel * 0.1 / h
    assert len(np.unique(parts["pos"], axis=0)) == n, "particles are told apart by their positions"
    return tuple(int(s) for s in size), parts, None, dict(h=float(h), off=tuple(off), methods=tuple(methods), **meta)


def tile_counts(counts=TILE_COUNTS, deferred=False, seed=101):
    """One particle tile per entry of `counts` with exactly that many particles in randomly chosen cells of the tile (no cell is
    given more than `cap` = max(64, what the count needs)), on a 40 x 16 x 16 grid: 5 x 2 x 2 tiles, filled in tile order, the rest
    empty - so the tiles share faces with each other and with tiles that hold nothing. `deferred` only selects another draw (the
    cloud the deferred-binning test runs)."""
    size = (40, 16, 16)
    rng = np.random.default_rng(seed + (1000 if deferred else 0))
    assert len(counts) <= 20
    pos, per_tile = [], []
    for k, n in enumerate(counts):
        tx, ty, tz = k % 5, (k // 5) % 2, k // 10
        cap = max(64, -(-n // 512))
        cells = rng.integers(0, 512, size=n)
        while np.bincount(cells, minlength=512).max() > cap:
            cells = rng.integers(0, 512, size=n)
        lc = np.stack([cells & 7, (cells >> 3) & 7, cells >> 6], axis=1)
        pos.append(np.array([tx, ty, tz]) * 8 + lc + rng.random((n, 3)))
        per_tile.append(((tx, ty, tz), int(n)))
    return _finish(size, np.concatenate(pos), rng, per_tile=per_tile, deferred=bool(deferred))


def _contrast_positions(size, rng, choices):
    nx, ny, nz = size
    cnt = rng.choice(np.asarray(choices), size=nx * ny * nz)
    raw = np.repeat(np.arange(nx * ny * nz), cnt)
    cell = np.stack([raw % nx, (raw // nx) % ny, raw // (nx * ny)], axis=1)
    return cell + rng.random((len(raw), 3))


def contrast(size, h=1.0, off=(0.0, 0.0, 0.0), seed=202):
    """Particles per cell drawn from {0, 0, 1, 2, 8, 33, 64}; the sizes in use, (21, 13, 18) and (9, 8, 7), are ragged."""
    rng = np.random.default_rng(seed)
    return _finish(size, _contrast_positions(size, rng, (0, 0, 1, 2, 8, 33, 64)), rng, h=h, off=off)


def _half_lattice(lo, hi):
    """All positions with coordinates lo, lo + 1/2, ..., hi (inclusive) per axis, as integers in half cells."""
    ax = [np.arange(int(round(2 * a)), int(round(2 * b)) + 1) for a, b in zip(lo, hi)]
    g = np.meshgrid(*ax, indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)


def lattice(size=(40, 21, 18), seed=303):
    """Every coordinate a multiple of 1/2 (0 and the max faces included), one particle per position:
    - cells 7 .. 16 of every axis, i.e. tile (1, 1, 1) and a layer of each of its 26 neighbours: the eight corner cells of an
      INTERIOR tile, whose faces k_p2g_finalize sums from eight staging blocks;
    - the last tile in x, y and z (ragged in y and z for the default size) up to and including the max faces;
    - the last tile in x at y = z = 0, filled up to its last half cell: a tile none of whose neighbours holds a particle;
    - a few positions on the x = 0 face."""
    nx, ny, nz = size
    assert nx >= 40 and nx % 8 == 0 and ny >= 21 and nz >= 18 and (ny % 8 or nz % 8)
    tx, ty, tz = (nx - 1) // 8, (ny - 1) // 8, (nz - 1) // 8
    assert tx >= 4 and ty >= 2 and tz >= 2
    boxes = [((7, 7, 7), (17, 17, 17)),
             ((8 * tx, 8 * ty, 8 * tz), (nx, ny, nz)),
             ((8 * tx, 0, 0), (nx - 0.5, 7.5, 7.5)),
             ((0, 8, 8), (1, 10, 10))]
    half = np.unique(np.concatenate([_half_lattice(lo, hi) for lo, hi in boxes]), axis=0)
    rng = np.random.default_rng(seed)
    return _finish(size, half * 0.5, rng, h=1.0, interior_tile=(1, 1, 1), ragged_tile=(tx, ty, tz), lonely_tile=(tx, 0, 0))


LONE_TARGETS = ((2e-6, True), (5e-6, True), (5e-7, False), (2e-7, False))  # (far-corner weight, kept by the threshold)


def lone_hats(h=1.0, unscaled=False, seed=404):
    """Isolated particles, 4 cells apart (a hat reaches 2 cells: no face sees two of them). The in-cell fractions of particle k put
    a prescribed weight on ONE face: the far corner of the hat of one velocity component. `unscaled`: the hat APIC uses at
    cell_size != 1, max(0, 1 - |p - face|) on world-space distances (src/simulation.cpp:367-369) - a narrower hat for h > 1, for
    which such weights are routine; otherwise the hat on distances in cells that PIC and FLIP (and APIC at h = 1) use.
    Per axis the weight towards the face is e_a (their product is the target): with hh = h (unscaled) or 1,
      low side  (face cell = particle cell - 1 on every axis):            own axis t = (1 - e) / hh,     others t = (1 - e) / hh - 1/2
      high side (face cell = particle cell on the own axis, + 1 on the others):   t = 1 - (1 - e) / hh,      t = 3/2 - (1 - e) / hh
    meta["hats"]: one dict per particle (index, comp, face cell, target weight, kept). Half of the particles sit in the corner cell
    of a tile, so that their far face lies in a tile that holds no particle."""
    size = (24, 16, 16)
    hh = float(h) if unscaled else 1.0
    assert 1.0 <= hh < 1.9
    rng = np.random.default_rng(seed)
    slots = [(x, y, z) for z in (4, 8, 12) for y in (4, 8, 12) for x in (4, 8, 12, 16, 20)]
    pos, hats = [], []
    combos = [(comp, high, tgt, kept) for comp in range(3) for high in (False, True) for tgt, kept in LONE_TARGETS]
    assert len(combos) <= len(slots)
    for k, (comp, high, tgt, kept) in enumerate(combos):
        cell = np.array(slots[(7 * k) % len(slots)])  # (7 and 45 are coprime: every slot at most once)
        e = tgt ** (1.0 / 3.0) * np.roll([1.3, 1.0 / 1.3, 1.0], k)
        t = np.empty(3)
        face = cell.copy()
        for a in range(3):
            reach = (1.0 - e[a]) / hh
            if a == comp:
                t[a] = 1.0 - reach if high else reach
                face[a] += 0 if high else -1
            else:
                t[a] = 1.5 - reach if high else reach - 0.5
                face[a] += 1 if high else -1
        assert (t > 0).all() and (t < 1).all()
        pos.append(cell + t)
        hats.append(dict(index=k, comp=comp, cell=tuple(int(c) for c in face), target=tgt, kept=kept))
    methods = (APIC,) if unscaled else (ALL_METHODS if h == 1.0 else (PIC, FLIP))
    size, parts, solid, meta = _finish(size, np.array(pos), rng, h=h, off=(0.0, 0.0, 0.0) if h == 1.0 else OFF_H17,
                                       methods=methods, hats=hats, unscaled=bool(unscaled))
    # no component near zero: "the face is not zero" must mean something
    parts["vel"] = np.where(parts["vel"] < 0, -1.0, 1.0) * (1.0 + np.abs(parts["vel"]))
    return size, parts, solid, meta


def zmirror(cloud):
    """A cloud reflected z -> nz - z (in cells; world z -> 2 off_z + nz h - z): what went down across a cell face goes up. Velocities and C
    stay as drawn (the cloud need not be the mirror image of a flow, only put its weights on the mirrored faces). The hats' face
    cells are reflected with the staggering: the w face of cell z lies at z + 1, so it becomes the w face of cell nz - 2 - z; a u or
    v face at z + 1/2 becomes the one of cell nz - 1 - z. Metadata that names tiles is dropped (nz need not be a whole number of
    tiles); meta["zmirror"] = True."""
    size, parts, solid, meta = cloud
    assert solid is None
    nz, h, off = size[2], meta["h"], meta["off"]
    parts = parts.copy()
    parts["pos"][:, 2] = (2.0 * off[2] + nz * h) - parts["pos"][:, 2]
    parts["old_pos"] = parts["pos"]
    meta = {k: v for k, v in meta.items() if k not in ("interior_tile", "ragged_tile", "lonely_tile", "per_tile")}
    if "hats" in meta:
        meta["hats"] = [dict(hat, cell=(hat["cell"][0], hat["cell"][1], nz - (2 if hat["comp"] == 2 else 1) - hat["cell"][2]))
                        for hat in meta["hats"]]
    meta["zmirror"] = True
    assert len(np.unique(parts["pos"], axis=0)) == len(parts)
    return size, parts, solid, meta


def above(cloud, z):
    """The particles of a cloud in the cell layers >= z, the hats' indices following them."""
    size, parts, solid, meta = cloud
    keep = np.floor((parts["pos"][:, 2] - meta["off"][2]) / meta["h"]) >= z
    new = np.cumsum(keep) - 1
    meta = dict(meta)
    if "hats" in meta:
        meta["hats"] = [dict(hat, index=int(new[hat["index"]])) for hat in meta["hats"] if keep[hat["index"]]]
    return size, parts[keep].copy(), solid, meta


def fast(vmax, seed=505, h=1.0):
    """The (9, 8, 7) contrast cloud with velocity components uniform in [-vmax, vmax] and C entries uniform in [-vmax, vmax] / (3 h):
    the affine term c . (face - p) of a face one cell away adds up to the same magnitude."""
    size = (9, 8, 7)
    rng = np.random.default_rng(seed)
    size, parts, solid, meta = _finish(size, _contrast_positions(size, rng, (0, 0, 1, 2, 8, 33, 64)), rng, h=h)
    n = len(parts)
    parts["vel"] = rng.uniform(-1.0, 1.0, size=(n, 3)) * vmax
    for f in ("cx", "cy", "cz"):
        parts[f] = rng.uniform(-1.0, 1.0, size=(n, 3)) * (vmax / (3.0 * h))
    meta["vmax"] = float(vmax)
    return size, parts, solid, meta


def thin(size, seed=606):
    """Grids below one tile: (2, 9, 17) and (17, 2, 9) have an axis of two cells - in the G2P's clamped sampling the last cell of an
    axis counts as clamped, so only one layer of faces is live there -, (5, 5, 5) fits a tile with room to spare. Contrast counts,
    and every tenth particle snapped to the half-cell lattice (faces, cell centres, the max faces).
    (The reference accepts all three sizes: none had to be dropped.)"""
    rng = np.random.default_rng(seed + sum(size))
    pos = _contrast_positions(size, rng, (0, 1, 2, 8, 33))
    snapped = np.unique(np.round(pos[::10] * 2.0 + rng.integers(0, 2, size=pos[::10].shape)) * 0.5, axis=0)
    snapped = np.minimum(snapped, np.asarray(size, dtype=np.float64))
    pos = np.concatenate([np.delete(pos, np.s_[::10], axis=0), np.unique(snapped, axis=0)])
    return _finish(size, pos, rng)


# ---------------------------------------------------------------------------------------------------- fp64 weights
def _contributions(size, parts, h, off, method):
    """The (particle, face) pairs of the reference's gather (every cell visits the particles of its clamped 27-cell neighbourhood,
    include/fluid/simulation.h:212-223), as a scatter: yields (comp, particle indices, target cells int[k, 3], weights, face - p)."""
    n = np.asarray(size, dtype=np.int64)
    off = np.asarray(off, dtype=np.float64)
    pos = parts["pos"]
    cell = np.minimum(np.maximum((pos - off) / h, 0.0).astype(np.int64), n - 1)  # src/simulation.cpp:251-264
    scale = 1.0 if method == APIC else 1.0 / h  # APIC: the hat on world-space distances (the un-scaled one for h != 1)
    idx = np.arange(len(pos))
    for comp in range(3):
        stag = np.full(3, 0.5)
        stag[comp] = 1.0
        for o in itertools.product((-1, 0, 1), repeat=3):
            tgt = cell + np.asarray(o)
            ok = ((tgt >= 0) & (tgt < n)).all(axis=1)
            d = off + (tgt[ok] + stag) * h - pos[ok]
            w = np.prod(np.maximum(0.0, 1.0 - np.abs(d * scale)), axis=1)
            yield comp, idx[ok], tgt[ok], w, d


def face_weight_sums(size, parts, h=1.0, off=(0.0, 0.0, 0.0), method=PIC):
    """fp64 `sum w` of every face component, float64[ncells, 3] in the order of cells()["vel"] (x fastest): the staggered trilinear
    hat, the un-scaled one for APIC. Only ever used to tell on which side of 1e-6 a face lies - never as an expected velocity."""
    nx, ny, nz = size
    out = np.zeros((nx * ny * nz, 3))
    for comp, _, tgt, w, _ in _contributions(size, parts, h, off, method):
        np.add.at(out[:, comp], tgt[:, 0] + nx * (tgt[:, 1] + ny * tgt[:, 2]), w)
    return out


def max_single_wv(size, parts, h=1.0, off=(0.0, 0.0, 0.0), method=APIC):
    """max |w (v + c . (face - p))| over every single (particle, face) contribution (PIC / FLIP: max |w v|): what the LDS-binned
    scatter converts to fixed point, valid below 2^15."""
    m = 0.0
    for comp, i, _, w, d in _contributions(size, parts, h, off, method):
        val = parts["vel"][i, comp]
        if method == APIC:
            val = val + (parts[("cx", "cy", "cz")[comp]][i] * d).sum(axis=1)
        if len(w):
            m = max(m, float(np.abs(w * val).max()))
    return m


# ---------------------------------------------------------------------------------------------------- the cases
CASES = {
    "tile_counts": lambda: tile_counts(TILE_COUNTS, False),
    "tile_counts_deferred": lambda: tile_counts(TILE_COUNTS, True),
    "contrast_21_13_18": lambda: contrast((21, 13, 18)),
    "contrast_9_8_7": lambda: contrast((9, 8, 7)),
    "contrast_9_8_7_h17": lambda: contrast((9, 8, 7), h=1.7, off=OFF_H17, seed=203),
    "lattice": lattice,
    "lone_hats": lambda: lone_hats(1.0, False),
    "lone_hats_h17": lambda: lone_hats(1.7, False),
    "lone_hats_h17_unscaled": lambda: lone_hats(1.7, True),
    "fast_2000": lambda: fast(2000.0),
    "thin_2_9_17": lambda: thin((2, 9, 17)),
    "thin_17_2_9": lambda: thin((17, 2, 9)),
    "thin_5_5_5": lambda: thin((5, 5, 5)),
    # (tests/slab_face_cases.py: the hats of the originals that cross z = 8 all cross it downwards; these cross it upwards. A
    # mirrored `lattice` would not: a fraction of 0 or 1/2 never reaches the cell above, mirrored or not)
    "lone_hats_zmirror": lambda: zmirror(lone_hats(1.0, False)),
    "lone_hats_h17_zmirror": lambda: zmirror(lone_hats(1.7, False)),
    "lone_hats_h17_unscaled_zmirror": lambda: zmirror(lone_hats(1.7, True)),
    # nothing below (mirrored: above) z = 8: the hats across that face end in tiles of a layer that holds no particle at all
    "lone_hats_above_z8": lambda: above(lone_hats(1.0, False), 8),
    "lone_hats_above_z8_zmirror": lambda: zmirror(above(lone_hats(1.0, False), 8)),
}


@functools.lru_cache(maxsize=None)
def build(name):
    """(size, parts, solid, meta) of a case; cached - callers copy `parts` before they change it."""
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


def case_methods():
    """Every (case, method) pair the tests run, in a stable order."""
    return [(name, m) for name in CASES for m in build(name)[3]["methods"]]


def method_id(m):
    return ("pic", "flip", "apic")[m]


BLEND = {PIC: 1.0, FLIP: 0.95, APIC: 1.0}
DT = 0.01


def order_by_position(parts):
    p = parts["pos"]
    return np.lexsort((p[:, 2], p[:, 1], p[:, 0]))


def staged(name, method, kind="oracle"):
    """hash, P2G, gravity, extrapolation and G2P of a case on the oracle or the reference, every stage recorded; particle arrays
    in the order of the case's `parts`. (No pressure solve: the transfers are what is compared, and a grid that has not been
    projected is as good an input to the G2P as one that has.)"""
    return staged_cloud(build(name), method, kind)


def staged_cloud(cloud, method, kind="oracle"):
    size, parts, solid, meta = cloud
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=method, blending=BLEND[method], kind=kind)
    if solid is not None:
        s.set_solid_cells(solid)
    s.set_particles(parts)
    out = {}
    s.hash()
    out["fluid_cells"] = s.fluid_cells()
    out["counts"] = s.space_hash()[1].astype(np.uint32)
    s.p2g()
    cells = s.cells()
    out["p2g_vel"], out["p2g_type"] = cells["vel"].copy(), cells["type"].copy()
    if method == FLIP:
        out["old_vel"] = s.old_cells()["vel"].copy()
    s.add_gravity(DT)
    out["grav_vel"] = s.cells()["vel"].copy()
    s.build_system(DT)
    s.extrapolate()
    cells = s.cells()
    out["extrap_vel"], out["extrap_type"] = cells["vel"].copy(), cells["type"].copy()
    s.g2p()
    after = s.particles()
    back = np.empty(len(parts), dtype=np.int64)
    back[order_by_position(parts)] = order_by_position(after)  # after[back[i]] is input particle i
    after = after[back]
    assert np.array_equal(after["pos"], parts["pos"])
    out["g2p_vel"] = after["vel"].copy()
    out["g2p_c"] = np.concatenate([after["cx"], after["cy"], after["cz"]], axis=1)
    out["cfl"] = np.float64(s.cfl())
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_stages(name, method):
    """staged(..., "oracle"), computed once per (case, method) and shared; treat the arrays as read-only."""
    out = staged(name, method, "oracle")
    for v in out.values():
        if isinstance(v, np.ndarray) and v.ndim:
            v.setflags(write=False)
    return out


def crowded_tiles(seed=707):
    """The cloud of the stale-order G2P test: 32 particles per cell in a block of 2 x 2 x 2 tiles (the position correction pushes
    hundreds of them out of every one of these tiles), two cells of 32 beside a tile face in a tile of their own (a few dozen leave),
    and a tile with three far-apart particles (none has a neighbour: none moves)."""
    size = (40, 24, 24)
    rng = np.random.default_rng(seed)
    raw = np.repeat(np.arange(16 ** 3), 32)
    block = np.stack([8 + raw % 16, (raw // 16) % 16, raw // 256], axis=1) + rng.random((len(raw), 3))
    pair = np.repeat(np.array([[32, 20, 20], [33, 20, 20]]), 32, axis=0) + rng.random((64, 3))
    lone = np.array([[34.5, 3.5, 18.5], [37.5, 5.5, 21.5], [35.5, 1.5, 22.5]])
    return _finish(size, np.concatenate([block, pair, lone]), rng, vel=3.0)
