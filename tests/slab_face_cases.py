"""Which designed case runs on which z-slab decomposition, and what of it crosses a slab face. Pure numpy, no GPU.

The designed inputs of tests/move_cases.py, tests/transfer_cases.py and tests/stencil_cases.py were built for one domain. This module
pairs every case with nz >= 16 with layer bounds (`init_local_slab`), counts from the ORACLE's results what crosses a slab face
(tests/test_slab_face_cases.py asserts that every class of crossing is there and prints the counts), and holds the helpers of the
slab tests (tests/test_gpu_slab_faces.py): the owner of a cell layer, stitching of owned z-ranges, poison for everything a rank
does not own, and the thread-per-rank harness.

Bounds, by number of tile layers L = ceil(nz / 8):
  L = 2   [0, 1, 2]
  L = 3   [0, 1, 3], [0, 2, 3], [0, 1, 2, 3] - the last layer of an 18- (17-) cell axis is 2 cells (1 cell) thick, so the last slab of
          [0, 2, 3] and [0, 1, 2, 3] is two cell layers or ONE cell layer thin
  L = 5   (walls_z, 9 x 10 x 40) [0, 1, 2, 5] and [0, 2, 5]: the faces z = 8 and z = 16 are the two sides of its solid tile

What is NOT run (the product family x case x bounds x method x state x vector type would be some 900 ids). The GPU file has 198
ids; they take 3 s together on an MI355X, so the number was not pressed further towards the 150 aimed at:
  moves      tile_reach_x+ is the one transverse case (y would repeat it) and runs on [0, 1, 2, 3] alone: its particles move less
             than a cell in z, the bounds only decide who holds them. Every (case, bounds) runs TWO of the 18 combinations of
             handle state x stage x method, rotated over the table so that every state meets every stage and every method (MOVE_RUNS
             of the GPU file). The three (case, bounds) of FAR_MOVES run the refusal instead. lfa_time_step runs on one split per
             ISOLATED case.
  transfers  on [0, 1, 2, 3] (or [0, 1, 2]) every method of the case; [0, 1, 3] and [0, 2, 3] get one method each, rotated
             (transfer_methods). The G2P runs on the finest split of each case only - it reads the grid through the same refresh on
             every split - and on one of the three reflected hat clouds: a gather does not care which way a hat points.
  grid       the solve runs the three preconditioners on five (case, bounds) with the vector type alternating, both types on
             maze [0, 1, 2, 3], and LFA_MG_DIST_LEVELS=1 on two; maze_h17 / maze_h05 repeat maze's field at another h and run on the
             three-slab split only; the extrapolation runs 1, 2 and 3 sweeps on six (case, bounds); k_apply_pressure alternates the
             vector type over the table instead of running both on every entry.
"""
import functools
import threading

import numpy as np

from tests import move_cases as mc
from tests import stencil_cases as sc
from tests import transfer_cases as tc

TILE = 8
B2 = ((0, 1, 2),)
B3 = ((0, 1, 3), (0, 2, 3), (0, 1, 2, 3))
B3_FINE = ((0, 1, 2, 3),)
B5 = ((0, 1, 2, 5), (0, 2, 5))

# family -> ((case, bounds of the case), ...)
MOVES = (
    ("tile_reach_z+", B3), ("tile_reach_z-", B3), ("tile_reach_x+", B3_FINE), ("obstacles", B3), ("axis_aligned", B2),
    ("walls_2_9_17", B3), ("walls_24_21_18_n513", B3), ("walls_24_21_18_n511", B3),
)
TRANSFERS = (
    ("tile_counts", B2), ("tile_counts_deferred", B2), ("contrast_21_13_18", B3), ("lattice", B3),
    ("lone_hats", B2), ("lone_hats_h17", B2), ("lone_hats_h17_unscaled", B2),
    ("lone_hats_zmirror", B2), ("lone_hats_h17_zmirror", B2), ("lone_hats_h17_unscaled_zmirror", B2),
    ("lone_hats_above_z8", B2), ("lone_hats_above_z8_zmirror", B2),
    ("thin_2_9_17", B3),
)
# Builders added to tests/transfer_cases.py for these tests (every one a reflection or a subset of an existing cloud):
#   lone_hats*_zmirror          the five hats of lone_hats* that cross z = 8 all have their particle above it; reflected, the three of
#                               them on u and v faces cross it upwards (the two on w faces land on the face itself: the w face at z = 8
#                               belongs to cell 7, where the reflected particle now sits)
#   lone_hats_above_z8(_zmirror) every tile of lone_hats holds a particle; with the particles below z = 8 taken out the lower slab of
#                               [0, 1, 2] holds none - its tiles are processed only because of the hats across the face
# Not added: a reflected `lattice`. Its fractions are 0 and 1/2, a reflection maps them onto themselves, and neither reaches the
# cell above (a particle ON a face belongs to the cell above the face and reaches down): the reflection sends nothing upwards.
# And no w contribution ever crosses upwards: the w face at z + 1 is stored in cell z, the topmost w face a particle of cell z reaches.
STENCILS = (
    ("maze", B3), ("maze_h17", B3_FINE), ("maze_h05", B3_FINE), ("sheets", B3), ("droplets", B2), ("walls_z", B5),
    ("thin_2_9_17", B3_FINE),
)
# (case, bounds) -> particles whose end owner lies two or more ranks from their start owner (tests/test_slab_face_cases.py computes
# them from the oracle): one migration hands a particle to the ADJACENT rank, so these moves are refused
FAR_MOVES = {("walls_2_9_17", (0, 1, 2, 3)): 2, ("walls_24_21_18_n513", (0, 1, 2, 3)): 53, ("walls_24_21_18_n511", (0, 1, 2, 3)): 45}
FAMILIES = {"moves": (mc, MOVES), "transfers": (tc, TRANSFERS), "stencils": (sc, STENCILS)}


def layers(nz):
    return -(-int(nz) // TILE)


def bounds_id(bounds):
    return "-".join(str(b) for b in bounds)


def table(family):
    """[(case, bounds)] of a family, every bounds a tuple."""
    return [(name, tuple(b)) for name, bb in FAMILIES[family][1] for b in bb]


def check_table():
    """Every entry names an existing case with nz >= 16 on a grid of at most 40 x 24 x 24 and bounds that partition its layers."""
    for family, (mod, rows) in FAMILIES.items():
        for name, bb in rows:
            size = mod.build(name)[0]
            assert size[2] >= 16 and size[0] <= 40 and max(size[1:]) <= 24 or name == "walls_z" and size == (9, 10, 40), (name, size)
            for b in bb:
                assert b[0] == 0 and b[-1] == layers(size[2]) and all(x < y for x, y in zip(b, b[1:])) and len(b) - 1 <= 4, (name, b)


# ---------------------------------------------------------------------------------------------------- helpers
def owner(z_cell, bounds):
    """The rank that owns cell layer z (an int or an array): the slab whose tile layers hold z // 8."""
    return np.searchsorted(np.asarray(bounds), np.asarray(z_cell) // TILE, side="right") - 1


def z_range(bounds, rank, nz):
    """The cell layers [z0, z1) of a rank."""
    return TILE * bounds[rank], min(TILE * bounds[rank + 1], int(nz))


def faces(bounds):
    """The interior slab faces, in cells."""
    return [TILE * b for b in bounds[1:-1]]


def stitch(per_rank_arrays, bounds, size):
    """One array of ncells entries (x fastest) that takes from every rank's array the rank's own cell layers."""
    nx, ny, nz = size
    first = np.asarray(per_rank_arrays[0])
    out = np.zeros_like(first)
    shape = (nz, ny, nx) + first.shape[1:]
    for r, a in enumerate(per_rank_arrays):
        z0, z1 = z_range(bounds, r, nz)
        out.reshape(shape)[z0:z1] = np.asarray(a).reshape(shape)[z0:z1]
    return out


def own_mask(bounds, rank, size):
    """bool[ncells]: the cells of the rank's own layers."""
    nx, ny, nz = size
    z0, z1 = z_range(bounds, rank, nz)
    m = np.zeros((nz, ny, nx), dtype=bool)
    m[z0:z1] = True
    return m.reshape(-1)


POISON_TYPE = 0  # neither AIR (1), FLUID (2) nor SOLID (4)


def poison_outside(cells, bounds, rank, fields, size):
    """A copy of a cell array (ncells records of a grid of `size`) in which the named fields are destroyed outside the rank's own
    cell layers: "vel" becomes NaN, "type" becomes POISON_TYPE - except on solid cells, which keep their type: an uploaded grid's
    types define the handle's solid mask, and that is the host's knowledge (set_solid_cells with the whole list on every rank),
    not a field that travels between ranks."""
    out = cells.copy()
    outside = ~own_mask(bounds, rank, size)
    for f in fields:
        if f == "vel":
            out["vel"][outside] = np.nan
        elif f == "type":
            out["type"][outside & (cells["type"] != sc.SOLID)] = POISON_TYPE
        else:
            raise KeyError(f)
    return out


def run_ranks(sims, fn, timeout=60, hub=None, raise_errors=True):
    """fn(rank, sim) on one host thread per rank (the in-process transport's collectives meet at a rendezvous). Returns
    (results per rank, [(rank, exception)]). Exceptions are collected, never raised inside a thread; no thread may be alive
    after `timeout` seconds; the handles and the hub are closed only when nothing hangs (closing a handle under a thread that
    still uses it would turn a hang into a crash). raise_errors: assert that no rank failed."""
    n = len(sims)
    results, errors = [None] * n, []

    def worker(r):
        try:
            results[r] = fn(r, sims[r])
        except Exception as e:  # noqa: BLE001
            errors.append((r, e))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    alive = any(t.is_alive() for t in threads)
    if not alive:
        for s in sims:
            s.close()
        if hub is not None:
            hub.close()
    if raise_errors:
        assert not errors, [(r, repr(e)) for r, e in errors]
    assert not alive, "slab threads hung"
    return results, sorted(errors, key=lambda re: re[0])


# ---------------------------------------------------------------------------------------------------- moves
@functools.lru_cache(maxsize=None)
def move_owners(name, bounds):
    """(start owner, end owner, end cell z) per particle id: the start from the case, the end from the oracle's collide stage."""
    size, parts, solid, meta = mc.build(name)
    top = size[2] - 1
    z0 = np.minimum(np.floor(mc.cells_of(parts["pos"], meta)[:, 2]).astype(np.int64), top)
    z1 = np.minimum(np.floor(mc.cells_of(mc.oracle(name)["collide"], meta)[:, 2]).astype(np.int64), top)
    return owner(z0, bounds), owner(z1, bounds), z1


def far_movers(name, bounds):
    """Ids of the particles whose end owner is two or more ranks from their start owner: what one migration cannot deliver."""
    a, b, _ = move_owners(name, tuple(bounds))
    return np.flatnonzero(np.abs(b - a) >= 2)


def move_counts(name, bounds):
    """The classes of tests/test_slab_face_cases.py for one (case, bounds), from the oracle."""
    bounds = tuple(bounds)
    size, parts, solid, meta = mc.build(name)
    a, b, z1 = move_owners(name, bounds)
    n = len(bounds) - 1
    start_z = mc.cells_of(parts["pos"], meta)[:, 2]
    near = np.zeros(len(parts), dtype=bool)
    for f in faces(bounds):
        near |= np.abs(start_z - f) < meta["skin"]
    # a bounce or a push-out: the end is not the free flight's clamped end
    _, _, flight = mc.free_flight((size, parts, solid, meta))
    end = mc.cells_of(mc.oracle(name)["collide"], meta)
    deflected = np.abs(end - flight).max(axis=1) > 1e-9
    first = np.isin(z1, [TILE * x for x in bounds[:-1]])
    last = np.isin(z1, [min(TILE * x, size[2]) - 1 for x in bounds[1:]])
    return dict(up_one=int((b == a + 1).sum()), down_one=int((b == a - 1).sum()),
                skin_start_crosses_deflected=int((near & deflected & (a != b)).sum()),
                ends_in_first_layer=int(first.sum()), ends_in_last_layer=int(last.sum()),
                ranks_ending_empty=int(sum((b == r).sum() == 0 for r in range(n))),
                ranks_starting_empty=int(sum((a == r).sum() == 0 for r in range(n))),
                far=int((np.abs(b - a) >= 2).sum()))


def end_face_gap(name, bounds):
    """Smallest distance (cells) of an oracle end position to a slab face: ownership of the end is only decided beyond the bar."""
    size, parts, solid, meta = mc.build(name)
    z = mc.cells_of(mc.oracle(name)["collide"], meta)[:, 2]
    return min(float(np.abs(z - f).min()) for f in faces(bounds))


# ---------------------------------------------------------------------------------------------------- transfers
def transfer_counts(name, method, bounds):
    """(particle, face) contributions whose face is stored by another rank than the particle's, per component and direction ("up":
    the face's owner is the higher rank); lone hats across a slab face by direction and fate; hats whose face lies in a tile
    across the face that holds no particle."""
    size, parts, solid, meta = tc.build(name)
    top = size[2] - 1
    pz = np.minimum(np.maximum((parts["pos"][:, 2] - meta["off"][2]) / meta["h"], 0.0).astype(np.int64), top)
    po = owner(pz, bounds)
    out = {f"{'uvw'[c]}_{d}": 0 for c in range(3) for d in ("up", "down")}
    out["into_empty_tile_up"] = out["into_empty_tile_down"] = 0
    cell = np.minimum(np.floor((parts["pos"] - np.asarray(meta["off"])) / meta["h"]).astype(np.int64), np.asarray(size) - 1)
    ntile = -(-np.asarray(size) // TILE)
    has = np.zeros(ntile, dtype=bool)
    has[tuple((cell // TILE).T)] = True
    tiles = {tuple(int(a) for a in t) for t in np.argwhere(has)}
    for comp, idx, tgt, w, _ in tc._contributions(size, parts, meta["h"], meta["off"], method):
        live = w > 0.0
        fo = owner(tgt[:, 2], bounds)
        empty = ~has[tuple((tgt // TILE).T)]
        out[f"{'uvw'[comp]}_up"] += int((live & (fo > po[idx])).sum())
        out[f"{'uvw'[comp]}_down"] += int((live & (fo < po[idx])).sum())
        out["into_empty_tile_up"] += int((live & empty & (fo > po[idx])).sum())
        out["into_empty_tile_down"] += int((live & empty & (fo < po[idx])).sum())
    for k in ("kept_up", "kept_down", "zeroed_up", "zeroed_down", "hat_into_empty_tile"):
        out[k] = 0
    if "hats" in meta:
        for hat in meta["hats"]:
            a, b = int(po[hat["index"]]), int(owner(hat["cell"][2], bounds))
            if a == b:
                continue
            out[("kept_" if hat["kept"] else "zeroed_") + ("up" if b > a else "down")] += 1
            out["hat_into_empty_tile"] += tuple(c // TILE for c in hat["cell"]) not in tiles
    return out


def hats_across(name, bounds):
    """The hats of a case whose face is stored by another rank than their particle's."""
    size, parts, solid, meta = tc.build(name)
    pz = np.minimum(np.floor((parts["pos"][:, 2] - meta["off"][2]) / meta["h"]).astype(np.int64), size[2] - 1)
    return [hat for hat in meta.get("hats", ()) if owner(pz[hat["index"]], bounds) != owner(hat["cell"][2], bounds)]


def transfer_methods(name, bounds):
    """The methods a (case, bounds) runs: all of the case's on its finest split, one (rotated) on the others."""
    methods = tc.build(name)[3]["methods"]
    rows = dict(TRANSFERS)[name]
    if tuple(bounds) == tuple(rows[-1]):
        return tuple(methods)
    k = [tuple(b) for b in rows].index(tuple(bounds)) + sorted(dict(TRANSFERS)).index(name)
    return (methods[k % len(methods)],)


# ---------------------------------------------------------------------------------------------------- grid stages
@functools.lru_cache(maxsize=None)
def oracle_extrapolation(name, sweeps):
    """The oracle's extrapolation with `sweeps` sweeps from the applied grid of stencil_cases.oracle_stages(name, True) (which
    records 1 and 3; the slab tests also run 2, where exactly one exchange of validity bytes happens)."""
    want = sc.oracle_stages(name, True)
    if sweeps in (1, 3):
        return want[f"extrap{sweeps}_vel"]
    s = sc.cpu_sim(name)
    s.hash()
    s.p2g()
    s.build_system(sc.DT)  # (the oracle's sweeps start from the unknowns of the last system)
    cells = s.cells()
    cells["vel"], cells["type"] = want["apply_vel"], want["type"]
    s.set_cells(cells)
    s.set_extrapolation_iterations(sweeps)
    s.extrapolate()
    out = s.cells()["vel"].copy()
    s.close()
    out.setflags(write=False)
    return out


def stencil_counts(name, bounds):
    """A couplings, pressure-gradient faces and extrapolation sweeps that reach across a slab face, from the oracle's stages."""
    size, parts, solid, meta = sc.build(name)
    nx, ny, nz = size
    want = sc.oracle_stages(name, True)
    fc = want["fluid_cells"].astype(np.int64)
    z = fc // (nx * ny)
    below = np.isin(z + 1, faces(bounds))  # unknowns in the last cell layer under a slab face
    out = dict(a_couplings=int((below & (((want["abits"] >> 5) & 1) == 1)).sum()))
    _, cls, _ = sc.apply_pressure_faces(size, want["type"], fc, want["grav_vel"], want["p"], sc.coeff_of(meta))
    zc = np.arange(nx * ny * nz) // (nx * ny)
    at_face = np.isin(zc + 1, faces(bounds))
    # the +z face of a cell under a slab face whose rule reads the pressure of the cell above it - the neighbour rank's
    out["apply_faces_second_pressure_across"] = int((at_face & (cls["unknown-fluid"][:, 2] | cls["air-unknown"][:, 2])).sum())
    for sweeps, key in ((1, "sweep1_from_across"), (2, "sweep2_from_sweep1_across")):
        _, written, count, born, _ = sc.extrapolate_sweeps(size, want["type"], fc, want["apply_vel"], sweeps)
        b3 = born.reshape(nz, ny, nx)
        hit = np.zeros((nz, ny, nx), dtype=bool)
        for f in faces(bounds):
            # cells of layer f - 1 and f made valid in this sweep with a neighbour across the face valid since the sweep before
            hit[f - 1] |= (b3[f - 1] == sweeps) & (b3[f] == sweeps - 1)
            hit[f] |= (b3[f] == sweeps) & (b3[f - 1] == sweeps - 1)
        out[key] = int(hit.sum())
    return out
