"""GPU tests (-m gpu) of the z-slab decomposition at the bars of the stages it changes: the designed moves, clouds and cell fields of
tests/move_cases.py, tests/transfer_cases.py and tests/stencil_cases.py on N <= 4 virtual slabs (N handles on one GPU, one host
thread each, lfa.LocalHub), every rank handed the whole cloud. tests/slab_face_cases.py says which case runs on which bounds and
tests/test_slab_face_cases.py shows, from the oracle, what of each crosses a slab face.

No bar here is new: 2e-5 h for positions (tests/test_gpu_move_edges.py), VEL_REL, P_REL (tests/test_gpu_parity.py), C_REL and
g2p_bar (tests/test_gpu_transfer_edges.py), K_APPLY, K_APPLY_TWICE, K_EXTRAP roundings per face (tests/test_gpu_stencil_edges.py), the
correction's flat bar (tests/test_gpu_correction_edges.py), 1e-6 / 1e-13 for b and the matrix probe, 1e-4 for the CFL figure.
What a rank owns is read from that rank: the ranks' own cell layers are stitched, particles are joined by id.

Entry points on a slab handle (established from the code, csrc/core.hip, pcg.hip, grid_ops.hip, and used accordingly):
  upload_cells      writes the whole grid of the rank, ghost layers included, and derives the solid mask from the types - so the poison
                    outside a rank's layers spares solid cells. It does not touch the particle counts.
  counts, types     of the neighbour's adjacent tile layer arrive in lfa_build_system alone (lfa_dist_refresh_grid(true)); the
                    extrapolation and the G2P refresh velocities only. A stage test that starts at k_extrapolate therefore runs
                    build_system first and uploads its poisoned input after it; FLIP's G2P does the same for the old grid.
  upload_pressure,  take and return the rank's OWN unknowns (ascending raw index, i.e. the oracle's list cut at the slab faces);
  apply_a, b ...    apply_a exchanges the slices itself.
  lfa_cfl           is local to a rank: the job's figure is the minimum over the ranks.
  advect_collide,   complete a deferred binning before they move anything (they read v), so the migration behind them never sees one:
  advect            the `from` / `vc_extent` paths of k_pack_leavers / k_unpack_arrivals run behind correct_collide (and in
                    lfa_time_step's second migration). test_correction_migrants_keep_v_and_c goes that way; the move stages still run
                    from all three handle states.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts, every solve `ITERS ...` (pytest -s shows them;
docs/experiments.md records them)."""
import functools
import itertools
import time

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import correction_cases as cc
from tests import move_cases as mc
from tests import slab_face_cases as sf
from tests import stencil_cases as sc
from tests import transfer_cases as tc
from tests.test_gpu_correction_edges import bar_of as corr_bar_of, close as close_corr
from tests.test_gpu_move_edges import close as close_pos, device_fused
from tests.test_gpu_parity import P_REL, VEL_REL, cells_from
from tests.test_gpu_stencil_edges import DTYPE_ID, EPS, K_APPLY, K_APPLY_TWICE, K_EXTRAP, PRECOND_ID, PRECONDS, pointwise
from tests.test_gpu_transfer_edges import C_REL, c_of, close, g2p_bar

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -6  # LFA_E_UNSUPPORTED (include/libfluid_amd.h)
METHOD_OF = {tc.PIC: lfa.PIC, tc.FLIP: lfa.FLIP_BLEND, tc.APIC: lfa.APIC}


def make_ranks(cloud, bounds, method, blending, **extra):
    """One handle per slab of `bounds`, each with the case's grid, solids and the WHOLE cloud: a rank keeps what lies in its layers,
    ids are upload indices. Returns (hub, handles)."""
    size, parts, solid, meta = cloud
    n = len(bounds) - 1
    assert n <= 4
    hub = lfa.LocalHub(n)
    sims = []
    for r in range(n):
        s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], density=meta.get("rho", 1.0), method=method, blending=blending, **extra)
        if solid is not None:
            s.set_solid_cells(solid)
        s.init_local_slab(hub.h, r, list(bounds))
        s.upload_particles(parts)
        sims.append(s)
    return hub, sims


def by_id(results, n):
    """The ranks' downloads joined by particle id: every id exactly once. Returns (records in id order, rank of each id)."""
    ids = np.concatenate([res["ids"] for res in results]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(n)), "a particle was lost or is resident on two ranks"
    rec = np.concatenate([res["parts"] for res in results])
    rank = np.concatenate([np.full(len(res["ids"]), r) for r, res in enumerate(results)])
    back = np.empty(n, dtype=np.int64)
    back[ids] = np.arange(n)
    return rec[back], rank[back]


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ====================================================================================================== moves and migration
MOVE_STATES = ("upload", "hash", "hash_p2g")
MOVE_STAGES = ("fused", "split")
MOVE_METHODS = (lfa.FLIP_BLEND, lfa.PIC, lfa.APIC)  # FLIP and PIC keep C in its home array (c_home), APIC carries it in the record
MOVE_METHOD_ID = {lfa.FLIP_BLEND: "flip", lfa.PIC: "pic", lfa.APIC: "apic"}
MOVE_COMBOS = list(itertools.product(MOVE_STATES, MOVE_STAGES, MOVE_METHODS))
NEAR_MOVES = [(n, b) for n, b in sf.table("moves") if (n, b) not in sf.FAR_MOVES]
# two of the 18 combinations per (case, bounds): 7 and 18 are coprime, so the 17 entries walk through 17 different first picks, and
# the second pick (+10) differs from the first in state, stage and method
MOVE_RUNS = [(n, b) + MOVE_COMBOS[(7 * k + j) % 18] for k, (n, b) in enumerate(NEAR_MOVES) for j in (0, 10)]


def move_id(run):
    name, bounds, state, stage, method = run
    return f"{name}-{sf.bounds_id(bounds)}-{state}-{stage}-{MOVE_METHOD_ID[method]}"


def tagged(parts):
    """The case's particles with every C entry but the id in cx[:, 0] drawn at random (fp32 values: the device holds them exactly).
    The move stages read neither v's history nor C; whatever comes back must be what went in."""
    rng = np.random.default_rng(len(parts))
    out = parts.copy()
    c = rng.normal(size=(len(parts), 9)).astype(np.float32).astype(np.float64)
    out["cx"][:, 1:] = c[:, 1:3]
    out["cy"], out["cz"] = c[:, 3:6], c[:, 6:9]
    return out


def blend_of(method):
    return mc.BLEND if method == lfa.FLIP_BLEND else 1.0


@functools.lru_cache(maxsize=None)
def device_split(name):
    """advect, then collide on ONE domain: what the split stages of the slab ranks must reproduce bit for bit."""
    size, parts, solid, meta = mc.build(name)
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=mc.BLEND)
    if solid is not None:
        s.set_solid_cells(solid)
    s.upload_particles(parts)
    s.advect(meta["dt"])
    s.collide()
    out = s.download_particles(into=parts.copy(), write_positions=True)
    s.close()
    return out


def end_cells(pos, size, meta):
    return np.minimum(np.floor(mc.cells_of(pos, meta)).astype(np.int64), np.asarray(size) - 1)


@pytest.mark.parametrize("run", MOVE_RUNS, ids=move_id)
def test_moves_hand_every_particle_to_the_owner_of_its_end_cell(run):
    """advect_collide, or advect and collide, on slabs from three handle states: straight after the upload, after hash() and after
    hash(); p2g(). The union of the ranks' downloads by id: every id once, positions within 2e-5 h of the oracle and BIT-IDENTICAL
    to the single domain's (the kernels read the particle's own record and the solid mask, nothing a decomposition changes),
    old_pos == pos, v and C exactly what was uploaded; every particle resident on the owner of its end cell's layer, the ranks'
    particle counts the oracle's, and after hash() the ranks' own cell counts, stitched, the oracle's."""
    name, bounds, state, stage, method = run
    size, parts, solid, meta = mc.build(name)
    up = tagged(parts)
    hub, sims = make_ranks((size, up, solid, meta), bounds, method, blend_of(method))
    label = move_id(run)

    def fn(r, s):
        if state != "upload":
            s.hash()
        if state == "hash_p2g":
            s.p2g()
        if stage == "fused":
            s.advect_collide(meta["dt"])
        else:
            s.advect(meta["dt"])
            s.collide()
        # (a slab handle refuses a download before its first binning - ids and records pair up through it -, and until then its
        # particle count is the extent of the array, the leavers' holes included: both are read behind the hash, which moves nobody)
        n_before = s.num_particles
        s.hash()
        return dict(n_before=n_before, n=s.num_particles, parts=s.download_particles(), ids=s.particle_ids(), counts=s.cell_counts())

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    got, rank = by_id(results, len(parts))
    want = mc.oracle(name)["collide"]
    close_pos(got["pos"], want, meta["h"], f"{label} positions")
    one = device_fused(name) if stage == "fused" else device_split(name)
    assert np.array_equal(got["pos"], one["pos"]), f"{label}: {int((got['pos'] != one['pos']).any(axis=1).sum())} positions differ from the single domain's"
    assert np.array_equal(got["pos"], got["old_pos"])
    assert np.array_equal(got["vel"], up["vel"]), label
    assert np.array_equal(c_of(got), c_of(up)), label
    # residence: by the device's own end cell, and that is the oracle's owner (no oracle end lies within the bar of a slab face)
    cell = end_cells(got["pos"], size, meta)
    assert np.array_equal(rank, sf.owner(cell[:, 2], bounds)), label
    start, end, _ = sf.move_owners(name, bounds)
    assert np.array_equal(rank, end), label
    n_ranks = len(bounds) - 1
    assert [res["n"] for res in results] == [int((end == r).sum()) for r in range(n_ranks)], label
    if state != "upload":  # a binned handle's count follows the hand-over at once
        assert [res["n_before"] for res in results] == [res["n"] for res in results], label
    print(f"MOVED {label} per rank before {[int((start == r).sum()) for r in range(n_ranks)]} after {[res['n'] for res in results]}")
    nx, ny, nz = size
    ocell = end_cells(want, size, meta)
    ocounts = np.bincount(ocell[:, 0] + nx * (ocell[:, 1] + ny * ocell[:, 2]), minlength=nx * ny * nz).astype(np.uint32)
    assert np.array_equal(sf.stitch([res["counts"] for res in results], bounds, size), ocounts), label


STEP_RUNS = [("tile_reach_z+", (0, 1, 2, 3)), ("tile_reach_z-", (0, 1, 2, 3)), ("tile_reach_x+", (0, 1, 2, 3)), ("walls_2_9_17", (0, 1, 3)),
             ("walls_24_21_18_n513", (0, 1, 3)), ("walls_24_21_18_n511", (0, 2, 3))]


@pytest.mark.parametrize("name,bounds", STEP_RUNS, ids=[f"{n}-{sf.bounds_id(b)}" for n, b in STEP_RUNS])
def test_full_time_step_on_slabs(name, bounds):
    """One lfa_time_step of an ISOLATED case (the particles stay 2 cells apart: the correction moves nobody) against the oracle's
    time_step at 2e-5 h, as test_gpu_move_edges.py::test_full_time_step does on one domain; every id once, resident on its end
    cell's owner."""
    assert name in mc.ISOLATED and (name, bounds) not in sf.FAR_MOVES
    cloud = mc.build(name)
    size, parts, solid, meta = cloud
    hub, sims = make_ranks(cloud, bounds, lfa.FLIP_BLEND, mc.BLEND)

    def fn(r, s):
        res, it, rc = s.time_step(meta["dt"])
        assert rc >= 0
        return dict(parts=s.download_particles(), ids=s.particle_ids())

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    got, rank = by_id(results, len(parts))
    assert np.array_equal(got["cx"][:, 0], np.arange(len(parts)))
    close_pos(got["pos"], mc.oracle_time_step(name), meta["h"], f"{name} {sf.bounds_id(bounds)} time_step")
    assert np.array_equal(rank, sf.owner(end_cells(got["pos"], size, meta)[:, 2], bounds))


@pytest.mark.parametrize("method", MOVE_METHODS, ids=MOVE_METHOD_ID.get)
def test_correction_migrants_keep_v_and_c(method):
    """hash(); correct_collide(): the one stage that migrates while the binning is still deferred - v (and APIC's C) of a leaver
    are read through the binning's source index, an arrival's go behind the other buffer's records. correction_cases' `solids` on
    three slabs pushes particles across both faces: positions at the correction's bar, v and C per id exactly what was uploaded,
    everybody resident where it ended."""
    name, bounds = "solids", (0, 1, 2, 3)
    size, parts, solid, meta = cc.build(name)
    up = tagged(parts)
    up["vel"] = np.random.default_rng(3).normal(size=(len(parts), 3)).astype(np.float32)
    hub, sims = make_ranks((size, up, solid, meta), bounds, method, cc.BLEND if method == lfa.FLIP_BLEND else 1.0)

    def fn(r, s):
        s.hash()
        s.correct_collide(cc.DT)
        return dict(parts=s.download_particles(), ids=s.particle_ids())

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    got, rank = by_id(results, len(parts))
    label = f"{name} {sf.bounds_id(bounds)} {MOVE_METHOD_ID[method]} hash,correct_collide"
    want = cc.oracle(name)["collide"]
    close_corr(got["pos"], want, corr_bar_of(name), f"{label} positions")
    assert np.array_equal(got["vel"], up["vel"]), f"{label}: {int((got['vel'] != up['vel']).any(axis=1).sum())} velocities changed"
    assert np.array_equal(c_of(got), c_of(up)), label
    top = size[2] - 1
    home = sf.owner(np.minimum(np.floor(cc.cells_of(parts["pos"], meta)[:, 2]).astype(np.int64), top), bounds)
    end = sf.owner(np.minimum(np.floor(cc.cells_of(want, meta)[:, 2]).astype(np.int64), top), bounds)
    assert np.array_equal(rank, end)
    print(f"MOVED {label} up {int((end > home).sum())} down {int((end < home).sum())}")
    assert (end != home).sum() >= 2  # (the dumbbells of `solids` across a face push their ends away from it)


FAR_RUNS = [(n, b, how) for (n, b) in sf.FAR_MOVES for how in ("advect_collide", "advect,collide", "time_step")]


@pytest.mark.parametrize("name,bounds,how", FAR_RUNS, ids=[f"{n}-{sf.bounds_id(b)}-{h}" for n, b, h in FAR_RUNS])
def test_a_move_beyond_the_adjacent_slab_is_refused(name, bounds, how):
    """The far set of tests/test_slab_face_cases.py: particles whose end owner lies two ranks from their start owner (free flight over
    a one-layer slab plus the clamp). A migration hands a particle to the adjacent rank only, so the rank that holds such a particle
    returns LFA_E_UNSUPPORTED - naming the move and the neighbour's thickness - before any record is packed, and breaks the
    transport: the other ranks fail in their next exchange instead of waiting 20 s for a rank that has left. Nobody hangs, no
    rank reports success, the whole thing takes well under the hub's time-out."""
    cloud = mc.build(name)
    size, parts, solid, meta = cloud
    far = sf.far_movers(name, bounds)
    assert len(far) == sf.FAR_MOVES[(name, bounds)]
    holders = sorted(set(int(r) for r in sf.move_owners(name, bounds)[0][far]))
    hub, sims = make_ranks(cloud, bounds, lfa.FLIP_BLEND, mc.BLEND)

    def fn(r, s):
        if how == "advect_collide":
            s.advect_collide(meta["dt"])
        elif how == "time_step":
            s.time_step(meta["dt"])
        else:
            s.advect(meta["dt"])  # (moves, hands nobody over)
            s.collide()
        return "done"

    t0 = time.monotonic()
    results, errors = sf.run_ranks(sims, fn, hub=hub, raise_errors=False)
    took = time.monotonic() - t0
    print(f"REFUSED {name} {sf.bounds_id(bounds)} {how}: {len(far)} far movers on ranks {holders}, {took:.2f} s, " +
          "; ".join(f"rank {r}: {str(e)[:150]}" for r, e in errors))
    assert results == [None] * len(sims), results
    assert [r for r, _ in errors] == list(range(len(sims)))
    assert all(isinstance(e, lfa.LibfluidError) for _, e in errors), errors
    refusing = [r for r, e in errors if e.code == E_UNSUPPORTED]
    assert refusing == holders, (refusing, holders)
    for r, e in errors:
        if r in holders:
            assert "beyond the adjacent slab" in str(e) and "layers thick" in str(e), str(e)
    assert took < 10.0, took  # (the hub gives a missing rank 20 s)


# ====================================================================================================== transfers
# (tile_counts_deferred is the deferred-binning test's cloud and runs there)
P2G_RUNS = [(n, b, m) for n, b in sf.table("transfers") if n != "tile_counts_deferred" for m in sf.transfer_methods(n, b)]


def transfer_id(run):
    return f"{run[0]}-{sf.bounds_id(run[1])}-{tc.method_id(run[2])}"


def p2g_on_rank(s, method):
    out = {}
    s.hash()
    out["fluid_cells"], out["counts"] = s.fluid_cells(), s.cell_counts()
    before = s.solver_stats()["p2g_deferred_scatters"]
    s.p2g()
    out["deferred"] = s.solver_stats()["p2g_deferred_scatters"] - before
    cells = s.cells()
    out["p2g_vel"], out["p2g_type"] = cells["vel"].copy(), cells["type"].copy()
    if method == tc.FLIP:
        out["old_vel"] = s.old_cells()["vel"].copy()
    s.add_gravity(tc.DT)
    out["grav_vel"] = s.cells()["vel"].copy()
    out["n"] = s.num_particles
    return out


def check_stitched_p2g(results, want, bounds, size, method, label):
    """test_gpu_transfer_edges.check_p2g on the ranks' own layers: fluid cells (the ranks' lists, concatenated, ARE the oracle's list:
    raw indices ascend with z), counts and types exact, the face velocities at VEL_REL."""
    assert np.array_equal(np.concatenate([res["fluid_cells"] for res in results]), want["fluid_cells"]), label
    own = lambda k: sf.stitch([res[k] for res in results], bounds, size)
    assert np.array_equal(own("counts"), want["counts"]), label
    assert np.array_equal(own("p2g_type"), want["p2g_type"]), label
    close(own("p2g_vel"), want["p2g_vel"], VEL_REL, f"{label} p2g_vel")
    if method == tc.FLIP:
        close(own("old_vel"), want["old_vel"], VEL_REL, f"{label} flip_old_grid")
    close(own("grav_vel"), want["grav_vel"], VEL_REL, f"{label} grav_vel")


@pytest.mark.parametrize("run", P2G_RUNS, ids=transfer_id)
def test_p2g_sums_contributions_from_both_sides_of_a_slab_face(run):
    """hash(); p2g(); add_gravity() on every rank, the owned layers stitched against the oracle. A lone hat across a slab face is
    read from the rank that OWNS the face: exactly 0.0 where its only weight is 5e-7 or 2e-7, the particle's own w v / w at the bar
    of test_p2g_on_adversarial_clouds where it is 2e-6 or 5e-6 - the value that came over with the neighbour's plane."""
    name, bounds, method = run
    cloud = tc.build(name)
    size, parts, solid, meta = cloud
    hub, sims = make_ranks(cloud, bounds, METHOD_OF[method], tc.BLEND[method])
    results, _ = sf.run_ranks(sims, lambda r, s: p2g_on_rank(s, method), hub=hub)
    label = f"{transfer_id(run)}"
    check_stitched_p2g(results, tc.oracle_stages(name, method), bounds, size, method, label)
    assert all(res["deferred"] == (1 if res["n"] else 0) for res in results), [(res["n"], res["deferred"]) for res in results]
    nx, ny, nz = size
    for hat in sf.hats_across(name, bounds):
        x, y, z = hat["cell"]
        comp, p = hat["comp"], parts[hat["index"]]
        face = results[int(sf.owner(z, bounds))]["p2g_vel"][x + nx * (y + ny * z), comp]
        if not hat["kept"]:
            assert face == 0.0, (label, hat, face)
            continue
        own = p["vel"][comp]
        if method == tc.APIC:
            stag = np.full(3, 0.5)
            stag[comp] = 1.0
            own = own + p[("cx", "cy", "cz")[comp]] @ (np.array(meta["off"]) + (np.array(hat["cell"]) + stag) * meta["h"] - p["pos"])
        bar = VEL_REL * np.linalg.norm(p["vel"])
        print(f"MARGIN {label} lone_hat_across_{hat['target']:g} {abs(face - own) / bar:.3f}")
        assert abs(face - own) <= bar, (label, hat, face, own)


def test_the_global_atomic_scatter_is_refused_on_a_slab_handle():
    cloud = tc.build("lone_hats")
    hub, sims = make_ranks(cloud, (0, 1, 2), lfa.APIC, 1.0, p2g_variant=lfa.P2G_GLOBAL_ATOMIC)

    def fn(r, s):
        s.hash()
        s.p2g()

    _, errors = sf.run_ranks(sims, fn, hub=hub, raise_errors=False)
    assert [(r, e.code) for r, e in errors] == [(0, E_UNSUPPORTED), (1, E_UNSUPPORTED)], errors


DEFERRED_RUNS = [("tile_counts_deferred", (0, 1, 2)), ("contrast_21_13_18", (0, 1, 2, 3))]


@pytest.mark.parametrize("seq", ["hash,hash", "hash,correct,hash"])
@pytest.mark.parametrize("method", tc.ALL_METHODS, ids=tc.method_id)
@pytest.mark.parametrize("name,bounds", DEFERRED_RUNS, ids=[f"{n}-{sf.bounds_id(b)}" for n, b in DEFERRED_RUNS])
def test_p2g_on_slabs_with_a_deferred_binning(name, bounds, method, seq):
    """test_gpu_transfer_edges.py::test_p2g_with_a_deferred_binning on slabs: a second binning on top of a deferred one, and a
    binning after a position correction that has moved particles across the slab faces (the oracle is given the ranks' own
    downloaded particles, joined by id: cell + fp32 fraction, exact in fp64 at cell_size 1)."""
    cloud = tc.build(name)
    size, parts, solid, meta = cloud
    assert meta["h"] == 1.0
    hub, sims = make_ranks(cloud, bounds, METHOD_OF[method], tc.BLEND[method])

    def fn(r, s):
        s.hash()
        now = None
        if seq == "hash,correct,hash":
            s.correct_collide(1e-3)
            now = dict(parts=s.download_particles(), ids=s.particle_ids())  # (completes the first binning; the next one defers again)
        out = p2g_on_rank(s, method)  # (starts with its own hash)
        out["now"] = now
        after = s.download_particles()
        out["after"] = dict(parts=after, ids=s.particle_ids())
        return out

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    label = f"{name} {sf.bounds_id(bounds)} {seq} {tc.method_id(method)}"
    now = parts
    if seq == "hash,correct,hash":
        moved, _ = by_id([res["now"] for res in results], len(parts))
        assert not np.array_equal(moved["pos"], parts["pos"])
        now = parts.copy()
        now["pos"] = moved["pos"]
        now["old_pos"] = moved["pos"]
    # nothing was lost on the way: every particle still has its own v and C
    after, _ = by_id([res["after"] for res in results], len(parts))
    assert np.array_equal(after["vel"], f32(parts["vel"])) and np.array_equal(c_of(after), f32(c_of(parts))), label
    assert all(res["deferred"] == (1 if res["n"] else 0) for res in results)
    want = tc.staged_cloud((size, now, solid, meta), method) if seq == "hash,correct,hash" else tc.oracle_stages(name, method)
    check_stitched_p2g(results, want, bounds, size, method, label)


# (the G2P gathers, it does not care which way a hat points: of the reflected clouds the h = 1 one runs)
G2P_SKIP = ("tile_counts_deferred", "lone_hats_h17_zmirror", "lone_hats_h17_unscaled_zmirror", "lone_hats_above_z8_zmirror")
G2P_RUNS = [(n, bb[-1], m) for n, bb in sf.TRANSFERS if n not in G2P_SKIP for m in tc.build(n)[3]["methods"]]


@pytest.mark.parametrize("run", G2P_RUNS, ids=transfer_id)
def test_g2p_reads_the_neighbours_layer_through_the_refresh(run):
    """Each rank uploads the oracle's extrapolated grid with the velocities outside its own layers replaced by NaN: what a particle
    next to a slab face gathers from across it can only have come with lfa_g2p's refresh. v per id at g2p_bar, APIC's C at C_REL,
    PIC's and FLIP's C untouched, everything finite, the job's CFL figure (the minimum over the ranks: lfa_cfl is local) within 1e-4.
    FLIP blends with the old grid of the device's own P2G, whose ghost layer arrives in lfa_build_system - so FLIP runs that first."""
    name, bounds, method = run
    cloud = tc.build(name)
    size, parts, solid, meta = cloud
    want = tc.oracle_stages(name, method)
    label = f"{transfer_id(run)} g2p"
    grid = cells_from(want["extrap_vel"], want["extrap_type"])
    hub, sims = make_ranks(cloud, bounds, METHOD_OF[method], tc.BLEND[method])

    def fn(r, s):
        s.hash()
        out = {}
        if method == tc.FLIP:
            s.p2g()
            out["old_vel"] = s.old_cells()["vel"].copy()
            s.build_system(tc.DT)
        s.upload_cells(sf.poison_outside(grid, bounds, r, ("vel",), size))
        s.g2p()
        out["cfl"] = s.cfl()
        out["parts"], out["ids"] = s.download_particles(), s.particle_ids()
        return out

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    got, _ = by_id(results, len(parts))
    if method == tc.FLIP:
        close(sf.stitch([res["old_vel"] for res in results], bounds, size), want["old_vel"], VEL_REL, f"{label} flip_old_grid")
    assert np.isfinite(got["vel"]).all() and np.isfinite(c_of(got)).all(), label
    close(got["vel"], want["g2p_vel"], g2p_bar(method), f"{label} g2p_vel")
    if method == tc.APIC:
        close(c_of(got), want["g2p_c"], C_REL, f"{label} g2p_c")
    else:
        assert np.array_equal(c_of(got), f32(c_of(parts))), label
    cfl = min(res["cfl"] for res in results)
    assert np.isfinite(want["cfl"]) and abs(cfl - want["cfl"]) <= 1e-4 * want["cfl"], (label, cfl, want["cfl"])


# ====================================================================================================== grid stages
GRID_RUNS = sf.table("stencils")
GRID_IDS = [f"{n}-{sf.bounds_id(b)}" for n, b in GRID_RUNS]
DTYPES = [lfa.PCG_F32, lfa.PCG_F64]


def unknown_ranges(want, bounds, size):
    """[(first, end)] per rank: the rank's own unknowns are a contiguous run of the oracle's list (raw indices ascend with z)."""
    nx, ny, nz = size
    z = want["fluid_cells"].astype(np.int64) // (nx * ny)
    cuts = np.searchsorted(z, [sf.TILE * b for b in bounds])
    return list(zip(cuts[:-1], cuts[1:]))


def refreshed_ghost_cells(want, bounds, rank, size):
    """bool[ncells]: the cells of the two tile layers next to the rank's own whose tile lies within one tile of a particle tile - what
    the binning flags as processed on the neighbour and lists for the halo exchange."""
    nx, ny, nz = size
    nt = [-(-n // sf.TILE) for n in size]
    r = want["fluid_cells"].astype(np.int64)
    has = np.zeros((nt[2], nt[1], nt[0]), dtype=bool)
    has[(r // (nx * ny)) // 8, ((r // nx) % ny) // 8, (r % nx) // 8] = True
    pad = np.pad(has, 1)
    near = np.zeros_like(has)
    for dz, dy, dx in itertools.product(range(3), repeat=3):
        near |= pad[dz:dz + nt[2], dy:dy + nt[1], dx:dx + nt[0]]
    layers = [l for l in (bounds[rank] - 1, bounds[rank + 1]) if 0 <= l < nt[2]]
    keep = np.zeros_like(has)
    keep[layers] = near[layers]
    cells = np.repeat(np.repeat(np.repeat(keep, 8, axis=0), 8, axis=1), 8, axis=2)[:nz, :ny, :nx]
    return cells.reshape(-1)


def stencil_ranks(name, bounds, **extra):
    return make_ranks(sc.build(name), bounds, lfa.APIC, 1.0, **extra)


OWN_RUNS = [(n, b) for n, b in GRID_RUNS if n == "maze" or b == dict(sf.STENCILS)[n][0] and n != "sheets" or (n, b) == ("sheets", (0, 1, 2, 3))]


@pytest.mark.parametrize("name,bounds", OWN_RUNS, ids=[f"{n}-{sf.bounds_id(b)}" for n, b in OWN_RUNS])
def test_unknowns_types_and_matrix_bits_from_the_ranks_own_binning(name, bounds):
    """The device's own binning and P2G on every rank, nothing uploaded: the ranks' fluid-cell lists, concatenated, are the
    oracle's list (same order: raw indices ascend with z), counts and types of the owned layers and the A bits of the owned unknowns
    are exact - a bit towards the cell across the face depends on the neighbour's types and counts."""
    size = sc.build(name)[0]
    want = sc.oracle_stages(name, True)
    hub, sims = stencil_ranks(name, bounds)

    def fn(r, s):
        s.hash()
        out = dict(fluid_cells=s.fluid_cells(), counts=s.cell_counts())
        s.p2g()
        s.add_gravity(sc.DT)
        out["type"] = s.cells()["type"].copy()
        s.build_system(sc.DT)
        out["abits"] = s.abits()
        return out

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    assert np.array_equal(np.concatenate([res["fluid_cells"] for res in results]), want["fluid_cells"])
    assert np.array_equal(sf.stitch([res["counts"] for res in results], bounds, size), want["counts"])
    assert np.array_equal(sf.stitch([res["type"] for res in results], bounds, size), want["p2g_type"])
    got = np.concatenate([res["abits"] for res in results])
    assert np.array_equal(got, want["abits"]), np.flatnonzero(got != want["abits"])[:10]


@pytest.mark.parametrize("name,bounds", GRID_RUNS, ids=GRID_IDS)
def test_system_from_a_grid_poisoned_outside_the_ranks_layers(name, bounds):
    """Each rank uploads the oracle's grid after gravity with velocities AND types destroyed outside its own layers;
    lfa_build_system's refresh must bring types, counts and u, v, w of the neighbour's adjacent tile layer: those cells are read
    back and compared exactly, A bits exact, b at 1e-6 and the matrix probe at 1e-6 (fp32 vectors) / 1e-13 (fp64) of their maxima -
    each rank on its own unknowns, the probe's slice across the face arriving in lfa_apply_a's exchange."""
    size = sc.build(name)[0]
    want = sc.oracle_stages(name, True)
    grid = cells_from(want["grav_vel"], want["type"])
    ranges = unknown_ranges(want, bounds, size)
    probe = sc.probe(len(want["b"]))
    for dtype in DTYPES:
        hub, sims = stencil_ranks(name, bounds, precond=lfa.PRECOND_MIC0_TILED, pcg_dtype=dtype)

        def fn(r, s):
            s.hash()
            s.upload_cells(sf.poison_outside(grid, bounds, r, ("vel", "type"), size))
            s.build_system(sc.DT)
            a, e = ranges[r]
            return dict(cells=s.cells(), counts=s.cell_counts(), abits=s.abits(), b=s.b(), Aprobe=s.apply_a(probe[a:e]))

        results, _ = sf.run_ranks(sims, fn, hub=hub)
        label = f"{name} {sf.bounds_id(bounds)} {DTYPE_ID[dtype]}"
        for r, res in enumerate(results):
            m = refreshed_ghost_cells(want, bounds, r, size)
            assert m.any()
            assert np.array_equal(res["cells"]["type"][m], want["type"][m]), f"{label}: types of rank {r}'s ghost layers"
            assert np.array_equal(res["counts"][m], want["counts"][m]), f"{label}: counts of rank {r}'s ghost layers"
            assert np.array_equal(res["cells"]["vel"][m], want["grav_vel"][m]), f"{label}: velocities of rank {r}'s ghost layers"
            assert [len(res["b"]), len(res["abits"])] == [ranges[r][1] - ranges[r][0]] * 2
        assert np.array_equal(np.concatenate([res["abits"] for res in results]), want["abits"])
        close(np.concatenate([res["b"] for res in results]), want["b"], 1e-6, f"{label} b")
        close(np.concatenate([res["Aprobe"] for res in results]), want["Aprobe"], 1e-6 if dtype == lfa.PCG_F32 else 1e-13, f"{label} A_probe")


# the solve: three preconditioners on five (case, bounds) with the vector type alternating, both types on maze [0, 1, 2, 3]
SOLVE_PAIRS = [("maze", (0, 1, 2, 3)), ("maze_h17", (0, 1, 2, 3)), ("sheets", (0, 2, 3)), ("droplets", (0, 1, 2)), ("walls_z", (0, 1, 2, 5))]
SOLVE_RUNS = [(n, b, p, DTYPES[(i + j) % 2], None) for i, (n, b) in enumerate(SOLVE_PAIRS) for j, p in enumerate(PRECONDS)]
SOLVE_RUNS += [("maze", (0, 1, 2, 3), p, DTYPES[(j + 1) % 2], None) for j, p in enumerate(PRECONDS)]
SOLVE_RUNS += [(n, b, lfa.PRECOND_MULTIGRID, d, "1") for n, b in (("maze", (0, 1, 2, 3)), ("droplets", (0, 1, 2))) for d in DTYPES]


def solve_id(run):
    name, bounds, precond, dtype, levels = run
    return f"{name}-{sf.bounds_id(bounds)}-{PRECOND_ID[precond]}-{DTYPE_ID[dtype]}" + ("-one_dist_level" if levels else "")


@pytest.mark.parametrize("run", SOLVE_RUNS, ids=solve_id)
def test_every_preconditioner_solves_the_system_on_slabs(run, monkeypatch):
    """The answer, not the rate (max_iterations 1000, the count printed): from the oracle's grid, poisoned outside each rank's layers,
    the ranks' pressures, concatenated, against the oracle's at P_REL; every rank reports the same iteration count.
    one_dist_level: LFA_MG_DIST_LEVELS=1, the finest multigrid level alone distributed."""
    name, bounds, precond, dtype, levels = run
    if levels:
        monkeypatch.setenv("LFA_MG_DIST_LEVELS", levels)
    else:
        monkeypatch.delenv("LFA_MG_DIST_LEVELS", raising=False)
    size = sc.build(name)[0]
    want = sc.oracle_stages(name, True)
    grid = cells_from(want["grav_vel"], want["type"])
    hub, sims = stencil_ranks(name, bounds, precond=precond, pcg_dtype=dtype, max_iterations=1000)

    def fn(r, s):
        s.hash()
        s.upload_cells(sf.poison_outside(grid, bounds, r, ("vel", "type"), size))
        return s.solve(sc.DT)

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    its = [int(res[2]) for res in results]
    print(f"ITERS {solve_id(run)} {its} (oracle {int(want['iters'])})")
    assert len(set(its)) == 1, its
    assert all(res[3] == 0 and res[1] < 1e-6 for res in results), [(res[1], res[3]) for res in results]
    close(np.concatenate([res[0] for res in results]), want["p"], P_REL, f"{solve_id(run)} p")


@pytest.mark.parametrize("name,bounds", GRID_RUNS, ids=GRID_IDS)
def test_apply_pressure_face_by_face_on_slabs(name, bounds):
    """k_apply_pressure with each rank holding the oracle's pressure of its OWN unknowns: the +z faces under a slab face take their
    second pressure from the slice the rank above sends. The owned layers, stitched, face by face as in
    test_gpu_stencil_edges.py::test_apply_pressure_face_by_face: untouched faces bit-identical, zeroed faces exactly 0, every
    computed face within K_APPLY roundings, class by class. The vector type alternates over the table."""
    size, parts, solid, meta = sc.build(name)
    want = sc.oracle_stages(name, True)
    grid = cells_from(want["grav_vel"], want["type"])
    ranges = unknown_ranges(want, bounds, size)
    dtype = DTYPES[GRID_RUNS.index((name, bounds)) % 2]
    label = f"{name} {sf.bounds_id(bounds)} {DTYPE_ID[dtype]} apply"
    hub, sims = stencil_ranks(name, bounds, pcg_dtype=dtype)

    def fn(r, s):
        s.hash()
        s.upload_cells(sf.poison_outside(grid, bounds, r, ("vel", "type"), size))
        s.build_system(sc.DT)
        a, e = ranges[r]
        s.upload_pressure(want["p"][a:e])
        s.apply_pressure(sc.DT)
        return s.cells()["vel"].copy()

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    got = sf.stitch(results, bounds, size)
    vin, vout = want["grav_vel"], want["apply_exact"]
    ref, cls, scale = sc.apply_pressure_faces(size, want["type"], want["fluid_cells"], vin, want["p"], sc.coeff_of(meta))
    assert np.array_equal(ref, vout)
    close(got, vout, VEL_REL, f"{label} max_norm")
    same = vout == vin
    zero = (vout == 0.0) & ~same
    rest = ~same & ~zero
    assert np.array_equal(got[same], vin[same]), f"{label}: {int((got[same] != vin[same]).sum())} faces changed that the oracle leaves alone"
    assert not got[zero].any(), f"{label}: {int((got[zero] != 0).sum())} faces not exactly 0"
    assert not cls["computed-twice"].any()
    bar = np.where(cls["computed-twice"], K_APPLY_TWICE, K_APPLY) * EPS * scale
    for k in sc.FACE_CLASSES:
        m = cls[k] & rest
        if m.any():
            pointwise(got[m], vout[m], bar[m], f"{label} {k}")
    # the faces the slab exchange is for: +z faces of the last cell layer under a slab face that read the pressure above it
    nx, ny, nz = size
    under = np.isin(np.arange(nx * ny * nz) // (nx * ny) + 1, sf.faces(bounds))
    m = rest[:, 2] & under & (cls["unknown-fluid"][:, 2] | cls["air-unknown"][:, 2])
    assert m.any() == (sf.stencil_counts(name, bounds)["apply_faces_second_pressure_across"] > 0)
    if m.any():
        pointwise(got[m, 2], vout[m, 2], bar[m, 2], f"{label} faces_with_the_second_pressure_across")


EXTRAP_PAIRS = [("maze", (0, 1, 2, 3)), ("sheets", (0, 1, 2, 3)), ("sheets", (0, 2, 3)), ("droplets", (0, 1, 2)), ("walls_z", (0, 1, 2, 5)),
                ("thin_2_9_17", (0, 1, 2, 3))]


@pytest.mark.parametrize("sweeps", [1, 2, 3])
@pytest.mark.parametrize("name,bounds", EXTRAP_PAIRS, ids=[f"{n}-{sf.bounds_id(b)}" for n, b in EXTRAP_PAIRS])
def test_extrapolation_sweeps_across_slab_faces(name, bounds, sweeps):
    """k_extrapolate with 1, 2 and 3 sweeps from the oracle's projected grid, its velocities NaN outside each rank's layers: what a
    sweep averages from across the face came with lfa_extrapolate's refresh, what the next sweep finds valid there with the
    validity bytes sent between two sweeps. Component by component as on one domain: untouched components bit-identical, written
    ones within K_EXTRAP roundings per sweep. (Counts and types of the ghost layers arrive in lfa_build_system, which runs first on
    the same grid; the poisoned upload follows it.)"""
    size = sc.build(name)[0]
    want = sc.oracle_stages(name, True)
    label = f"{name} {sf.bounds_id(bounds)} extrapolate_{sweeps}"
    grid = cells_from(want["apply_vel"], want["type"])
    hub, sims = stencil_ranks(name, bounds, velocity_extrapolation_iterations=sweeps)

    def fn(r, s):
        s.hash()
        s.upload_cells(grid)
        s.build_system(sc.DT)
        s.upload_cells(sf.poison_outside(grid, bounds, r, ("vel",), size))
        s.extrapolate()
        return s.cells()["vel"].copy()

    results, _ = sf.run_ranks(sims, fn, hub=hub)
    got = sf.stitch(results, bounds, size)
    vin, vout = want["apply_vel"], sf.oracle_extrapolation(name, sweeps)
    ref, written, count, born, unit = sc.extrapolate_sweeps(size, want["type"], want["fluid_cells"], vin, sweeps)
    assert np.array_equal(ref, vout)
    assert np.isfinite(got).all(), f"{label}: {int((~np.isfinite(got)).sum())} components are not finite"
    close(got, vout, VEL_REL, f"{label} max_norm")
    assert np.array_equal(got[~written], vin[~written]), f"{label}: {int((got[~written] != vin[~written]).sum())} components changed that the oracle leaves alone"
    if written.any():
        pointwise(got[written], vout[written], K_EXTRAP * EPS * unit[written], f"{label} written_components")
