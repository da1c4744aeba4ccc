"""CPU: the inputs of tests/tracer_slab_cases.py contain what they are designed to contain, shown from the oracle alone, and the
built library exports the collective tracer entry points (tests/test_gpu_tracer_slabs.py runs them)."""
import numpy as np
import pytest

import libfluid_amd as lfa
from tests import tracer_cases as tc
from tests import tracer_slab_cases as ts

NEW_SYMBOLS = ("lfa_tracers_add_collective", "lfa_tracers_advect_collide_collective", "lfa_tracers_transfer_collective",
               "lfa_tracers_step_collective", "lfa_tracers_download_ids")


def test_the_library_exports_the_collective_tracer_calls():
    lib = lfa.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in lfa.SIGNATURES, name
    for method in ("add_tracers_collective", "tracers_advect_collide_collective", "tracers_transfer_collective", "tracers_step_collective",
                   "tracers_with_ids"):
        assert callable(getattr(lfa.Sim, method))


def test_scenes_are_what_the_issue_names():
    assert ts.A.size == (40, 24, 17) and ts.A.bounds == ([0, 1, 3], [0, 2, 3], [0, 1, 2, 3]) and ts.A.faces == (8, 16)
    assert ts.B.size == (16, 16, 33) and ts.B.bounds == ([0, 1, 2, 3, 4, 5], [0, 2, 3, 5], [0, 1, 5]) and ts.B.faces == (8, 16, 24, 32)
    for scene in (ts.A, ts.B):
        assert -(-scene.size[2] // 8) == scene.bounds[0][-1] and scene.size[2] % 8 == 1  # the last tile layer: ONE cell layer
        assert all((scene.h * k) != round(scene.h * k, 0) for k in (1, 2, 4)) and scene.off[2] * 8 != round(scene.off[2] * 8)
    z = ts.B.solid[:, 2]
    assert z.min() == 15 and z.max() == 16  # the slab straddles the face z = 16
    assert np.array_equal(ts.A.mask(), tc.solid_mask())


@pytest.mark.parametrize("run", list(ts.RUNS))
def test_owner_partitions_all_tracers(run):
    scene, pos, vel = ts.tracers(run)
    for when in (pos, ts.moved(run)):
        for bounds in scene.bounds:
            own = ts.owner(scene, when, bounds)
            assert own.min() >= 0 and own.max() <= len(bounds) - 2
            assert sum(int((own == r).sum()) for r in range(len(bounds) - 1)) == len(pos)


def test_the_owner_of_a_far_or_outside_position_is_the_clamped_cell_s():
    at, n = ts.groups("A")["far"]
    own = ts.owner(ts.A, ts.tracers("A")[1][at:at + n], [0, 1, 2, 3])
    assert own.tolist() == [0, 2, 0, 2]
    for name, want in (("outside_z_lo", [0] * 4), ("outside_z_hi", [2] * 4), ("outside_x", [0, 1, 2, 0])):
        at, n = ts.groups("A")[name]
        assert ts.owner(ts.A, ts.tracers("A")[1][at:at + n], [0, 1, 2, 3]).tolist() == want, name


def crossing(scene, run, face):
    """(up bool[n], down bool[n]): the oracle's move takes the tracer across the cell layer `face`."""
    a, b = ts.cell_layer(scene, ts.tracers(run)[1]), ts.cell_layer(scene, ts.moved(run))
    return (a < face) & (b >= face), (a >= face) & (b < face)


def test_every_face_has_its_movers_in_both_directions():
    for run, scene in (("A", ts.A), ("B", ts.B)):
        for face in scene.faces:
            up, down = crossing(scene, run, face)
            print(run, "face", face, "up", int(up.sum()), "down", int(down.sum()))
            assert up.sum() >= 65 and down.sum() >= 65, (run, face)
    # scene A: every group of every size crosses its face whole, in its direction
    a, b = ts.cell_layer(ts.A, ts.tracers("A")[1]), ts.cell_layer(ts.A, ts.moved("A"))
    for face in ts.A.faces:
        for n in ts.GROUP_SIZES:
            r = ts.rows("A", f"face{face}_up_{n}")
            assert r.stop - r.start == n and (a[r] < face).all() and (b[r] >= face).all() and (b[r] < face + 8).all(), (face, n)
            r = ts.rows("A", f"face{face}_down_{n}")
            assert r.stop - r.start == n and (a[r] >= face).all() and (b[r] < face).all() and (b[r] >= face - 8).all(), (face, n)


def hops(scene, run, bounds):
    return ts.owner(scene, ts.moved(run), bounds) - ts.owner(scene, ts.tracers(run)[1], bounds)


def test_hop_distances():
    h = hops(ts.A, "A", [0, 1, 2, 3])
    assert (h[ts.rows("A", "hop2_up")] == 2).all() and (h[ts.rows("A", "hop2_down")] == -2).all()
    h = hops(ts.B, "B", [0, 1, 2, 3, 4, 5])
    for k in (1, 2, 3, 4):
        assert (h[ts.rows("B", f"hop{k}_up")] == k).all() and (h[ts.rows("B", f"hop{k}_down")] == -k).all(), k
    assert (h[ts.rows("B", "stay")] == 0).all()
    assert set(np.unique(h).tolist()) == set(range(-4, 5))  # every distance in one step, stayers included
    for run, table in ts.ROUNDS.items():
        scene, pos, _ = ts.tracers(run)
        assert set(table) == {tuple(b) for b in scene.bounds}
        for bounds, want in table.items():
            assert ts.rounds_model(scene, pos, ts.moved(run), list(bounds)) == want, (run, bounds)


def test_lattice_tracers_end_on_the_face_and_the_division_decides():
    scene, pos, vel = ts.tracers("A")
    end = ts.moved("A")
    for face in ts.A.faces:
        r = ts.rows("A", f"lattice{face}")
        zs = ts.face_lattice(ts.A, face)
        assert np.isin(end[r, 2], zs).all()  # the oracle's move ends on the lattice point, to the bit
        assert (vel[r, 2] != 0.0).sum() >= 4
        cz = ts.cell_layer(ts.A, end[r])
        print("face", face, "cells", np.unique(cz).tolist())
        assert set(np.unique(cz).tolist()) == {face - 1, face}
        # built for cell `face`, owned by the rank of cell face - 1: on a decomposition with a rank face there the owners differ
        bounds = [0, 1, 2, 3]
        nominal = np.searchsorted(bounds, face >> 3, side="right") - 1
        assert (ts.owner(ts.A, end[r], bounds) != nominal).any() and (ts.owner(ts.A, end[r], bounds) == nominal).any()


def test_bounce_groups_stay_on_the_side_they_came_from():
    scene, pos, vel = ts.tracers("B")
    end = ts.moved("B")
    free = pos + vel * ts.DT  # the move without the obstacle
    for name, near, far in (("bounce_up", 1, 2), ("bounce_down", 2, 1)):
        r = ts.rows("B", name)
        assert ((ts.cell_layer(ts.B, pos[r]) >> 3) == near).all() and ((ts.cell_layer(ts.B, free[r]) >> 3) == far).all(), name
        assert ((ts.cell_layer(ts.B, end[r]) >> 3) == near).all(), name
        assert tc.march_model(ts.B.size, ts.B.mask(), ts.B.h, ts.B.off, pos[r], vel[r], ts.DT)[1].all(), name


def test_stopped_at_the_z_walls_and_frozen_tracers_are_present():
    scene, pos, vel = ts.tracers("A")
    # the walls stop a tracer through the clamp of the move: it ends a skin's width inside the box, whatever its velocity asked for
    end, skin = ts.moved("A"), tc.SKIN
    lo, hi = ts.A.off[2] + skin, ts.A.h * ts.A.size[2] + ts.A.off[2] - skin
    assert (np.abs(end[ts.rows("A", "wall_lo"), 2] - lo) < 1e-9).all() and (np.abs(end[ts.rows("A", "wall_hi"), 2] - hi) < 1e-9).all()
    assert (ts.cell_layer(ts.A, end[ts.rows("A", "wall_lo")]) == 0).all() and (ts.cell_layer(ts.A, end[ts.rows("A", "wall_hi")]) == 16).all()
    assert (ts.cell_layer(ts.A, pos[ts.rows("A", "wall_hi")]) < 16).all()  # ... across the face z = 16 on its way
    # a march meets the wall itself only from outside: the tracers added beyond the box in z
    outside = np.r_[ts.rows("A", "outside_z_lo"), ts.rows("A", "outside_z_hi")]
    assert tc.march_model(ts.A.size, ts.A.mask(), ts.A.h, ts.A.off, pos[outside], vel[outside], ts.DT)[1].all()
    frozen = ts.frozen_rows(pos, vel)
    r = ts.rows("A", "frozen")
    assert frozen[r].all() and frozen.sum() == r.stop - r.start == 8
    assert np.array_equal(ts.moved("A")[r], pos[r])
    cz = ts.cell_layer(ts.A, pos[r])
    assert set(cz.tolist()) == {7, 8, 15, 16}  # next to both faces, on both sides


@pytest.mark.parametrize("run", list(ts.RUNS))
def test_march_model_is_the_oracle_on_these_inputs(run):
    """Pins the expected `stopped` counts: the counting restatement ends where the oracle ends, bit for bit. Not asked: the four rows
    at +-1e300 (ts.stopped says why); the oracle clamps them into the box, which the first assertion holds it to."""
    scene, pos, vel = ts.tracers(run)
    moves = ~ts.frozen_rows(pos, vel)
    if "far" in ts.groups(run):
        far = ts.rows(run, "far")
        lo, hi = scene.off[2] + tc.SKIN, scene.h * scene.size[2] + scene.off[2] - tc.SKIN
        assert np.isin(ts.moved(run)[far, 2], [lo, hi]).all() and ts.stopped(run)[far].all()
        moves[far] = False
    end, stopped = tc.march_model(scene.size, scene.mask(), scene.h, scene.off, pos[moves], vel[moves], ts.DT)
    want = ts.moved(run)[moves]
    bad = np.flatnonzero((end != want).any(axis=1))
    print(run, "tracers", int(moves.sum()), "stopped", int(stopped.sum()), "rows that differ", bad[:8], end[bad[:4]], want[bad[:4]])
    assert end.tobytes() == want.tobytes()
    assert stopped.sum() > 0 or run in ("A_stay", "grow")


def test_grow_run_ranks_are_as_designed():
    scene, pos, vel = ts.tracers("grow")
    end = ts.moved("grow")
    assert len(pos) == 1501
    for bounds in scene.bounds:
        nr = len(bounds) - 1
        before = np.bincount(ts.owner(scene, pos, bounds), minlength=nr)
        after = np.bincount(ts.owner(scene, end, bounds), minlength=nr)
        want = ts.GROW_RANKS[tuple(bounds)]
        assert [r for r in range(nr) if before[r] == 0] == want["empty"], bounds
        assert [r for r in range(nr) if before[r] > 0 and after[r] == 0] == want["emptied"], bounds
        assert [r for r in range(nr) if before[r] == 1 and after[r] == 1501] == want["growing"], bounds
        assert 1501 > 1024


def test_migrate_model_places_stayers_then_below_then_above():
    dest = {0: 1, 1: 0, 2: 1, 3: 2, 4: 1, 5: 0, 6: 2}
    lists, down, up, got = ts.migrate_model([[0, 1], [2, 3, 5], [4, 6]], dest, 1)
    assert lists == [[1, 5], [2, 0, 4], [6, 3]] and down == [0, 1, 1] and up == [1, 1, 0] and got == [1, 2, 1]
    lists, down, up, got = ts.migrate_model([[9], [], []], {9: 2}, 2)  # forwarded through the middle rank
    assert lists == [[], [], [9]] and up == [1, 1, 0] and got == [0, 1, 1]
