"""Tracers on virtual slabs (N handles on one GPU, in-process transport, one host thread per rank for every collective, as in
tests/test_gpu_seed_slabs.py) against tests/tracer_slab_cases.py: gathered by id, the ranks' tracers are the single domain's - the
oracle's move, and the oracle's PIC transfer on the ranks' grids stitched by owned z-range - byte for byte; every tracer lives on
the rank that owns its cell layer; the placement is the model's, stayers, then from below, then from above. Tolerance 0 throughout.
The 16 tracers of scene A that START outside the grid are held to a single-domain handle's plain call instead of the oracle
(reference_move; tests/tracer_slab_cases.py: starts_outside says why), every other tracer to the oracle. Comparisons between calls
("the collective call equals the plain one", "the one call equals the two stage calls") are made on one set of handles and one
grid: two fluids stepped side by side do not stay equal to the bit.
tests/test_tracer_slab_cases.py shows on the CPU that the inputs contain what they are designed to contain."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import sample_cases as sc
from tests import sample_slab_cases as ss
from tests import tracer_slab_cases as ts
from tests.test_gpu_seed_slabs import close_all, collective, make_slabs

pytestmark = pytest.mark.gpu

KW = dict(gravity=sc.GRAVITY, method=lfa.PIC)
E_INVALID, E_UNSUPPORTED = -1, -6
CASES = [(run, tuple(b)) for run in ("A", "A_stay", "B") for b in ts.RUNS[run][0].bounds]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def slabs(scene, bounds):
    hub, sims = make_slabs(scene.grid(), list(bounds), **KW)
    for s in sims:
        s.set_solid_cells(scene.solid)
    return hub, sims


def add(sims, pos, vel):
    """The same list on every rank, one rank after the other on this thread: the call sends no message, so none waits."""
    return [s.add_tracers_collective(pos, vel) for s in sims]


def by_id(per_rank, n):
    """The ranks' (ids, pos, vel[, types]) gathered and ordered by id; asserts that every id 0 .. n - 1 is there once."""
    ids = np.concatenate([p[0] for p in per_rank])
    assert ids.dtype == np.uint32 and np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32)), "the union is not every id once"
    order = np.argsort(ids, kind="stable")
    return [np.concatenate([p[k] for p in per_rank])[order] for k in range(1, len(per_rank[0]))]


def reference_move(scene, pos, vel, oracle=None):
    """The positions one move must give: the oracle's (`oracle`: computed already) for every tracer that starts inside the grid;
    for one that starts outside - ts.starts_outside says why the reference has no answer there - the plain lfa_tracers_advect_collide
    of a single-domain handle, the other side of the contract."""
    want = np.array(ts.expected_move(scene, pos, vel) if oracle is None else oracle)
    out = ts.starts_outside(scene, pos) & ~ts.frozen_rows(pos, vel)
    if out.any():
        one = lfa.Sim(**scene.grid(), **KW)
        one.set_solid_cells(scene.solid)
        one.add_tracers(pos[out], vel[out])
        one.tracers_advect_collide(ts.DT)
        want[out] = one.tracers()[0]
        one.close()
    return want


# ---------------------------------------------------------------------------------------------------- 1. add
@pytest.mark.parametrize("run,bounds", [c for c in CASES if c[0] != "A_stay"], ids=str)
def test_add_keeps_the_owned_tracers_in_list_order(run, bounds):
    scene, pos, vel = ts.tracers(run)
    hub, sims = slabs(scene, bounds)
    cut = 1001
    own = ts.owner(scene, pos, bounds)
    first = add(sims, pos[:cut], vel[:cut])
    second = add(sims, pos[cut:], None)  # (no velocities: zeros)
    got = [s.tracers_with_ids(types=True) for s in sims]
    counts = [s.num_tracers() for s in sims]
    close_all(hub, sims)
    want_vel = np.concatenate([vel[:cut], np.zeros_like(vel[cut:])])
    for r, (ids, p, v, t) in enumerate(got):
        mine = np.flatnonzero(own == r)
        print(run, bounds, "rank", r, "keeps", len(mine), "of", len(pos))
        assert first[r] == (int((own[:cut] == r).sum()), 0) and second[r] == (int((own[cut:] == r).sum()), cut), (r, first[r], second[r])
        assert counts[r] == len(mine)
        assert np.array_equal(ids, mine.astype(np.uint32)), r  # list order, id = first_id + index in the list
        assert p.tobytes() == pos[mine].tobytes() and v.tobytes() == want_vel[mine].tobytes() and not t.any(), r
    by_id(got, len(pos))


# ---------------------------------------------------------------------------------------------------- 2. move
def run_move(run, bounds):
    scene, pos, vel = ts.tracers(run)
    hub, sims = slabs(scene, bounds)
    add(sims, pos, vel)
    counts = collective(sims, lambda r, s: s.tracers_advect_collide_collective(ts.DT))
    got = [s.tracers_with_ids(types=True) for s in sims]
    close_all(hub, sims)
    return counts, got


@pytest.mark.parametrize("run,bounds", CASES, ids=str)
def test_move_then_every_tracer_is_with_its_owner(run, bounds):
    scene, pos, vel = ts.tracers(run)
    want = reference_move(scene, pos, vel, oracle=ts.moved(run))
    n, nr = len(pos), len(bounds) - 1
    counts, got = run_move(run, bounds)
    before, after = ts.owner(scene, pos, bounds), ts.owner(scene, want, bounds)
    rounds = ts.ROUNDS[run][bounds]
    lists, down, up, received = ts.migrate_model([np.flatnonzero(before == r).tolist() for r in range(nr)], after, rounds)
    for r in range(nr):
        print(run, bounds, "rank", r, "counts", counts[r], "model: down", down[r], "up", up[r], "received", received[r], "holds", len(lists[r]))
    got_pos, got_vel, got_types = by_id(got, n)
    bad = np.flatnonzero((got_pos != want).any(axis=1))
    assert got_pos.tobytes() == want.tobytes(), (bad[:8], got_pos[bad[:4]], want[bad[:4]])
    assert got_vel.tobytes() == vel.tobytes() and not got_types.any()
    for r, (ids, p, v, t) in enumerate(got):
        assert set(ids.tolist()) == set(np.flatnonzero(after == r).tolist()), r       # residence is owner(new position)
        assert ids.tolist() == lists[r], r                                               # stayers, then from below, then from above
        assert counts[r][2:] == (down[r], up[r], received[r], rounds), (r, counts[r])
    assert rounds == ts.rounds_model(scene, pos, want, bounds)
    assert sum(c[0] for c in counts) == int(ts.stopped(run).sum()) and sum(c[1] for c in counts) == int(ts.frozen_rows(pos, vel).sum())
    assert sum(c[2] + c[3] for c in counts) == sum(c[4] for c in counts) == int(np.abs(after - before).sum())
    # a second job, from fresh handles: the same bytes in the same order on every rank
    counts2, again = run_move(run, bounds)
    assert counts2 == counts
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------- 3. transfer and steps
def fluid_slabs(bounds):
    """States (b) of tests/test_gpu_sample_slabs.py: ss.slab_particles() after hash + P2G + gravity."""
    hub, sims = slabs(ts.A, bounds)
    for s in sims:
        s.upload_particles(ss.slab_particles())

    def p2g(r, s):
        s.hash()
        s.p2g()
        s.add_gravity(sc.DT)

    collective(sims, p2g)
    return hub, sims


def grid_of(sims, bounds):
    return ss.stitch([s.cells() for s in sims], list(bounds))


def restart(sims, pos, vel):
    """The job's tracers replaced by the rows (pos, vel), id = row: clear on EVERY rank - it resets first_id -, then the add."""
    for s in sims:
        s.clear_tracers()
    assert all(first == 0 for _, first in add(sims, pos, vel))


@pytest.mark.parametrize("bounds", [tuple(b) for b in ts.A.bounds], ids=str)
def test_transfer_and_three_steps_are_the_single_domain_s(bounds):
    scene, pos0, vel0 = ts.tracers("A")
    n, nr = len(pos0), len(bounds) - 1
    hub, sims = fluid_slabs(bounds)
    # (b): the transfer alone, at the positions as added - outside points get +0.0 and type 0
    add(sims, pos0, vel0)
    collective(sims, lambda r, s: s.tracers_transfer_collective())
    pos, vel, types = by_id([s.tracers_with_ids(types=True) for s in sims], n)
    want_vel, want_types, n_out = sc.model(grid_of(sims, bounds), pos0)
    assert pos.tobytes() == pos0.tobytes() and vel.tobytes() == want_vel.tobytes() and types.tobytes() == want_types.tobytes()
    assert n_out == 16  # the four groups added outside the grid
    restart(sims, pos0, vel0)  # the caller's velocities again
    for step in range(3):
        collective(sims, lambda r, s: s.time_step(sc.DT))
        pos, vel = by_id([s.tracers_with_ids() for s in sims], n)
        counts = collective(sims, lambda r, s: s.tracers_step_collective(sc.DT))
        got = [s.tracers_with_ids(types=True) for s in sims]
        got_pos, got_vel, got_types = by_id(got, n)
        grid = grid_of(sims, bounds)
        want_pos = reference_move(ts.A, pos, vel)
        want_vel, want_types, _ = sc.model(grid, want_pos)
        bad = np.flatnonzero((got_vel.view(np.uint64) != want_vel.view(np.uint64)).any(axis=1))
        print(bounds, "step", step, "counts", counts, "rows whose velocity differs", len(bad))
        assert got_pos.tobytes() == want_pos.tobytes(), step
        assert got_vel.tobytes() == want_vel.tobytes(), (step, bad[:8], got_vel[bad[:4]], want_vel[bad[:4]])
        assert got_types.tobytes() == want_types.tobytes(), step
        own = ts.owner(ts.A, want_pos, bounds)
        for r, (ids, p, v, t) in enumerate(got):
            assert set(ids.tolist()) == set(np.flatnonzero(own == r).tolist()), (step, r)
        # on every face a tracer reads the ghost layer from either side
        below, above = ss.reads_ghost(want_pos, list(bounds))
        for r in range(nr):
            assert r == 0 or (below & (own == r)).any(), (step, r)
            assert r == nr - 1 or (above & (own == r)).any(), (step, r)
        if step == 0:
            assert counts[0][5] == ts.ROUNDS["A"][bounds] and sum(c[1] for c in counts) == 8
        # the twin job, on the same handles and the same grid (two fluids stepped apart need not agree to the bit): from the state
        # before the step once more with the one call, once with the two stage calls - the same bytes in the same order
        restart(sims, pos, vel)
        counts_one = collective(sims, lambda r, s: s.tracers_step_collective(sc.DT))
        one = [s.tracers_with_ids(types=True) for s in sims]
        restart(sims, pos, vel)
        counts_two = collective(sims, lambda r, s: s.tracers_advect_collide_collective(sc.DT))
        collective(sims, lambda r, s: s.tracers_transfer_collective())
        two = [s.tracers_with_ids(types=True) for s in sims]
        assert counts_one == counts_two and [c[5] for c in counts_one] == [c[5] for c in counts]
        for a, b in zip(one, two):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), step
        for x, y in zip(by_id(two, n), (got_pos, got_vel, got_types)):
            assert x.tobytes() == y.tobytes(), step
        assert grid_of(sims, bounds).tobytes() == grid.tobytes()  # the tracer step writes ghost layers only
    close_all(hub, sims)


# ---------------------------------------------------------------------------------------------------- 4. single domain
def test_on_a_single_domain_the_collective_calls_are_the_plain_ones():
    """One handle, so one fluid: the tracer calls never write it (tests/test_gpu_tracers.py), and every variant starts from the same
    tracers after the same time steps."""
    scene, pos, vel = ts.tracers("A")
    n = len(pos)
    sim = lfa.Sim(**ts.A.grid(), **KW)
    sim.set_solid_cells(ts.A.solid)
    sim.upload_particles(ss.slab_particles())
    for step in range(2):
        sim.time_step(sc.DT)
        sim.clear_tracers()
        sim.add_tracers(pos[:1001], vel[:1001])
        sim.add_tracers(pos[1001:], vel[1001:])
        stopped, frozen = sim.tracers_step(sc.DT)
        want = sim.tracers(types=True)
        for staged in (False, True):
            sim.clear_tracers()
            assert sim.add_tracers_collective(pos[:1001], vel[:1001]) == (1001, 0)
            assert sim.add_tracers_collective(pos[1001:], vel[1001:]) == (n - 1001, 1001)
            if staged:
                assert sim.tracers_advect_collide_collective(sc.DT) == (stopped, frozen, 0, 0, 0, 0)
                sim.tracers_transfer_collective()
            else:
                assert sim.tracers_step_collective(sc.DT) == (stopped, frozen, 0, 0, 0, 0)
            ids, p, v, t = sim.tracers_with_ids(types=True)
            assert np.array_equal(ids, np.arange(n, dtype=np.uint32))
            assert p.tobytes() == want[0].tobytes() and v.tobytes() == want[1].tobytes() and t.tobytes() == want[2].tobytes(), (step, staged)
        assert frozen == (8 if step == 0 else 0)  # (the NaN velocities are gone after the first transfer)
        pos, vel = want[0], want[1]
    sim.close()


def test_the_plain_calls_refuse_a_slab_handle_before_anything_is_touched():
    scene, pos0, vel0 = ts.tracers("A_stay")
    bounds = (0, 1, 2, 3)
    hub, sims = slabs(ts.A, bounds)
    add(sims, pos0, vel0)
    s = sims[1]
    before = s.tracers_with_ids(types=True)
    counts = (C.c_uint64 * 2)(7, 7)
    assert s.lib.lfa_tracers_step(s.h, sc.DT, C.byref(counts)) == E_UNSUPPORTED and tuple(counts) == (7, 7)
    assert "lfa_tracers_step_collective" in s.lib.lfa_last_error(s.h).decode()
    assert s.lib.lfa_tracers_advect_collide(s.h, sc.DT) == E_UNSUPPORTED and s.lib.lfa_tracers_transfer(s.h) == E_UNSUPPORTED
    with pytest.raises(lfa.LibfluidError) as e:
        s.add_tracers(pos0[:4], vel0[:4])
    assert e.value.code == E_UNSUPPORTED
    for a, b in zip(before, s.tracers_with_ids(types=True)):
        assert a.tobytes() == b.tobytes()
    # local calls work on a slab handle: count, download (storage order), clear
    p, v, t = s.tracers(types=True)
    assert s.num_tracers() == len(before[0]) and p.tobytes() == before[1].tobytes() and v.tobytes() == before[2].tobytes()
    close_all(hub, sims)


# ---------------------------------------------------------------------------------------------------- 5. errors without a hang
def test_state_errors_refuse_on_every_rank_without_a_message():
    scene, pos0, vel0 = ts.tracers("A_stay")
    bounds = (0, 1, 2, 3)
    hub, sims = slabs(ts.A, bounds)
    for s in sims:
        s.upload_particles(sc.sparse_particles())
    add(sims, pos0, vel0)
    before = [s.tracers_with_ids(types=True) for s in sims]
    # one rank after the other on this thread: a call that had sent a message would wait for its peers here
    for s in sims:
        with pytest.raises(lfa.LibfluidError) as e:
            s.tracers_transfer_collective()
        assert e.value.code == E_INVALID and "lfa_hash_particles" in str(e.value)
        with pytest.raises(lfa.LibfluidError) as e:
            s.tracers_step_collective(sc.DT)  # (the transfer's state check comes before the migration's first message)
        assert e.value.code == E_INVALID and "lfa_hash_particles" in str(e.value)
        for dt in (np.nan, np.inf, -np.inf):
            counts = (C.c_uint64 * 6)(*([7] * 6))
            assert s.lib.lfa_tracers_advect_collide_collective(s.h, dt, C.byref(counts)) == E_INVALID and tuple(counts) == (0,) * 6
            assert s.lib.lfa_tracers_step_collective(s.h, dt, C.byref(counts)) == E_INVALID
    for s, b in zip(sims, before):
        for x, y in zip(b, s.tracers_with_ids(types=True)):
            assert x.tobytes() == y.tobytes()
    # the job is intact: binned, it steps
    collective(sims, lambda r, s: s.hash())
    counts = collective(sims, lambda r, s: s.tracers_step_collective(sc.DT))
    assert all(c[5] == 0 for c in counts)
    close_all(hub, sims)


def test_a_bad_download_buffer_is_that_rank_s_alone():
    scene, pos0, vel0 = ts.tracers("A_stay")
    bounds = (0, 1, 2, 3)
    hub, sims = slabs(ts.A, bounds)
    add(sims, pos0, vel0)
    collective(sims, lambda r, s: s.tracers_advect_collide_collective(sc.DT))
    s = sims[1]
    n = s.num_tracers()
    assert n > 1
    ids = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    xyz = np.full(3 * n, 7.0)
    # short: LFA_E_INVALID, nothing written; NULL arrays: nothing asked, LFA_OK
    assert s.lib.lfa_tracers_download_ids(s.h, ptr(ids), ptr(xyz), None, None, n - 1) == E_INVALID
    assert (ids == 0xA5A5A5A5).all() and (xyz == 7.0).all()
    assert s.lib.lfa_tracers_download_ids(s.h, None, None, None, None, n) == 0
    assert s.lib.lfa_tracers_download_ids(s.h, ptr(ids), None, None, None, n) == 0 and (xyz == 7.0).all()
    want = ts.moved("A_stay")
    got = by_id([q.tracers_with_ids() for q in sims], len(pos0))
    assert np.array_equal(np.sort(ids), np.sort(np.flatnonzero(ts.owner(ts.A, want, bounds) == 1)).astype(np.uint32))
    assert got[0].tobytes() == want.tobytes()
    close_all(hub, sims)


# ---------------------------------------------------------------------------------------------------- 6. growth
@pytest.mark.parametrize("bounds", [tuple(b) for b in ts.A.bounds], ids=str)
def test_arrivals_beyond_the_capacity_grow_the_arrays(bounds):
    scene, pos, vel = ts.tracers("grow")
    want = ts.moved("grow")
    n, nr = len(pos), len(bounds) - 1
    design = ts.GROW_RANKS[bounds]
    hub, sims = slabs(ts.A, bounds)
    kept = [k for k, _ in add(sims, pos, vel)]
    assert [r for r in range(nr) if kept[r] == 0] == design["empty"]
    counts = collective(sims, lambda r, s: s.tracers_advect_collide_collective(ts.DT))
    got = [s.tracers_with_ids() for s in sims]
    print(bounds, "kept at the add", kept, "counts", counts, "resident", [len(g[0]) for g in got])
    got_pos, got_vel = by_id(got, n)
    assert got_pos.tobytes() == want.tobytes() and got_vel.tobytes() == vel.tobytes()
    for r in design["emptied"]:
        assert kept[r] > 0 and sims[r].num_tracers() == 0 and len(got[r][0]) == 0
    for r in design["growing"]:
        assert kept[r] == 1 and sims[r].num_tracers() == 1501
        assert got[r][0].tolist() == [0] + list(range(1, 1501))  # the stayer, then the arrivals from below in the sender's order
    # the same handles go on: a later add, and a step back down across the face for a part of the crowd
    more_pos, more_vel = (a[ts.rows("A", "face8_down_513")] for a in ts.tracers("A")[1:])
    assert all(first == n for _, first in add(sims, more_pos, more_vel))
    all_pos, all_vel = by_id([s.tracers_with_ids() for s in sims], n + 513)
    assert all_pos.tobytes() == np.concatenate([want, more_pos]).tobytes()
    collective(sims, lambda r, s: s.tracers_advect_collide_collective(ts.DT))
    got = [s.tracers_with_ids() for s in sims]
    got_pos, _ = by_id(got, n + 513)
    want2 = ts.expected_move(ts.A, all_pos, all_vel)
    assert got_pos.tobytes() == want2.tobytes()
    own = ts.owner(ts.A, want2, bounds)
    for r, g in enumerate(got):
        assert set(g[0].tolist()) == set(np.flatnonzero(own == r).tolist()), r
    close_all(hub, sims)
