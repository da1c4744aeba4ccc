"""Tracers on the device (libfluid_amd/csrc/tracers.hip) against tests/tracer_cases.py: positions equal the oracle's
_advect_particles + _detect_collisions, velocities and types the oracle's PIC transfer on a download of the same handle - every
comparison np.array_equal on fp64, no tolerance. Every operation is an IEEE fp64 operation in a fixed order, so a differing bit is a
bug: contraction, reassociation, grid units where the reference works in world units, or a second copy of a rule."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import move_cases as mc
from tests import sample_cases as sc
from tests import tracer_cases as tc

pytestmark = pytest.mark.gpu


def same(a, b):
    """Bit for bit (np.array_equal alone takes -0.0 for +0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.array_equal(a, b) and a.tobytes() == b.tobytes()


def scene_sim(**kw):
    kw.setdefault("method", lfa.PIC)
    sim = lfa.Sim(sc.SIZE, cell_size=sc.H, offset=sc.OFFSET, gravity=sc.GRAVITY, **kw)
    sim.set_solid_cells(tc.block_cells())
    sim.upload_particles(sc.sparse_particles())
    return sim


def oracle_move(pos, vel, dt=sc.DT):
    return tc.advect_collide(sc.SIZE, sc.H, sc.OFFSET, tc.block_cells(), pos, vel, dt)["collide"]


# ---------------------------------------------------------------------------------------------------- 1. move and collide
@pytest.mark.parametrize("name", tc.MOVE_NAMES)
def test_advect_collide_stage_is_the_oracle(name):
    size, h, off, dt, solid, pos, vel = tc.move_case(name)
    sim = lfa.Sim(size, cell_size=h, offset=off, method=mc.METHOD, blending=mc.BLEND)
    if solid is not None:
        sim.set_solid_cells(solid)
    sim.upload_particles(mc.build(name)[1])
    parts_before = sim.download_particles(write_positions=True)
    sim.add_tracers(pos, vel)
    assert sim.num_tracers() == len(pos)
    sim.tracers_advect_collide(dt)
    got_pos, got_vel = sim.tracers()
    want = mc.oracle(name)["collide"]
    bad = np.flatnonzero((got_pos != want).any(axis=1))
    print(name, "tracers", len(pos), "rows that differ", len(bad), "moved by the collision handling",
          int((want != mc.oracle(name)["advect"]).any(axis=1).sum()))
    assert same(got_pos, want), (name, bad[:8], got_pos[bad[:4]], want[bad[:4]])
    assert same(got_vel, vel)
    assert sim.download_particles(write_positions=True).tobytes() == parts_before.tobytes()
    sim.close()


# ---------------------------------------------------------------------------------------------------- 2. transfer
def test_transfer_stage_is_the_model_and_sample_velocity():
    pts, field = tc.transfer_points(), sc.random_field()
    sim = lfa.Sim(sc.SIZE, cell_size=sc.H, offset=sc.OFFSET, gravity=sc.GRAVITY, method=lfa.PIC)
    sim.upload_cells(field)
    sim.add_tracers(pts, np.full_like(pts, 7.0))
    sim.tracers_transfer()
    pos, vel, types = sim.tracers(types=True)
    want_vel, want_types, n_out = sc.model(sim.cells(), pts)
    assert same(pos, pts)
    assert same(vel, want_vel) and same(types, want_types) and n_out == 7
    s_vel, s_types, s_out = sim.sample_velocity(pts, types=True)
    assert same(vel, s_vel) and same(types, s_types) and s_out == 7
    sim.close()


# ---------------------------------------------------------------------------------------------------- 3. fused == staged
def test_fused_step_equals_the_stages():
    pos0, vel0 = tc.stepped_tracers()
    sim = scene_sim()
    sim.time_step(sc.DT)
    sim.add_tracers(pos0, vel0)
    sim.tracers_advect_collide(sc.DT)
    sim.tracers_transfer()
    staged = sim.tracers(types=True)
    sim.clear_tracers()
    assert sim.num_tracers() == 0
    sim.add_tracers(pos0, vel0)
    stopped, frozen = sim.tracers_step(sc.DT)
    fused = sim.tracers(types=True)
    for a, b in zip(staged, fused):
        assert same(a, b)
    want_pos, want_stopped = tc.march_model(sc.SIZE, tc.solid_mask(), sc.H, sc.OFFSET, pos0, vel0, sc.DT)
    assert same(fused[0], want_pos) and same(fused[0], oracle_move(pos0, vel0))
    assert (stopped, frozen) == (int(want_stopped.sum()), 0) and stopped == tc.stepped_cpu_model()[1][0] >= 20
    sim.close()


# ---------------------------------------------------------------------------------------------------- 4. three steps
def test_three_steps_are_exact_every_step():
    pos0, vel0 = tc.stepped_tracers()
    sim = scene_sim()
    sim.add_tracers(pos0, vel0)
    mask, total = tc.solid_mask(), 0
    for step in range(3):
        sim.time_step(sc.DT)
        pos, vel = sim.tracers()
        cells = sim.cells()
        stopped, frozen = sim.tracers_step(sc.DT)
        got_pos, got_vel, got_types = sim.tracers(types=True)
        want_pos = oracle_move(pos, vel)
        want_vel, want_types, n_out = sc.model(cells, want_pos)
        model_pos, model_stopped = tc.march_model(sc.SIZE, mask, sc.H, sc.OFFSET, pos, vel, sc.DT)
        print("step", step, "stopped", stopped, "frozen", frozen, "rows that differ", int((got_pos != want_pos).any(axis=1).sum()))
        assert same(got_pos, want_pos) and same(model_pos, want_pos), step
        assert same(got_vel, want_vel) and same(got_types, want_types) and n_out == 0, step
        assert (stopped, frozen) == (int(model_stopped.sum()), 0), step
        c = sc.cells_of(sc.classify(got_pos)[0])
        assert not mask[c[:, 0], c[:, 1], c[:, 2]].any() and not (got_types == orc.SOLID).any(), step
        assert same(sim.cells(), cells), step  # the tracer step writes nothing but the tracer arrays
        total += stopped
    assert total > 0
    sim.close()


# ---------------------------------------------------------------------------------------------------- 5. the simulation is untouched
def test_the_simulation_is_untouched():
    pos0, vel0 = tc.stepped_tracers()
    sim = scene_sim()
    sim.time_step(sc.DT)

    def state():
        st, occ = sim.frame_stats()
        return sim.download_particles(write_positions=True).tobytes(), sim.cells().tobytes(), bytes(st), occ.tobytes()

    before = state()
    sim.add_tracers(pos0, vel0)
    sim.tracers_step(sc.DT)
    sim.tracers(types=True)
    sim.clear_tracers()
    assert state() == before
    sim.close()


# ---------------------------------------------------------------------------------------------------- 6. edges
def test_zero_tracers():
    sim = scene_sim()
    assert sim.num_tracers() == 0
    sim.tracers_advect_collide(sc.DT)
    sim.tracers_transfer()
    assert sim.tracers_step(sc.DT) == (0, 0)
    pos, vel, types = sim.tracers(types=True)
    assert pos.shape == (0, 3) and vel.shape == (0, 3) and types.shape == (0,)
    sim.add_tracers(np.zeros((0, 3)))
    assert sim.num_tracers() == 0
    ms = C.c_double(-1.0)
    assert sim.lib.lfa_tracers_time(sim.h, C.byref(ms)) == -1  # LFA_E_INVALID: no tracer kernel has run
    sim.close()


def test_batches_grow_with_live_contents():
    pos0, vel0 = (a[:257] for a in tc.stepped_tracers())
    sim = scene_sim()
    sim.time_step(sc.DT)
    sim.add_tracers(pos0[:255], vel0[:255])
    sim.add_tracers(pos0[255:], vel0[255:])
    assert sim.num_tracers() == 257
    sim.tracers_step(sc.DT)
    two = sim.tracers(types=True)
    sim.clear_tracers()
    sim.add_tracers(pos0, vel0)
    sim.tracers_step(sc.DT)
    one = sim.tracers(types=True)
    for a, b in zip(two, one):
        assert same(a, b)
    assert same(one[0], oracle_move(pos0, vel0))
    # growth beyond the first allocation with live contents: the rest of the set on top
    rest = tc.stepped_tracers()[0][257:]
    big = np.tile(rest, (5, 1))
    sim.add_tracers(big)
    pos, vel = sim.tracers()
    assert same(pos[:257], one[0]) and same(vel[:257], one[1]) and same(pos[257:], big) and not vel[257:].any()
    sim.close()


def test_a_nan_position_is_rejected():
    pos0, vel0 = (a[:64].copy() for a in tc.stepped_tracers())
    sim = scene_sim()
    sim.add_tracers(pos0[:10], vel0[:10])
    bad = pos0.copy()
    bad[37, 1] = np.nan
    with pytest.raises(lfa.LibfluidError) as e:
        sim.add_tracers(bad, vel0)
    assert e.value.code == -1 and "37" in str(e.value)
    bad[37, 1] = np.inf
    with pytest.raises(lfa.LibfluidError):
        sim.add_tracers(bad)
    assert sim.num_tracers() == 10
    assert same(sim.tracers()[0], pos0[:10])
    sim.close()


def test_a_nan_velocity_freezes_its_tracer():
    pos0, vel0 = (a[:64].copy() for a in tc.stepped_tracers())
    vel0[21, 2] = np.nan
    sim = scene_sim()
    sim.time_step(sc.DT)
    cells = sim.cells()
    sim.add_tracers(pos0, vel0)
    stopped, frozen = sim.tracers_step(sc.DT)
    pos, vel = sim.tracers()
    assert frozen == 1
    assert same(pos[21], pos0[21]) and np.isfinite(vel[21]).all()
    others = np.arange(64) != 21
    want = oracle_move(pos0[others], vel0[others])
    assert same(pos[others], want)
    want_pos = pos0.copy()
    want_pos[others] = want
    assert same(vel, sc.model(cells, want_pos)[0])
    assert stopped == int(tc.march_model(sc.SIZE, tc.solid_mask(), sc.H, sc.OFFSET, pos0[others], vel0[others], sc.DT)[1].sum())
    sim.close()


def test_a_dt_that_is_not_finite_is_rejected():
    pos0, vel0 = (a[:64] for a in tc.stepped_tracers())
    sim = scene_sim()
    sim.add_tracers(pos0, vel0)
    for dt in (np.nan, np.inf, -np.inf):
        with pytest.raises(lfa.LibfluidError) as e:
            sim.tracers_step(dt)
        assert e.value.code == -1
        with pytest.raises(lfa.LibfluidError):
            sim.tracers_advect_collide(dt)
    assert same(sim.tracers()[0], pos0)
    sim.close()


def test_slab_handles_take_no_tracers():
    pos0, vel0 = (a[:64] for a in tc.stepped_tracers())
    ntz = -(-sc.SIZE[2] // 8)
    hub = lfa.LocalHub(1)
    slab = scene_sim()
    slab.init_local_slab(hub.h, 0, [0, ntz])
    with pytest.raises(lfa.LibfluidError) as e:
        slab.add_tracers(pos0, vel0)
    assert e.value.code == -6 and slab.num_tracers() == 0  # LFA_E_UNSUPPORTED
    # and a handle that holds tracers takes no transport
    single = scene_sim()
    single.add_tracers(pos0, vel0)
    with pytest.raises(lfa.LibfluidError) as e:
        single.init_local_slab(hub.h, 0, [0, ntz])
    assert e.value.code == -6
    single.tracers_step(sc.DT)  # still a single domain
    assert same(single.tracers()[0], oracle_move(pos0, vel0))
    single.close()
    slab.close()
    hub.close()


def test_the_step_is_timed():
    pos0, vel0 = tc.stepped_tracers()
    sim = scene_sim()
    sim.add_tracers(pos0, vel0)
    sim.tracers_step(sc.DT)
    assert sim.tracers_ms() > 0.0
    sim.close()
