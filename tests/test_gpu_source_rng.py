"""lfa_update_sources_rng / lfa_set_source_rng on the device against tests/source_model.py (pinned to the reference by
tests/test_source_model.py), in the scenes of tests/source_cases.py.

Every case checks: the count, the fp64 positions handed back and the generator state handed back equal the model's bit for bit;
and the download (by id) of the seeded handle is byte-identical to that of a second handle that was given the resident records
plus the model's through lfa_upload_particles and binned them - position, velocity, C = 0 and cell of every particle."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from libfluid_amd import scenes
from tests import seed_model as sm
from tests import source_cases as sc
from tests import source_model as srcm

pytestmark = pytest.mark.gpu

NO_PARTS = np.zeros(0, dtype=lfa.PARTICLE_DTYPE)


def sim_of(name, sources=True):
    grid, parts, srcs, _ = sc.case(name)
    s = lfa.Sim(**grid)
    s.upload_particles(NO_PARTS if parts is None else parts)
    s.hash()
    for cells, vel, root, active in (srcs if sources else []):
        s.add_source(cells, vel, root, active, False)
    return s


def uploaded(grid, *record_sets):
    """Download of a handle that was given the records through lfa_upload_particles and binned them."""
    other = lfa.Sim(**grid)
    other.upload_particles(np.concatenate(record_sets))
    other.hash()
    out, ids = other.download_particles(write_positions=True), other.particle_ids()
    other.close()
    assert np.array_equal(np.sort(ids), np.arange(len(out)))
    return out


def assert_handle_holds(sim, grid, parts, pos, vel):
    got = sim.download_particles(write_positions=True)
    assert np.array_equal(np.sort(sim.particle_ids()), np.arange(len(got)))  # ids continue in draw order, none twice
    want = uploaded(grid, NO_PARTS if parts is None else parts, srcm.records(pos, vel))
    assert len(got) == len(want)
    new = got[len(got) - len(pos):]
    assert not new["cx"].any() and not new["cy"].any() and not new["cz"].any()
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", sc.ALL)
def test_case(name):
    grid, parts, _, ltr = sc.case(name)
    pos, _, vel, state = sc.expected(name)
    sim = sim_of(name)
    n, got_state, got_pos = sim.update_sources_rng(sm.initial_state(), flags=lfa.SEED_DRAW_LTR if ltr else 0, positions=True)
    assert n == len(pos) > 0
    assert got_pos.tobytes() == pos.tobytes()
    assert got_state == state
    assert sim.num_particles == (0 if parts is None else len(parts)) + n
    assert_handle_holds(sim, grid, parts, pos, vel)
    # every cell is at its target now (or above it): a second call creates what the lowered counts of the model make it create
    counts = sim.cell_counts()
    pos2, _, vel2, state2 = srcm.update_sources(grid["size"], grid["cell_size"], grid["offset"], counts, sc.case(name)[2], state, ltr=ltr)
    n2, got_state2, _ = sim.update_sources_rng(state, flags=lfa.SEED_DRAW_LTR if ltr else 0)
    assert (n2, got_state2) == (len(pos2), state2)
    if name in ("A", "B", "E_root16", "E_root1", "F_ltr_B"):  # (C and D list a cell under a smaller and then a larger target)
        assert n2 == 0 and got_state2 == state  # nothing to create: the state is left alone
    else:
        assert n2 > 0
    sim.close()


def test_handle_mode_in_time_steps_and_staged():
    """G: lfa_set_source_rng - the seeding inside lfa_time_step and the plain lfa_update_sources draw from the handle's state."""
    grid = sc.UNIT16
    cells = [(x, 15, z) for z in range(5, 11) for x in range(5, 11)]  # on the top face
    sources = [(cells, (0.0, -30.0, 0.0), 2, True)]
    s0 = sm.initial_state()
    pos, _, vel, s1 = srcm.update_sources(grid["size"], 1.0, grid["offset"], np.zeros(16 ** 3), sources, s0)
    sim = lfa.Sim(**grid)
    sim.upload_particles(NO_PARTS)
    sim.add_source(*sources[0], False)
    assert sim.get_source_rng() == (False, 0)
    sim.set_source_rng(True, s0)
    assert sim.get_source_rng() == (True, s0)
    assert sim.time_step(0.004)[2] >= 0
    assert sim.num_particles == len(pos) == 8 * len(cells)
    sim.hash()
    assert np.array_equal(np.sort(sim.particle_ids()), np.arange(len(pos)))
    assert sim.get_source_rng() == (True, s1)
    assert sim.time_step(0.004)[2] >= 0
    growth = sim.num_particles - len(pos)
    assert sim.get_source_rng() == (True, sm.advance(s1, 6 * growth))
    # staged: the model is fed the counts the device binned and the carried state
    state = sim.get_source_rng()[1]
    for _ in range(2):
        sim.advect_collide(0.01)
        sim.hash()
        before = sim.num_particles
        want_pos, _, want_vel, state = srcm.update_sources(grid["size"], 1.0, grid["offset"], sim.cell_counts(), sources, state)
        assert sim.update_sources() == len(want_pos) > 0
        assert sim.get_source_rng() == (True, state)
        got = sim.download_particles(write_positions=True)
        assert len(got) == before + len(want_pos)
        assert got[before:].tobytes() == uploaded(grid, srcm.records(want_pos, want_vel)).tobytes()
    # and off again: the state is dropped, the counter-based generator is back
    sim.set_source_rng(False)
    assert sim.get_source_rng() == (False, 0)
    sim.close()


def test_chain_from_seed_box():
    """H: Sim.seed_box hands back a state, update_sources_rng goes on from it."""
    grid = sc.UNIT16
    box = ((2.3, 1.2, 3.1), (5.5, 2.4, 4.2))
    cells = [(x, 3, z) for z in range(3, 9) for x in range(1, 9)]  # overlaps the box's top cells, and dry cells beside it
    sources = [(cells, (2.0, 0.0, 0.0), 2, True)]
    box_pos, s1 = sm.seed_box(grid["size"], 1.0, grid["offset"], *box, density=2)
    counts = srcm.cell_counts(grid["size"], 1.0, grid["offset"], box_pos)
    pos, _, vel, s2 = srcm.update_sources(grid["size"], 1.0, grid["offset"], counts, sources, s1)
    sim = lfa.Sim(**grid)
    n, state, _ = sim.seed_box(*box, velocity=(0.0, 1.0, 0.0), density=2, rng_state=sm.initial_state())
    assert (n, state) == (len(box_pos), s1)
    sim.hash()
    sim.add_source(*sources[0], False)
    n, state, got_pos = sim.update_sources_rng(state, positions=True)
    assert 0 < n == len(pos) < 8 * len(cells) and state == s2
    assert got_pos.tobytes() == pos.tobytes()
    assert_handle_holds(sim, grid, sm.records(box_pos, (0.0, 1.0, 0.0)), pos, vel)
    sim.close()


def test_refusals_leave_everything_alone():
    """I: slabs are unsupported; an unbinned handle, a short positions buffer, a NULL state are invalid."""
    s0 = 0x0123456789ABCDEF
    # two virtual slabs
    hub = lfa.LocalHub(2)
    sims = [lfa.Sim((16, 16, 16)) for _ in range(2)]
    for r, s in enumerate(sims):
        s.init_local_slab(hub.h, r, [0, 1, 2])
    for s in sims:
        s.add_source([(3, 3, 3), (3, 3, 12)], (0.0, 0.0, 0.0), 2, True, False)
        state = C.c_uint64(s0)
        assert s.lib.lfa_update_sources_rng(s.h, C.byref(state), 0, None, None, 0) == -6  # LFA_E_UNSUPPORTED
        assert b"slab" in s.lib.lfa_last_error(s.h) and state.value == s0
        with pytest.raises(lfa.LibfluidError) as e:
            s.set_source_rng(True, s0)
        assert e.value.code == -6 and s.get_source_rng() == (False, 0) and s.num_particles == 0
    for s in sims:
        s.close()
    hub.close()
    # a transport attached after the mode was switched on: the plain call and the step refuse
    hub = lfa.LocalHub(2)
    sims = [lfa.Sim((16, 16, 16)) for _ in range(2)]
    for r, s in enumerate(sims):
        s.set_source_rng(True, s0)
        s.init_local_slab(hub.h, r, [0, 1, 2])
        s.add_source([(3, 3, 3), (3, 3, 12)], (0.0, 0.0, 0.0), 2, True, False)
    for s in sims:
        for call in (s.update_sources, lambda: s.time_step(0.01)):
            with pytest.raises(lfa.LibfluidError) as e:
                call()
            assert e.value.code == -6
        assert s.get_source_rng() == (True, s0) and s.num_particles == 0
    for s in sims:
        s.close()
    hub.close()
    # single domain
    grid, parts, srcs, _ = sc.case("C")
    sim = lfa.Sim(**grid)
    sim.upload_particles(parts)  # not binned yet
    for cells, vel, root, active in srcs:
        sim.add_source(cells, vel, root, active, False)
    before = sim.download_particles(write_positions=True)
    state = C.c_uint64(s0)
    assert sim.lib.lfa_update_sources_rng(sim.h, C.byref(state), 0, None, None, 0) == -1  # LFA_E_INVALID: unbinned
    assert state.value == s0 and sim.num_particles == len(parts)
    sim.hash()
    want = len(sc.expected("C")[0])
    with pytest.raises(lfa.LibfluidError) as e:
        sim.update_sources_rng(s0, positions=want - 1)
    assert e.value.code == -1
    assert sim.lib.lfa_update_sources_rng(sim.h, None, 0, None, None, 0) == -1
    assert sim.lib.lfa_update_sources_rng(sim.h, C.byref(state), 4, None, None, 0) == -1  # an unknown flag
    assert state.value == s0 and sim.num_particles == len(parts)
    assert sim.download_particles(write_positions=True).tobytes() == before.tobytes()
    # an exact fit is accepted
    n, _, pos = sim.update_sources_rng(s0, positions=want)
    assert n == want == len(pos)
    sim.close()
    # cell_size never set (lfa_create alone)
    raw = C.c_void_p()
    lib = lfa.load_library()
    assert lib.lfa_create(C.byref(raw), 16, 16, 16, -1) == 0
    assert lib.lfa_update_sources_rng(raw, C.byref(state), 0, None, None, 0) == -1
    assert b"cell_size" in lib.lfa_last_error(raw) and state.value == s0 and lib.lfa_num_particles(raw) == 0
    lib.lfa_destroy(raw)


def test_mode_off_is_the_default_path():
    """J: a handle whose mode was switched on and off again seeds what a handle that never heard of the mode seeds."""
    plain, toggled = sim_of("B"), sim_of("B")
    toggled.set_source_rng(True, 12345, lfa.SEED_DRAW_LTR)
    toggled.set_source_rng(False)
    for _ in range(2):  # (the second call: the sequence of the counter-based generator goes on alike)
        assert plain.update_sources() == toggled.update_sources()
        a, b = plain.download_particles(write_positions=True), toggled.download_particles(write_positions=True)
        assert a.tobytes() == b.tobytes()
        plain.advect_collide(0.05); toggled.advect_collide(0.05)
        plain.hash(); toggled.hash()
    assert np.array_equal(plain.particle_ids(), toggled.particle_ids())
    plain.close(); toggled.close()


def test_counter_based_default_against_the_model():
    """K: the plain lfa_update_sources (no pcg32) creates the records of source_model.counter_update_sources, byte for byte, in
    two consecutive calls (the epoch advances); the resident records stay what they were."""
    grid = sc.COUNTER_GRID
    sim = lfa.Sim(**grid)
    sim.upload_particles(sc.counter_parts())
    sim.hash()
    for cells, vel, root, active in sc.COUNTER_SOURCES:
        sim.add_source(cells, vel, root, active, False)
    held = sim.download_particles(write_positions=True)
    for (want, ids), n_want in zip((c[0] for c in sc.counter_expected(2)), (86, 19)):
        assert len(want) == n_want
        assert sim.update_sources() == n_want
        got = sim.download_particles(write_positions=True)  # (single domain: record i is particle i)
        assert np.array_equal(sim.particle_ids(), np.arange(len(held) + n_want))
        assert np.array_equal(ids, np.arange(len(held), len(held) + n_want))
        assert got[:len(held)].tobytes() == held.tobytes()
        assert got[len(held):].tobytes() == want.tobytes()
        held = got
    sim.close()
