"""lfa_seed_box / lfa_seed_sphere on the device against tests/seed_model.py (pinned to the reference by tests/test_seed_model.py).

Every case checks three things: the fp64 positions handed back and their count equal the model's bit for bit; the generator
state handed back equals the model's; and download_particles of the seeded handle is byte-identical to that of a second handle
that was given upload_particles of the model's records (key, fractions, velocity, C and ids)."""
import functools

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import seed_model as sm

pytestmark = pytest.mark.gpu

GRID = dict(size=(16, 12, 20), cell_size=0.7, offset=(-1.3, 0.4, 2.1))
VEL = (1.5, -0.25, 3.0)
BOX = ((0.25, 1.1, 3.0), (5.3, 4.9, 6.2))  # unaligned on all six faces
# a corner of GRID: centre - r lies below the grid in x and y, centre + r above it in z
CORNER_SPHERE = ((-0.3, 1.2, 15.1), 2.0)
BIG = dict(size=(40, 40, 24), cell_size=1.0, offset=(0.0, 0.0, 0.0))
BIG_BOX = ((0.3, 0.3, 0.3), (39.4, 39.4, 23.4))  # cells 0..39, 0..39, 0..23: 307 200 candidates at density 2


@functools.lru_cache(maxsize=None)
def model(grid, calls, state=None):
    """calls: tuple of ("box", start, size, density, ltr) / ("sphere", centre, radius, density, ltr), run one after the other.
    Returns [(positions, state after)] per call."""
    g = dict(grid)
    state = sm.initial_state() if state is None else state
    out = []
    for kind, a, b, density, ltr in calls:
        fn = sm.seed_box if kind == "box" else sm.seed_sphere
        pos, state = fn(g["size"], g["cell_size"], g["offset"], a, b, density=density, state=state, ltr=ltr)
        pos.setflags(write=False)
        out.append((pos, state))
    return out


def key(grid):
    return tuple(sorted(grid.items()))


def device_call(sim, call, state, **kw):
    kind, a, b, density, ltr = call
    fn = sim.seed_box if kind == "box" else sim.seed_sphere
    return fn(a, b, velocity=VEL, density=density, rng_state=state, flags=lfa.SEED_DRAW_LTR if ltr else 0, **kw)


def check(grid, calls, keep=False):
    want = model(key(grid), tuple(calls))
    sim = lfa.Sim(**grid)
    state, all_pos = sm.initial_state(), []
    for call, (pos, state_after) in zip(calls, want):
        n, state, got = device_call(sim, call, state, positions=True)
        assert n == len(pos) and n > 0, (call, n, len(pos))
        assert got.tobytes() == pos.tobytes(), call
        assert state == state_after, call
        all_pos.append(pos)
    all_pos = np.concatenate(all_pos)
    assert sim.num_particles == len(all_pos)
    other = lfa.Sim(**grid)
    other.upload_particles(sm.records(all_pos, VEL))
    a, b = sim.download_particles(write_positions=True), other.download_particles(write_positions=True)
    other.close()
    assert a.tobytes() == b.tobytes()
    assert not a["cx"].any() and not a["cy"].any() and not a["cz"].any()
    if keep:
        return sim, a
    sim.close()


@pytest.mark.parametrize("density", [1, 2, 3])
def test_box_with_unaligned_ends(density):
    """The predicate rejects candidates on all six faces; the cell range is e - s + 1."""
    pos, _ = model(key(GRID), (("box", *BOX, density, False),))[0]
    start, end = np.array(BOX[0]), np.array(BOX[0]) + np.array(BOX[1])
    s, e = sm.cell_unclamped(start, GRID["offset"], GRID["cell_size"]), sm.cell_unclamped(end, GRID["offset"], GRID["cell_size"])
    n_cand = int(np.prod([e[k] - s[k] + 1 for k in range(3)])) * density ** 3
    assert len(pos) < n_cand  # (the case does what it is there for)
    check(GRID, [("box", *BOX, density, False)])


def test_sphere_at_a_grid_corner():
    """max(g, 0) in two components, the upper end clamped by the grid in the third."""
    c, r = np.array(CORNER_SPHERE[0]), CORNER_SPHERE[1]
    g = (np.array([c - r, c + r]) - np.array(GRID["offset"])) / GRID["cell_size"]
    assert g[0, 0] < 0 and g[0, 1] < 0 and g[1, 2] > GRID["size"][2]
    check(GRID, [("sphere", *CORNER_SPHERE, 2, False)])


def test_sphere_then_box_appends():
    """The testbed's scene 2: ids continue behind the resident particles, the state is carried from call to call."""
    calls = [("sphere", (4.0, 7.0, 9.0), 1.2, 2, False), ("box", GRID["offset"], (11.2, 2.5, 14.0), 2, False)]
    check(GRID, calls)


@pytest.mark.parametrize("density", [2, 3])
def test_many_workgroups(density):
    """307 200 candidates (4 800 per-wave counts: several tiles of the scan's one-workgroup form) and, at density 3, 1 036 800
    (16 200 counts: the scan's three-launch form)."""
    check(BIG, [("box", *BIG_BOX, density, False)])


def test_left_to_right_draw_order():
    ltr = model(key(GRID), (("box", *BOX, 2, True),))[0][0]
    rtl = model(key(GRID), (("box", *BOX, 2, False),))[0][0]
    assert ltr.tobytes() != rtl.tobytes()
    check(GRID, [("box", *BOX, 2, True), ("sphere", *CORNER_SPHERE, 2, True)])


def test_nothing_to_seed_leaves_the_handle_alone():
    sim, before = check(GRID, [("box", *BOX, 2, False)], keep=True)
    s0 = 0x0123456789ABCDEF
    # wholly above the grid: an empty cell range, no draw
    n, state, pos = sim.seed_box((20.0, 20.0, 30.0), (1.0, 1.0, 1.0), velocity=VEL, rng_state=s0, positions=True)
    assert (n, state, len(pos)) == (0, s0, 0)
    # wholly below it: max(g, 0) makes the range cell (0, 0, 0), whose eight candidates are drawn and rejected
    call = ("box", (-10.0, -10.0, -10.0), (1.0, 1.0, 1.0), 2, False)
    (want_pos, want_state), = model(key(GRID), (call,), s0)
    assert len(want_pos) == 0 and want_state == sm.advance(s0, 48)
    n, state, pos = device_call(sim, call, s0, positions=True)
    assert (n, state, len(pos)) == (0, want_state, 0)
    assert sim.num_particles == len(before)
    assert sim.download_particles(write_positions=True).tobytes() == before.tobytes()
    sim.close()


def test_short_positions_buffer_is_refused():
    sim, before = check(GRID, [("sphere", *CORNER_SPHERE, 2, False)], keep=True)
    want = len(model(key(GRID), (("box", *BOX, 2, False),))[0][0])
    with pytest.raises(lfa.LibfluidError) as e:
        sim.seed_box(*BOX, velocity=VEL, rng_state=sm.initial_state(), positions=want - 1)
    assert e.value.code == -1  # LFA_E_INVALID
    assert sim.num_particles == len(before)
    assert sim.download_particles(write_positions=True).tobytes() == before.tobytes()
    # an exact fit is accepted
    n, _, pos = sim.seed_box(*BOX, velocity=VEL, rng_state=sm.initial_state(), positions=want)
    assert n == want == len(pos) and sim.num_particles == len(before) + want
    sim.close()


def test_bad_arguments():
    sim = lfa.Sim(**GRID)
    for density in (0, 17):
        with pytest.raises(lfa.LibfluidError) as e:
            sim.seed_box(*BOX, density=density)
        assert e.value.code == -1
    assert sim.num_particles == 0
    # a NULL generator state, and a handle whose cell_size was never set (lfa_create alone)
    import ctypes as C
    lib, three = sim.lib, (C.c_double * 3)(1.0, 1.0, 1.0)
    assert lib.lfa_seed_box(sim.h, three, three, three, 2, None, 0, None, None, 0) == -1
    raw, state = C.c_void_p(), C.c_uint64(1)
    assert lib.lfa_create(C.byref(raw), 16, 16, 16, -1) == 0
    assert lib.lfa_seed_box(raw, three, three, three, 2, C.byref(state), 0, None, None, 0) == -1
    assert lib.lfa_seed_sphere(raw, three, 2.0, three, 2, C.byref(state), 0, None, None, 0) == -1
    assert b"cell_size" in lib.lfa_last_error(raw) and state.value == 1 and lib.lfa_num_particles(raw) == 0
    lib.lfa_destroy(raw)
    sim.close()


def test_slab_decomposition_is_unsupported():
    hub = lfa.LocalHub(2)
    sims = [lfa.Sim((16, 16, 16)) for _ in range(2)]
    for r, s in enumerate(sims):
        s.init_local_slab(hub.h, r, [0, 1, 2])
    for s in sims:
        for call in (lambda: s.seed_box((1.0, 1.0, 1.0), (4.0, 4.0, 4.0)), lambda: s.seed_sphere((8.0, 8.0, 8.0), 3.0)):
            with pytest.raises(lfa.LibfluidError) as e:
                call()
            assert e.value.code == -6 and "slab" in str(e.value)  # LFA_E_UNSUPPORTED
        assert s.num_particles == 0
    for s in sims:
        s.close()
    hub.close()


def test_a_time_step_runs_on_seeded_particles():
    sim, before = check(GRID, [("box", *BOX, 2, False)], keep=True)
    _, _, rc = sim.time_step(0.005)
    assert rc >= 0 and sim.num_particles == len(before)
    # and seeding again after the step appends behind the (now binned) particles
    n, _, _ = sim.seed_sphere(*CORNER_SPHERE, velocity=VEL, rng_state=sm.initial_state())
    assert n > 0 and sim.num_particles == len(before) + n
    after = sim.download_particles(write_positions=True)
    want = model(key(GRID), (("sphere", *CORNER_SPHERE, 2, False),))[0][0]
    assert np.abs(after["pos"][len(before):] - want).max() <= GRID["cell_size"] * 2.0 ** -23
    assert np.array_equal(after["vel"][len(before):], np.broadcast_to(np.float32(VEL).astype(np.float64), (n, 3)))
    _, _, rc = sim.time_step(0.005)
    assert rc >= 0 and sim.num_particles == len(before) + n
    sim.close()
