"""CPU tests of tests/move_cases.py: the oracle is the reference on exactly these inputs (without that a device-against-oracle
comparison on them proves nothing), the inputs are dyadic, and every case holds what it is there for - counted with restatements
of the short cut's rule and of _detect_collisions that are checked against the oracle themselves."""
import numpy as np
import pytest

from oracle import loader as orc
from tests import move_cases as mc


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name", mc.NAMES)
def test_oracle_is_the_reference_on_the_adversarial_moves(name):
    """Advect alone and advect + detect_collisions, to 1e-13 (of a cell; positions are O(10))."""
    cloud = mc.build(name)
    want, got = mc.run_cpu(cloud, "ref"), mc.oracle(name)
    for k in ("advect", "collide"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * cloud[3]["h"], k


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
def test_oracle_is_the_reference_with_the_coercing_source():
    cloud, source = mc.coerce_source()
    want, got = mc.run_cpu(cloud, "ref", source), mc.run_cpu(cloud, "oracle", source)
    for k in ("advect", "collide", "vel"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13, k


@pytest.mark.parametrize("name", mc.NAMES)
def test_inputs_are_dyadic(name):
    size, parts, solid, meta = mc.build(name)
    h, off, dt = meta["h"], np.asarray(meta["off"]), meta["dt"]
    assert h in (1.0, 0.5, 2.0) and np.array_equal(off * 8, np.rint(off * 8)) and np.frexp(dt)[0] == 0.5
    assert meta["skin"] == 0.1 / h
    cells = (parts["pos"] - off) / h
    assert np.array_equal(cells * mc.Q, np.rint(cells * mc.Q)) and np.array_equal(np.rint(cells * mc.Q), meta["q16"])
    assert np.array_equal(off + cells * h, parts["pos"])  # the round trip is exact
    vel = parts["vel"]
    assert np.array_equal(vel * mc.M, np.rint(vel * mc.M)) and np.array_equal(vel.astype(np.float32).astype(np.float64), vel)
    move = vel * (dt / h)
    assert np.array_equal(move * mc.M, meta["m12"])
    end = cells + move
    assert np.array_equal(end * mc.Q, np.rint(end * mc.Q))  # an fp32 fraction (2^-23) holds the moved position exactly
    assert (cells >= 0).all() and (cells <= np.asarray(size)).all()
    assert np.array_equal(np.rint(parts["cx"][:, 0]), np.arange(len(parts)))
    assert max(size) <= 32 and len(parts) <= 4000 and len(parts) % 512


def test_particle_counts():
    counts = {name: len(mc.build(name)[1]) for name in mc.NAMES}
    print(counts)
    assert {1, 511, 513} <= set(counts.values())
    assert counts["lone_reach"] == 1 and all(counts[n] == 64 for n in mc.REACH)


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_restated_collision_handling_is_the_oracle_s_and_meets_no_tie(name):
    """collide_model counts bounces for the tests below: it has to end where the oracle ends. And no segment crosses two cell
    faces at (nearly) the same time: the DDA of the device and of the reference never have to break a tie."""
    size, parts, solid, meta = mc.build(name)
    end, bounces, gap = mc.model(name)
    assert np.abs(end - mc.cells_of(mc.oracle(name)["collide"], meta)).max() <= 1e-12
    assert gap > 1e-7, gap
    a, b, clamped = mc.free_flight(mc.build(name))
    assert np.abs(mc.cells_of(mc.oracle(name)["advect"], meta) - clamped).max() <= 1e-13


@pytest.mark.parametrize("name", mc.REACH + ("lone_reach",))
def test_tile_reach_takes_the_short_cut_and_still_needs_the_push_out(name):
    """At least 20 particles meet the short cut's rule (start tile clear, |move| < 8 per axis) AND are moved by the oracle by at
    least 0.02 cells from the clamped free flight - the plate's skin, two tiles from the start tile -; at least 20 meet it and
    need nothing. (lone_reach: its one particle is of the first kind.)"""
    cloud = mc.build(name)
    size, parts, solid, meta = cloud
    a, b, clamped = mc.free_flight(cloud)
    ow = mc.open_water(cloud)
    off_by = np.abs(mc.cells_of(mc.oracle(name)["collide"], meta) - clamped).max(axis=1)
    klass = np.array(meta["klass"])
    need, fine = ow & (off_by >= 0.02), ow & (off_by == 0.0)
    assert np.array_equal(need, klass == "skin") and np.array_equal(fine, klass == "short")
    assert np.array_equal(ow, np.abs(meta["m12"]).max(axis=1) < 8 * mc.M)
    if name == "lone_reach":
        assert need.all()
        return
    assert need.sum() >= 20 and fine.sum() >= 20
    assert (off_by[need] <= meta["skin"]).all()
    # the moves of 7 cells and more are all there, on both sides of 7.0 and of 8.0
    assert {abs(int(m)) for m in meta["m12"][:, meta["axis"]]} == {int(mc.m12_of(m)) for m in mc.REACH_MOVES}
    # the march stops the ones that end inside the plate
    assert ((mc.model(name)[1] == 1) & (klass == "far")).sum() >= 5
    # the start lies in the last `skin` of the far face layer of the start tile
    u = a[:, meta["axis"]] if meta["sign"] > 0 else 24 - a[:, meta["axis"]]
    assert (u >= 8 - meta["skin"]).all() and (u < 8).all()
    tr = [k for k in range(3) if k != meta["axis"]]
    assert (np.abs(b - a)[:, tr] < 1.0).all()


def test_obstacles_bounce_once_twice_and_three_times():
    cloud = mc.build("obstacles")
    size, parts, solid, meta = cloud
    end, bounces, _ = mc.model("obstacles")
    a, b, clamped = mc.free_flight(cloud)
    counts = np.bincount(bounces, minlength=4)
    print("bounces 0..3:", counts)
    assert (counts[1:] >= 20).all()
    pushed_only = (bounces == 0) & (np.abs(end - clamped).max(axis=1) > 1e-3)
    assert pushed_only.sum() >= 20
    # starts within the skin of a solid face on each of the six sides
    mask = np.pad(mc.solid_mask(size, solid), 1)
    cell, frac = a.astype(np.int64), a - a.astype(np.int64)
    for d in range(3):
        e = np.eye(3, dtype=np.int64)[d]
        lo, hi = cell - e + 1, cell + e + 1
        assert ((frac[:, d] < meta["skin"]) & mask[lo[:, 0], lo[:, 1], lo[:, 2]]).sum() >= 20
        assert ((frac[:, d] > 1 - meta["skin"]) & mask[hi[:, 0], hi[:, 1], hi[:, 2]]).sum() >= 20
    assert any(s % 8 for s in size) and np.abs(b - a).max() > 6.5


def test_axis_aligned_sits_on_faces_with_zero_velocity_and_hits():
    cloud = mc.build("axis_aligned")
    size, parts, solid, meta = cloud
    end, bounces, _ = mc.model("axis_aligned")
    a, b, clamped = mc.free_flight(cloud)
    on = meta["on_face"]
    assert np.array_equal(on, (meta["q16"] % mc.Q == 0))
    assert (meta["m12"][on] == 0).all()
    nan_path = on.any(axis=1)
    assert nan_path.all() and (on.sum(axis=1) == 2).sum() >= 20
    hit_solid = nan_path & (bounces >= 1)
    hit_wall = nan_path & (bounces == 0) & (np.abs(clamped - b).max(axis=1) > 0.1)
    print("on a face and into the block:", hit_solid.sum(), "into a wall:", hit_wall.sum())
    assert hit_solid.sum() >= 20 and hit_wall.sum() >= 20
    assert (nan_path & (np.abs(end - b).max(axis=1) == 0.0)).sum() >= 10  # and some that meet nothing
    # off a face with zero velocity: t = inf
    assert (~on & (meta["m12"] == 0)).any(axis=1).sum() >= 20


def test_still_is_pushed_out_of_solids_walls_and_corners():
    cloud = mc.build("still")
    size, parts, solid, meta = cloud
    end, bounces, _ = mc.model("still")
    a = mc.cells_of(parts["pos"], meta)
    assert not parts["vel"].any() and not bounces.any()
    moved = np.abs(end - a) > 0.02
    assert (moved.sum(axis=1) == 1).sum() >= 20 and (moved.sum(axis=1) == 2).sum() >= 20 and (moved.sum(axis=1) == 3).sum() >= 8
    cell = a.astype(np.int64)
    at_wall = (cell == 0) | (cell == np.asarray(size) - 1)
    assert (moved & at_wall).sum() >= 20 and (moved & ~at_wall).sum() >= 20  # walls and solid neighbours
    assert (moved & at_wall).any(axis=1)[(moved & ~at_wall).any(axis=1)].sum() >= 8  # both at once
    assert ((~moved).all(axis=1)).sum() >= 20


@pytest.mark.parametrize("name", [n for n in mc.NAMES if n.startswith("walls")])
def test_walls_clamp_far_moves_and_end_beside_the_skin(name):
    cloud = mc.build(name)
    size, parts, solid, meta = cloud
    a, b, clamped = mc.free_flight(cloud)
    assert solid is None
    n = np.asarray(size)
    assert (np.abs(b - a) > 3 * n).any() and (clamped != b).any()
    lo, hi = meta["skin"], n - meta["skin"]
    step = 1.0 / mc.M
    for edge in (lo * np.ones(3), hi):
        d = b - edge
        assert ((d > 0) & (d < step)).any() and ((d < 0) & (d > -step)).any()  # the dyadic neighbours of skin and n - skin
    end = mc.cells_of(mc.oracle(name)["collide"], meta)
    at = (np.abs(end - lo) < 1e-9) | (np.abs(end - hi) < 1e-9)
    assert (end >= lo - 1e-12).all() and (end <= hi + 1e-12).all()
    if min(size) >= 5:
        assert (at.sum(axis=1) == 2).any() and (at.sum(axis=1) == 3).any()  # edges and corners


@pytest.mark.parametrize("name", mc.ISOLATED)
def test_isolated_cases_keep_two_cells_between_particles(name):
    """Chebyshev distance >= 2 cells before and after the move: the position correction (springs below 0.71 cells) is a no-op."""
    size, parts, solid, meta = mc.build(name)
    assert meta["isolated"]
    for pos in (parts["pos"], mc.oracle(name)["collide"]):
        c = mc.cells_of(pos, meta)
        d = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2)
        d[np.diag_indices(len(c))] = np.inf
        assert len(c) == 1 or d.min() >= 2.0, d.min()
    # and the oracle's whole time step moves them nowhere else (nothing but the advection moves an isolated particle)
    assert np.abs(mc.oracle_time_step(name) - mc.oracle(name)["collide"]).max() <= 1e-12 * meta["h"]


def test_the_coercing_source_takes_half_the_start_cells():
    cloud, (cells, vel) = mc.coerce_source()
    size, parts, solid, meta = cloud
    start = mc.cells_of(parts["pos"], meta).astype(np.int64)
    taken = np.array([(c == cells).all(axis=1).any() for c in start])
    assert 20 <= taken.sum() <= len(parts) - 20
    assert 7.0 < vel[0] < 8.0 and np.array_equal(np.asarray(vel) * mc.M, np.rint(np.asarray(vel) * mc.M))
    assert (parts["vel"][:, 0] < 0).all()
    out = mc.run_cpu(cloud, "oracle", source=(cells, vel))
    assert np.array_equal((out["vel"] == np.asarray(vel)).all(axis=1), taken)
    a = mc.cells_of(parts["pos"], meta)
    flight = a + np.where(taken[:, None], np.asarray(vel), parts["vel"]) * meta["dt"] / meta["h"]
    pushed = taken & (np.abs(mc.cells_of(out["collide"], meta) - flight).max(axis=1) >= 0.02)
    assert pushed.sum() >= 8, pushed.sum()  # coerced, through the short cut's rule, into the plate's skin
