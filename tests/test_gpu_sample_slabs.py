"""lfa_sample_velocity_collective on virtual slabs (N handles on one GPU, in-process transport, one host thread per rank for every
collective, as in tests/test_gpu_seed_slabs.py) against tests/sample_cases.py's model on the ranks' downloads stitched by owned
z-range (tests/sample_slab_cases.py: stitch): every rank gets exactly the points of tests/sample_slab_cases.py's owner(), compact and
in input order, with the model's velocity and type bytes - tolerance 0. tests/test_sample_slab_cases.py asserts on the CPU that the
points put more than a thousand blocks across every slab face from either side, and that on the face z = 8 only the fp64 division
decides the owner.

States: (a) binned handles with a random grid uploaded on every rank, (b) particles after hash + P2G + gravity, (c) after two time
steps, (d) then a collective seed_box inside a tile that was implicit, and a collective hash: the binning's halo lists then follow
tile_flag while the grid the view reads still follows grid_flag, and the rank that kept the new particles reads its grid under
another rule than its neighbours."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import sample_cases as sc
from tests import sample_slab_cases as ss
from tests.test_gpu_seed_slabs import close_all, collective, make_slabs

pytestmark = pytest.mark.gpu

POINTS = sc.points()
N = len(POINTS)
INSIDE = sc.classify(POINTS)[1]
GRID = dict(size=sc.SIZE, cell_size=sc.H, offset=sc.OFFSET)
KW = dict(gravity=sc.GRAVITY, method=lfa.PIC)
E_INVALID, E_UNSUPPORTED = -1, -6


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def raw_call(sim, pts, capacity, fill=0xA5):
    """The C call on buffers of `capacity` rows pre-filled with a pattern: (rc, index, velocity, types, counts)."""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    idx = np.full(max(capacity, 1), fill * 0x01010101, dtype=np.uint32)
    vel = np.frombuffer(bytes([fill]) * (24 * max(capacity, 1)), dtype=np.float64).copy()
    typ = np.full(max(capacity, 1), fill, dtype=np.uint8)
    counts = (C.c_uint64 * 3)(7, 7, 7)
    rc = sim.lib.lfa_sample_velocity_collective(sim.h, ptr(pts), len(pts), ptr(idx), ptr(vel), ptr(typ), capacity, C.byref(counts))
    return rc, idx, vel, typ, tuple(int(c) for c in counts)


def check_state(sims, bounds, what):
    """Every assertion of this file that holds in each state; the calls under test come before the downloads."""
    nr = len(sims)
    own = ss.owner(POINTS, bounds)
    got = collective(sims, lambda r, s: s.sample_velocity_collective(POINTS, types=True))
    again = collective(sims, lambda r, s: s.sample_velocity_collective(POINTS, types=True))
    grid = ss.stitch([s.cells() for s in sims], bounds)
    want_vel, want_types, want_out = sc.model(grid, POINTS)
    assert want_out == 10
    for r, (idx, vel, typ, counts) in enumerate(got):
        mine = np.flatnonzero(own == r)
        bad = np.flatnonzero((vel.view(np.uint64) != want_vel[idx].view(np.uint64)).any(axis=1)) if len(idx) == len(mine) else []
        print(what, bounds, "rank", r, "counts", counts, "model owns", len(mine), "rows that differ", len(bad))
        assert idx.dtype == np.uint32 and (np.diff(idx.astype(np.int64)) > 0).all(), (what, r)
        assert np.array_equal(idx, mine), (what, r)
        assert vel.tobytes() == want_vel[mine].tobytes(), (what, r, bad[:8], vel[bad[:4]], want_vel[mine][bad[:4]])
        assert typ.tobytes() == want_types[mine].tobytes(), (what, r)
        assert counts == (len(mine), 10, N - 10 - len(mine)) and sum(counts) == N, (what, r, counts)
        for a, b in zip(got[r][:3], again[r][:3]):
            assert a.tobytes() == b.tobytes(), (what, r)
        assert again[r][3] == counts
    union = np.concatenate([g[0] for g in got])
    assert len(union) == len(set(union.tolist())) and np.array_equal(np.sort(union), np.flatnonzero(INSIDE)), what
    # the grid the ranks show is what it was: the refresh writes ghost layers only
    assert ss.stitch([s.cells() for s in sims], bounds).tobytes() == grid.tobytes(), what

    # rank-specific lists: rank r passes every nr-th point from r on, the last rank an empty list
    lists = [np.arange(r, N, nr) for r in range(nr)]
    lists[-1] = np.zeros(0, dtype=np.int64)
    part = collective(sims, lambda r, s: s.sample_velocity_collective(POINTS[lists[r]], types=True))
    for r, (idx, vel, typ, counts) in enumerate(part):
        where = lists[r][idx]
        assert np.array_equal(idx, np.flatnonzero(own[lists[r]] == r)), (what, r)
        assert vel.tobytes() == want_vel[where].tobytes() and typ.tobytes() == want_types[where].tobytes(), (what, r)
        assert counts == (len(idx), int((own[lists[r]] < 0).sum()), len(lists[r]) - len(idx) - int((own[lists[r]] < 0).sum())), (what, r)
    assert part[-1][3] == (0, 0, 0) and len(part[-1][0]) == 0

    # a short capacity on rank 0 alone: LFA_E_INVALID there, counts filled, nothing else written; the peers' results are intact
    n0 = int((own == 0).sum())
    assert n0 > 1
    short = collective(sims, lambda r, s: raw_call(s, POINTS, n0 - 1) if r == 0 else s.sample_velocity_collective(POINTS, types=True))
    rc, idx, vel, typ, counts = short[0]
    assert rc == E_INVALID and counts == (n0, 10, N - 10 - n0), (what, rc, counts)
    assert "owns" in sims[0].lib.lfa_last_error(sims[0].h).decode()
    assert (idx == 0xA5A5A5A5).all() and (typ == 0xA5).all() and vel.tobytes() == b"\xa5" * vel.nbytes, what
    for r in range(1, nr):
        for a, b in zip(short[r][:3], got[r][:3]):
            assert a.tobytes() == b.tobytes(), (what, r)
    # an exact fit is a new collective call and succeeds
    fit = collective(sims, lambda r, s: raw_call(s, POINTS, n0) if r == 0 else s.sample_velocity_collective(POINTS))
    rc, idx, vel, typ, counts = fit[0]
    assert rc == 0 and counts[0] == n0 and idx[:n0].tobytes() == got[0][0].tobytes() and vel[:3 * n0].tobytes() == got[0][1].tobytes()
    assert typ[:n0].tobytes() == got[0][2].tobytes()
    # the plain call still refuses a handle with a transport, before anything is touched
    with pytest.raises(lfa.LibfluidError) as e:
        sims[0].sample_velocity(POINTS[:4])
    assert e.value.code == E_UNSUPPORTED
    return grid


@pytest.mark.parametrize("bounds", ss.BOUNDS, ids=str)
def test_uploaded_grid_on_binned_handles(bounds):
    """(a): every tile of every rank is explicit (stored values, background 0): the ghost layers carry whole tile layers."""
    field = sc.random_field()
    hub, sims = make_slabs(GRID, bounds, **KW)
    for s in sims:
        s.upload_particles(sc.sparse_particles())
    collective(sims, lambda r, s: s.hash())
    for s in sims:
        s.upload_cells(field)
    grid = check_state(sims, bounds, "uploaded")
    close_all(hub, sims)
    # the values are fp32-representable: the upload itself is the grid
    assert grid["vel"].tobytes() == field["vel"].tobytes() and grid["type"].tobytes() == field["type"].tobytes()


@pytest.mark.parametrize("bounds", ss.BOUNDS, ids=str)
def test_p2g_then_steps_then_a_collective_seed(bounds):
    """(b), (c), (d) on the same handles."""
    hub, sims = make_slabs(GRID, bounds, **KW)
    parts = ss.slab_particles()
    for s in sims:
        s.upload_particles(parts)

    def p2g(r, s):
        s.hash()
        s.p2g()
        s.add_gravity(sc.DT)

    collective(sims, p2g)
    grid = check_state(sims, bounds, "hash + p2g + gravity")
    g_dt = np.array(sc.GRAVITY) * sc.DT
    vel = grid["vel"].reshape(sc.SIZE[2], sc.SIZE[1], sc.SIZE[0], 3)
    assert (vel[16:, 16:, :8] == g_dt).all() and np.abs(vel[:8, :8, :8] - g_dt).max() > 0.0  # implicit and explicit tiles

    def steps(r, s):
        for _ in range(2):
            assert s.time_step(sc.DT)[2] >= 0

    collective(sims, steps)
    check_state(sims, bounds, "two steps")

    # (d) every rank makes the seeding call; only the rank of tile layer 1 keeps particles, and its grid stops being "valid"
    kept = [s.seed_box(*ss.SEED_BOX, density=2, rng_state=42, flags=lfa.SEED_COLLECTIVE)[0] for s in sims]
    layer_owner = int(np.searchsorted(np.asarray(bounds), ss.SEED_TILE[2], side="right") - 1)
    assert kept[layer_owner] > 0 and sum(kept) == kept[layer_owner], kept
    collective(sims, lambda r, s: s.hash())
    grid = check_state(sims, bounds, "steps + collective seed + hash")
    close_all(hub, sims)


def test_unbinned_handles_refuse_on_every_rank_without_a_message():
    bounds = [0, 1, 2, 3]
    hub, sims = make_slabs(GRID, bounds, **KW)
    for s in sims:
        s.upload_particles(sc.sparse_particles())
    # one rank after the other on this thread: a call that sent a message would wait for its peers here
    for s in sims:
        with pytest.raises(lfa.LibfluidError) as e:
            s.sample_velocity_collective(POINTS)
        assert e.value.code == E_INVALID and "lfa_hash_particles" in str(e.value)
        assert e.value.counts == (0, 0, 0)
    collective(sims, lambda r, s: s.hash())
    got = collective(sims, lambda r, s: s.sample_velocity_collective(POINTS))
    assert sum(len(g[0]) for g in got) == int(INSIDE.sum())
    # this rank's own argument errors come after the refresh: the peers complete
    def bad_args(r, s):
        if r == 1:
            counts = (C.c_uint64 * 3)(7, 7, 7)
            vel = np.zeros(3 * N)
            rc = s.lib.lfa_sample_velocity_collective(s.h, ptr(POINTS), N, None, ptr(vel), None, N, C.byref(counts))
            return rc, tuple(counts)
        return s.sample_velocity_collective(POINTS)

    out = collective(sims, bad_args)
    assert out[1] == (E_INVALID, (0, 0, 0))
    for r in (0, 2):
        assert out[r][0].tobytes() == got[r][0].tobytes() and out[r][1].tobytes() == got[r][1].tobytes()
    close_all(hub, sims)


def test_a_single_domain_answers_like_the_plain_call():
    sim = lfa.Sim(**GRID, **KW)
    sim.upload_particles(ss.slab_particles())
    for state in ("unbinned", "stepped"):
        if state == "stepped":
            for _ in range(2):
                sim.time_step(sc.DT)
        vel, types, n_out = sim.sample_velocity(POINTS, types=True)
        idx, cvel, ctypes_, counts = sim.sample_velocity_collective(POINTS, types=True)
        assert np.array_equal(idx, np.flatnonzero(INSIDE)), state
        assert cvel.tobytes() == vel[INSIDE].tobytes() and ctypes_.tobytes() == types[INSIDE].tobytes(), state
        assert counts == (int(INSIDE.sum()), 10, 0) and n_out == 10
        assert sim.sample_velocity_ms() >= 0.0
        for n in (0, 1, 63, 64, 65, 257):
            sub = np.concatenate([POINTS[-14:], POINTS])[:n]
            i2, v2, c2 = sim.sample_velocity_collective(sub)
            keep = sc.classify(sub)[1] if n else np.zeros(0, dtype=bool)
            assert np.array_equal(i2, np.flatnonzero(keep)) and v2.tobytes() == sim.sample_velocity(sub)[0][keep].tobytes(), (state, n)
            assert c2 == (int(keep.sum()), n - int(keep.sum()), 0)
    sim.close()
