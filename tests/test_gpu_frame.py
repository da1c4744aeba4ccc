"""lfa_frame_stats / lfa_download_positions on the device against tests/frame_model.py applied to an LFA_DL_POSITIONS download of
the same handle: the occupation grid, the counts, the maximum, the box and the positions exactly; the two sums within the bound of
two summation orders of the same terms (frame_model.energy_bound, from the model's own energy_abs).

The grid is ragged in z and sits at an offset and a cell size that are no powers of two, so that the cell of a reconstructed
position can differ from the cell of the particle's key (tests/test_frame_model.py shows the arithmetic); the clouds put particles
on cell faces and one ulp either side of them, and crowd one cell so that the counting atomics contend.

A particle shows the difference only if the upload leaves it with key c and a fraction of (nearly) 0 in a cell whose face
off + c h divides back to just below c. Whether a double exists that the ingest's split (cell_and_fraction: fp64 division,
truncation) sends there depends on the offset: a search on the CPU over the faces of this grid and one ulp either side finds none
for an x offset of 0.7, nor for any offset near -0.35 or 15.3 at this cell size; for 0.69 the double one ulp above the face of
x cell 12 is one (key cell 12, occupation cell 11). Hence the x offset, and REACH particles uploaded exactly there."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from libfluid_amd import scenes
from tests import frame_model as fm

pytestmark = pytest.mark.gpu

SIZE = (24, 16, 9)
OFFSET = (0.69, -0.35, 15.3)
H = 0.3
GRAVITY = (0.3, -981.0, 0.1)
SIZES = [0, 1, 63, 64, 65, 257, 5000, 300000]
REACH = 24  # particles (clouds of 257 and more) on the x position whose key cell is 12 and whose occupation cell is 11
DT = 0.005
E_INVALID = -1


def make_sim(**kw):
    return lfa.Sim(SIZE, cell_size=H, offset=OFFSET, gravity=GRAVITY, **kw)


def cloud(n, seed=7):
    """n records: up to 96 in one cell, REACH on the reachable mismatch (see above), then a third on cell faces (exactly off + c h,
    and one ulp below / above), the rest jittered over the grid; random velocities."""
    rng = np.random.default_rng(seed)
    off, size = np.asarray(OFFSET), np.asarray(SIZE)
    pos = np.empty((n, 3))
    crowd = min(n, 96)
    pos[:crowd] = off + (np.array([5.0, 3.0, 2.0]) + 0.25 + 0.5 * rng.random((crowd, 3))) * H
    reach = REACH if n >= 257 else 0
    pos[crowd:crowd + reach] = off + rng.random((reach, 3)) * size * H
    pos[crowd:crowd + reach, 0] = np.nextafter(off[0] + 12.0 * H, np.inf)
    crowd += reach
    faces = (n - crowd) // 3
    c = rng.integers(0, size, size=(faces, 3)).astype(np.float64)
    on = off + c * H
    nudge = rng.integers(-1, 2, size=(faces, 3))
    on = np.where(nudge < 0, np.nextafter(on, -np.inf), np.where(nudge > 0, np.nextafter(on, np.inf), on))
    pos[crowd:crowd + faces] = on
    rest = n - crowd - faces
    pos[crowd + faces:] = off + rng.random((rest, 3)) * size * H
    parts = np.zeros(n, dtype=lfa.PARTICLE_DTYPE)
    parts["pos"] = pos
    parts["old_pos"] = pos
    parts["vel"] = rng.normal(size=(n, 3)) * 3.0
    return parts


def key_cells(parts):
    raw = parts["raw"].astype(np.int64)
    return np.stack([raw % SIZE[0], (raw // SIZE[0]) % SIZE[1], raw // (SIZE[0] * SIZE[1])], axis=1)


def stats_bytes(st):
    return bytes(memoryview(st))


def check(sim, what, energy=True):
    """Every comparison of this file, in whatever state the handle is in. The summary is taken BEFORE the download, so that it is
    the call under test that meets the state. Returns (download, model)."""
    st, occ = sim.frame_stats()
    pos = sim.positions()
    st2, occ2 = sim.frame_stats()
    st3, none = sim.frame_stats(occupation=False)
    d = sim.download_particles(write_positions=True)
    m = fm.summary(d, SIZE, OFFSET, H, GRAVITY)
    n = len(d)
    print(what, "n", n, "in grid", st.n_in_grid, "energy", st.energy, "model", m["energy"], "abs", st.energy_abs, "model", m["energy_abs"],
          "bound", fm.energy_bound(n, m["energy_abs"]), "max", st.max_speed2)
    assert st.n == m["n"] == sim.num_particles, what
    assert st.n_in_grid == m["n_in_grid"] == int(occ.sum(dtype=np.uint64)), what
    assert occ.dtype == np.uint32 and np.array_equal(occ, m["occupation"]), what
    assert st.max_speed2 == m["max_speed2"], what
    assert np.array_equal(np.array(st.lo), m["lo"]) and np.array_equal(np.array(st.hi), m["hi"]), what
    assert pos.shape == (n, 3) and pos.tobytes() == np.ascontiguousarray(d["pos"]).tobytes(), what
    if energy:
        bound = fm.energy_bound(n, m["energy_abs"])
        assert abs(st.energy - m["energy"]) <= bound, (what, st.energy, m["energy"], bound)
        assert abs(st.energy_abs - m["energy_abs"]) <= bound, (what, st.energy_abs, m["energy_abs"], bound)
    # two calls on the same resident state: the same bits; without the grid: the same scalars
    assert stats_bytes(st) == stats_bytes(st2) and np.array_equal(occ, occ2), what
    assert stats_bytes(st) == stats_bytes(st3) and none is None, what
    return d, m


@pytest.mark.parametrize("n", SIZES)
def test_sizes_unbinned_and_binned(n):
    sim = make_sim()
    sim.upload_particles(cloud(n))
    d, m = check(sim, f"n={n} after the upload")
    if n >= 257:
        # the inputs are what they are meant to be: cells that differ from the key's, and a cell the atomics contend on
        differ = (fm.cells(d["pos"], OFFSET, H) != key_cells(d)).any(axis=1).sum()
        print("particles whose occupation cell is not the key's cell:", differ, "fullest cell:", m["occupation"].max())
        assert differ >= 16
        assert m["occupation"].max() >= 64
    if n == 0:
        st, occ = sim.frame_stats()
        assert (st.n, st.n_in_grid, st.energy, st.energy_abs, st.max_speed2) == (0, 0, 0.0, 0.0, 0.0) and not occ.any()
        assert np.isposinf(np.array(st.lo)).all() and np.isneginf(np.array(st.hi)).all()
    sim.hash()
    check(sim, f"n={n} after lfa_hash_particles")
    sim.close()


def test_nan_velocity_is_skipped_by_the_maximum():
    parts = cloud(300)
    parts["vel"][7] = [np.nan, 1.0, 1.0]
    parts["vel"][11] = [50.0, 0.0, 0.0]
    sim = make_sim()
    sim.upload_particles(parts)
    d, m = check(sim, "a NaN velocity", energy=False)
    st, _ = sim.frame_stats()
    assert st.max_speed2 == 2500.0 and np.isnan(st.energy) and np.isnan(d["vel"][7, 0])
    sim.close()


def dam(method):
    sim = make_sim(method=method, blending=0.95)
    sim.upload_particles(scenes.seed_block((0, 0, 0), (8, 10, 6), cell_size=H, offset=OFFSET))
    return sim


@pytest.mark.parametrize("name", ["flip", "apic"])
def test_after_time_steps_and_between_advect_and_collide(name):
    """FLIP parks C in its home array and defers v through the binning, APIC defers v and C; lfa_time_step leaves the correction
    on its second stream. Then the split stages: between lfa_advect and lfa_collide the summary is of the moved positions."""
    sim = dam(lfa.FLIP_BLEND if name == "flip" else lfa.APIC)
    for k in range(3):
        assert sim.time_step(DT)[2] >= 0
        check(sim, f"{name} after time step {k + 1}")
    sim.advect(DT)
    d, _ = check(sim, f"{name} between lfa_advect and lfa_collide")
    assert not np.array_equal(d["pos"], d["old_pos"])  # the state is the one meant: old_position is of before the move
    sim.collide()
    check(sim, f"{name} after lfa_collide")
    sim.close()


def test_after_a_sphere_seeded_behind_resident_particles():
    sim = make_sim()
    sim.upload_particles(cloud(257))
    sim.hash()
    centre = np.asarray(OFFSET) + np.array([12.0, 8.0, 4.5]) * H
    seeded, _, _ = sim.seed_sphere(centre, 3.2 * H, velocity=(0.5, -2.0, 0.25), density=2)
    assert seeded > 0 and sim.num_particles == 257 + seeded
    check(sim, "after lfa_seed_sphere")
    sim.close()


def test_the_calls_change_nothing_a_step_reads():
    """(a) downloads before and after the calls, no step between them: identical, in the state lfa_time_step leaves and between
    lfa_advect and lfa_collide. (b) two handles with the same input take the same steps, one of them queried after every step:
    the full step is not bit-reproducible from run to run, so iteration counts and the CFL are held to the bars
    tests/test_gpu_parity.py holds two computations of one step to (one iteration; 1e-4 of the largest speed)."""
    a, b = dam(lfa.APIC), dam(lfa.APIC)
    for k in range(3):
        ra, rb = a.time_step(DT), b.time_step(DT)
        before = b.download_particles(write_positions=True)
        b.frame_stats()
        b.positions()
        b.frame_stats(occupation=False)
        assert b.download_particles(write_positions=True).tobytes() == before.tobytes(), k
        assert ra[2] >= 0 and rb[2] >= 0 and abs(ra[1] - rb[1]) <= 1, (k, ra, rb)
        va, vb = H / a.cfl(), H / b.cfl()
        assert abs(va - vb) <= 1e-4 * va + 1e-5 * 981.0 * DT, (k, va, vb)
    b.advect(DT)
    before = b.download_particles(write_positions=True)
    b.frame_stats()
    b.positions()
    assert b.download_particles(write_positions=True).tobytes() == before.tobytes()
    b.collide()
    a.advect_collide(DT)
    assert a.num_particles == b.num_particles
    a.close()
    b.close()


def test_errors_leave_the_buffers_untouched():
    lib = lfa.load_library()
    ncells = SIZE[0] * SIZE[1] * SIZE[2]
    st = lfa.FrameStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    mark = stats_bytes(st)
    occ = np.full(ncells, 0xDEADBEEF, dtype=np.uint32)
    # cell_size unset: a handle straight from lfa_create
    h = C.c_void_p()
    assert lib.lfa_create(C.byref(h), *SIZE, -1) == 0
    assert lib.lfa_frame_stats(h, C.byref(st), occ.ctypes.data_as(C.c_void_p)) == E_INVALID
    assert b"cell_size" in lib.lfa_last_error(h)
    xyz = np.full(3, 123.0)
    assert lib.lfa_download_positions(h, xyz.ctypes.data_as(C.c_void_p), 1) == E_INVALID
    ms = C.c_double(-1.0)
    assert lib.lfa_frame_stats_time(h, C.byref(ms)) == E_INVALID and ms.value == -1.0
    lib.lfa_destroy(h)
    assert stats_bytes(st) == mark and (occ == 0xDEADBEEF).all() and (xyz == 123.0).all()
    # NULL out; a wrong n for the positions
    sim = make_sim()
    sim.upload_particles(cloud(65))
    assert lib.lfa_frame_stats(sim.h, None, occ.ctypes.data_as(C.c_void_p)) == E_INVALID
    assert b"NULL" in lib.lfa_last_error(sim.h) and (occ == 0xDEADBEEF).all()
    for n in (64, 66):
        buf = np.full((66, 3), 123.0)
        assert lib.lfa_download_positions(sim.h, buf.ctypes.data_as(C.c_void_p), n) == E_INVALID
        assert b"65" in lib.lfa_last_error(sim.h) and (buf == 123.0).all()
    # and the handle is as usable as before
    check(sim, "after the refused calls")
    assert sim.frame_stats_ms() > 0.0
    sim.close()
