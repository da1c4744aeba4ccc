"""lfa_mesher_vertex_velocities: one velocity per vertex of the mesher's surface, sampled on the device from the vertex positions it
already holds. The bar: the bytes of Sim.sample_velocity (tests/test_gpu_sample.py pins that to the oracle) on the downloaded vertex
positions, outside count included - on the simulation's own grid, on a shifted mesher grid whose vertices partly leave the
simulation's box, on z-windows, after a rebase; and the state rules (stale after a new sample, an empty mesh is fine)."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from libfluid_amd import scenes

pytestmark = pytest.mark.gpu

SIZE = (24, 24, 24)
DT = 0.01
R = 0.5
E_INVALID = -1


@pytest.fixture(scope="module")
def sim():
    s = lfa.Sim(SIZE, method=lfa.APIC)
    s.upload_particles(scenes.seed_block((0, 0, 0), (10, 14, 12)))
    for _ in range(3):
        s.time_step(DT)
    yield s
    s.close()


def mesher(offset=(0.0, 0.0, 0.0), window=None, size=SIZE):
    return lfa.Mesher(size, grid_offset=offset, cell_size=1.0, particle_extent=2.0, cell_radius=3, window=window)  # (the testbed's)


def test_vertex_velocities_equal_the_sample_at_the_downloaded_vertices(sim):
    m = mesher()
    m.sample_sim(sim, R)
    pos, idx = m.marching_cubes()
    assert len(pos) > 500 and np.isfinite(pos).all()
    vel, n_out = m.vertex_velocities(sim)
    want, want_out = sim.sample_velocity(pos)
    assert vel.tobytes() == want.tobytes() and n_out == want_out
    assert np.abs(vel).max() > 0.0
    assert m.velocities_ms() >= 0.0
    # a second request: the same bytes
    again, n_again = m.vertex_velocities(sim)
    assert again.tobytes() == vel.tobytes() and n_again == n_out
    # rebasing the indices changes nothing
    m.rebase(12345)
    rebased, n_rebased = m.vertex_velocities(sim)
    assert rebased.tobytes() == vel.tobytes() and n_rebased == n_out
    out = np.empty_like(vel)
    assert m.lib.lfa_mesher_download_velocities(m.h, out.ctypes.data_as(C.c_void_p)) == 0 and out.tobytes() == vel.tobytes()
    m.close()


def test_a_shifted_mesher_grid_leaves_the_simulations_box(sim):
    m = mesher(offset=(-2.5, -2.5, -2.5))
    m.sample_sim(sim, R)
    pos, idx = m.marching_cubes()
    vel, n_out = m.vertex_velocities(sim)
    want, want_out = sim.sample_velocity(pos)
    assert vel.tobytes() == want.tobytes() and n_out == want_out
    outside = ~((pos >= 0.0) & (pos / 1.0 < np.array(SIZE, dtype=np.float64))).all(axis=1)
    print("vertices", len(pos), "outside", n_out)
    assert n_out == int(outside.sum()) > 0
    assert vel[outside].tobytes() == np.zeros((int(outside.sum()), 3)).tobytes()  # +0.0, every bit
    assert np.abs(vel[~outside]).max() > 0.0
    m.close()


def test_two_windows_concatenated_are_the_whole_grid(sim):
    whole = mesher()
    whole.sample_sim(sim, R)
    pos, _ = whole.marching_cubes()
    want, want_out = whole.vertex_velocities(sim)
    cut = 6
    parts, n_out = [], 0
    windows = [mesher(window=(0, cut)), mesher(window=(cut, SIZE[2]))]
    for w in windows:
        w.sample_sim(sim, R)
        wpos, _ = w.marching_cubes()
        v, k = w.vertex_velocities(sim)
        assert v.tobytes() == sim.sample_velocity(wpos)[0].tobytes()
        parts.append(v)
        n_out += k
    assert all(len(p) for p in parts)
    assert np.concatenate(parts).tobytes() == want.tobytes() and n_out == want_out
    for w in windows:
        w.close()
    whole.close()


def test_velocities_go_stale_where_normals_do_and_an_empty_mesh_is_fine(sim):
    m = mesher()
    buf = np.empty((4, 3))
    ms = C.c_double(0.0)
    # no mesh yet
    assert m.lib.lfa_mesher_vertex_velocities(m.h, sim.h, None) == E_INVALID
    m.sample_sim(sim, R)
    assert m.lib.lfa_mesher_vertex_velocities(m.h, sim.h, None) == E_INVALID
    pos, _ = m.marching_cubes()
    assert m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)) == E_INVALID  # none computed for this mesh
    assert m.lib.lfa_mesher_velocities_time(m.h, C.byref(ms)) == E_INVALID
    vel, _ = m.vertex_velocities(sim)
    # a new sample: stale until marching_cubes AND vertex_velocities have run again
    m.sample_sim(sim, R)
    assert m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)) == E_INVALID
    m.marching_cubes()
    assert m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)) == E_INVALID
    again, _ = m.vertex_velocities(sim)
    assert again.tobytes() == vel.tobytes()
    # an upload of values does the same
    m.set_values(np.full((SIZE[2] + 1, SIZE[1] + 1, SIZE[0] + 1), 1.0))
    assert m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)) == E_INVALID
    # an empty mesh is LFA_OK
    pos, idx = m.marching_cubes()
    assert len(pos) == 0 and len(idx) == 0
    n_out = C.c_uint64(7)
    assert m.lib.lfa_mesher_vertex_velocities(m.h, sim.h, C.byref(n_out)) == 0 and n_out.value == 0
    assert m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)) == 0
    empty, k = m.vertex_velocities(sim)
    assert empty.shape == (0, 3) and k == 0
    m.close()
