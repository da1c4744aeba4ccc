"""lfa_mesher_vertex_velocities_collective on virtual slabs: every rank meshes its own cell layers from its slab handle (the set-up of
tests/test_gpu_slabs.py: test_slab_ranks_mesh_their_windows_into_the_single_domain_mesh) and asks for the velocities of its
vertices. The bar: the bytes of lfa_sample_velocity_collective - which tests/test_gpu_sample_slabs.py pins to the oracle on the
stitched grid - at the downloaded vertex positions, every rank passing the same list and the ranks' compact answers put together.

A window's vertices on its top plane lie in the cell layer of the rank above: the mesher call answers by reach, not by ownership,
so with the windows [8 lo, min(8 hi, nz)) no vertex is left out. A whole-grid mesher on two slabs shows the other side: vertices
beyond a rank's reach are +0.0 in every bit and counted."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import sample_slab_cases as ss
from tests import util
from tests.test_gpu_seed_slabs import close_all, collective

pytestmark = pytest.mark.gpu

SIZE, BLOCK = (16, 16, 32), ((2, 0, 3), (14, 10, 29))
# the testbed's mesher parameters (tests/test_gpu_mesher_velocities.py). With particle_extent 1 and cell_radius 2, the parameters of
# the test this set-up is taken from, most grid points next to the surface see no particle, the reference's function is NaN there
# and so are nine vertex positions in ten - outside points for the sampling, which this test is not about
MKW = dict(size=SIZE, grid_offset=(0.0, 0.0, 0.0), cell_size=1.0, particle_extent=2.0, cell_radius=3)
E_INVALID = -1


def stepped_slabs(bounds):
    n = len(bounds) - 1
    hub = lfa.LocalHub(n)
    sims = []
    for r in range(n):
        t = lfa.Sim(SIZE, method=lfa.APIC)
        t.init_local_slab(hub.h, r, bounds)
        t.seed_block(*BLOCK)
        sims.append(t)

    def run(r, s):
        for _ in range(2):
            assert s.time_step(util.DT)[2] >= 0
        s.hash()

    collective(sims, run)
    return hub, sims


def in_box(pos):
    """The inside test of the sampling on this grid (cell size 1, offset 0: the division is exact); false for a NaN position - the
    mesher interpolates towards grid points no particle reaches, as the reference's does."""
    with np.errstate(invalid="ignore"):
        return ((pos >= 0.0) & (pos < np.array(SIZE, dtype=np.float64))).all(axis=1)


def union_answer(sims, pos):
    """sample_velocity_collective with the same list on every rank: (velocity[n, 3] put together from the ranks' rows, +0.0 where
    no rank answered; answered[n])."""
    got = collective(sims, lambda r, s: s.sample_velocity_collective(pos))
    vel, hit = np.zeros((len(pos), 3)), np.zeros(len(pos), dtype=np.int64)
    for idx, v, counts in got:
        vel[idx] = v
        hit[idx] += 1
        assert counts[1] == int((~in_box(pos)).sum())
    assert hit.max(initial=0) <= 1
    return vel, hit == 1


@pytest.mark.parametrize("bounds", [[0, 2, 4], [0, 1, 2, 4], [0, 1, 2, 3, 4]], ids=str)
def test_windows_get_the_union_answer_at_their_vertices(bounds):
    hub, sims = stepped_slabs(bounds)

    def mesh(r, s):
        lo, hi = s.slab()
        m = lfa.Mesher(window=(lo * 8, min(hi * 8, SIZE[2])), **MKW)
        m.sample_sim(s, 0.5)
        pos, _ = m.marching_cubes()
        vel, counts = m.vertex_velocities_collective(s)
        again, counts2 = m.vertex_velocities_collective(s)
        return m, pos, vel, counts, again, counts2

    meshes = collective(sims, mesh)
    n_top = 0
    for r, (m, pos, vel, counts, again, counts2) in enumerate(meshes):
        want, answered = union_answer(sims, pos)
        print(bounds, "rank", r, "vertices", len(pos), "counts", counts)
        inside = in_box(pos)
        assert int(inside.sum()) > 100 and np.array_equal(answered, inside)
        assert counts == (int((~inside).sum()), 0) and counts2 == counts, (r, counts)  # nothing is beyond the rank's reach
        assert not vel[~inside].any() and not np.signbit(vel[~inside]).any()
        assert vel.tobytes() == want.tobytes(), r
        assert again.tobytes() == vel.tobytes()
        assert np.abs(vel).max() > 0.0
        lo, hi = ss.window(bounds, r)
        if r + 2 < len(bounds):
            n_top += int((inside & (pos[:, 2] >= hi)).sum())  # vertices whose cell belongs to the rank above
        ms = m.velocities_ms()
        assert ms >= 0.0
    assert n_top > 0, "some vertex of a window's top plane is meant to lie in the cell layer of the rank above"

    # stale where the normals are: a new sample needs marching_cubes AND the velocities again (sample_sim on a slab handle is a
    # collective itself: every rank makes it)
    def stale(r, s):
        m, vel = meshes[r][0], meshes[r][2]
        buf, ms = np.empty_like(vel), C.c_double()
        m.sample_sim(s, 0.5)
        codes = [m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p))]
        m.marching_cubes()
        codes.append(m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)))
        codes.append(m.lib.lfa_mesher_velocities_time(m.h, C.byref(ms)))
        # the plain call still refuses the slab handle, and leaves the state as it is
        codes.append(m.lib.lfa_mesher_vertex_velocities(m.h, s.h, None))
        codes.append(m.lib.lfa_mesher_download_velocities(m.h, buf.ctypes.data_as(C.c_void_p)))
        return codes

    for codes in collective(sims, stale):
        assert codes == [E_INVALID, E_INVALID, E_INVALID, -6, E_INVALID], codes

    def redo(r, s):
        return meshes[r][0].vertex_velocities_collective(s)

    for r, (v, counts) in enumerate(collective(sims, redo)):
        assert v.tobytes() == meshes[r][2].tobytes() and counts == meshes[r][3]
    for m, *_ in meshes:
        m.close()
    close_all(hub, sims)


def test_vertices_beyond_reach_are_zero_and_counted():
    bounds = [0, 2, 4]
    hub, sims = stepped_slabs(bounds)
    # a tilted plane z = 1.37 + 1.8 x + 0.03 y: its vertices span the cell layers 1 .. 30
    z, y, x = np.meshgrid(np.arange(SIZE[2] + 1.0), np.arange(SIZE[1] + 1.0), np.arange(SIZE[0] + 1.0), indexing="ij")
    values = z - (1.37 + 1.8 * x + 0.03 * y)

    def mesh(r, s):
        m = lfa.Mesher(**MKW)
        m.set_values(values)
        pos, _ = m.marching_cubes()
        vel, counts = m.vertex_velocities_collective(s)
        return m, pos, vel, counts

    meshes = collective(sims, mesh)
    pos = meshes[0][1]
    assert meshes[1][1].tobytes() == pos.tobytes() and len(pos) > 500
    assert np.isfinite(pos).all()
    cz = np.floor(pos[:, 2]).astype(np.int64)  # (cell size 1, offset 0: the division is exact)
    inside = in_box(pos)
    assert cz.min() <= 2 and cz.max() >= 29
    want, answered = union_answer(sims, pos)
    assert np.array_equal(answered, inside)
    for r, (m, _, vel, counts) in enumerate(meshes):
        lo, hi = ss.reach(bounds, r, SIZE[2])
        reached = inside & (cz >= lo) & (cz < hi)
        print("rank", r, "reach", (lo, hi), "vertices", len(pos), "counts", counts, "model beyond reach", int((inside & ~reached).sum()))
        assert counts == (int((~inside).sum()), int((inside & ~reached).sum())) and counts[1] > 0
        assert vel[reached].tobytes() == want[reached].tobytes()
        assert vel[~reached].tobytes() == np.zeros((int((~reached).sum()), 3)).tobytes()  # +0.0 in every bit
        assert np.abs(vel[reached]).max() > 0.0
        m.close()
    close_all(hub, sims)


def test_a_single_domain_call_equals_the_plain_one():
    sim = lfa.Sim(SIZE, method=lfa.APIC)
    sim.seed_block(*BLOCK)
    for _ in range(2):
        sim.time_step(util.DT)
    m = lfa.Mesher(**MKW)
    m.sample_sim(sim, 0.5)
    m.marching_cubes()
    vel, n_out = m.vertex_velocities(sim)
    cvel, counts = m.vertex_velocities_collective(sim)
    assert cvel.tobytes() == vel.tobytes() and counts == (n_out, 0) and np.abs(vel).max() > 0.0
    m.close()
    sim.close()
