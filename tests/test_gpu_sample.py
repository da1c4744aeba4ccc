"""lfa_sample_velocity on the device against tests/sample_cases.py's model (the oracle's PIC grid-to-particle transfer, which
tests/test_sample_cases.py pins to the compiled reference) on a download of the same handle: velocity bytes, type bytes and the
outside count equal, tolerance 0. Every operation is an IEEE fp64 operation in a fixed order, so a differing bit is a bug:
contraction, reassociation, a float fraction, or a second copy of the rule for a cell's value.

The states cover the three branches of that rule (common.h: CellView): an uploaded grid (stored + bg with bg = 0), the same after
gravity (bg != 0), a sparse P2G whose implicit tiles hold bg alone next to explicit ones, and stepped simulations."""
import ctypes as C

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import sample_cases as sc

pytestmark = pytest.mark.gpu

POINTS = sc.points()


def make_sim(**kw):
    kw.setdefault("method", lfa.PIC)
    return lfa.Sim(sc.SIZE, cell_size=sc.H, offset=sc.OFFSET, gravity=sc.GRAVITY, **kw)


def check(sim, what, points=POINTS):
    """Every comparison of this file, in whatever state the handle is in; the sample is taken BEFORE the download, so that it is the
    call under test that meets the state. Returns the downloaded grid."""
    n_parts = sim.num_particles
    parts_before = sim.download_particles(write_positions=True) if n_parts else None
    cells_before = sim.cells()
    vel, types, n_out = sim.sample_velocity(points, types=True)
    vel2, types2, n_out2 = sim.sample_velocity(points, types=True)
    cells = sim.cells()
    want_vel, want_types, want_out = sc.model(cells, points)
    bad = np.flatnonzero((vel.view(np.uint64) != want_vel.view(np.uint64)).any(axis=1))
    print(what, "points", len(points), "outside", n_out, "model", want_out, "rows that differ", len(bad),
          "max |diff|", float(np.nanmax(np.abs(vel - want_vel))) if len(points) else 0.0)
    assert vel.tobytes() == want_vel.tobytes(), (what, bad[:8], vel[bad[:4]], want_vel[bad[:4]])
    assert types.tobytes() == want_types.tobytes(), what
    assert n_out == want_out, what
    assert vel2.tobytes() == vel.tobytes() and types2.tobytes() == types.tobytes() and n_out2 == n_out, what
    # the call changes nothing
    assert cells.tobytes() == cells_before.tobytes(), what
    if n_parts:
        assert sim.download_particles(write_positions=True).tobytes() == parts_before.tobytes(), what
    return cells


def test_uploaded_grid():
    field = sc.random_field()
    sim = make_sim()
    check(sim, "fresh handle")
    sim.upload_cells(field)
    check(sim, "uploaded")
    # the values are fp32-representable: the upload itself is the grid, which pins the sample without lfa_download_cells
    vel, types, n_out = sim.sample_velocity(POINTS, types=True)
    want = sc.model(field, POINTS)
    assert vel.tobytes() == want[0].tobytes() and types.tobytes() == want[1].tobytes() and n_out == want[2] == 10
    inside = sc.classify(POINTS)[1]
    assert not vel[~inside].any() and not np.signbit(vel[~inside]).any() and not types[~inside].any()
    assert np.abs(vel[inside]).max() > 1.0
    sim.close()


def test_upload_then_gravity_adds_the_background():
    sim = make_sim()
    sim.upload_cells(sc.random_field())
    sim.upload_particles(sc.sparse_particles())
    sim.hash()
    sim.add_gravity(sc.DT)
    cells = check(sim, "upload + hash + gravity")
    # (the branch under test: a cell outside the dilated set - tile (0, 2, 2), far from both blobs - is the upload plus g dt in fp64)
    far = 0 + sc.SIZE[0] * (sc.SIZE[1] - 1 + sc.SIZE[1] * (sc.SIZE[2] - 1))
    assert cells["vel"][far, 1] == sc.random_field()["vel"][far, 1] + sc.GRAVITY[1] * sc.DT
    sim.close()


def test_sparse_p2g_reads_explicit_and_implicit_tiles_in_one_block():
    sim = make_sim()
    sim.upload_particles(sc.sparse_particles())
    sim.hash()
    sim.p2g()
    sim.add_gravity(sc.DT)
    cells = check(sim, "sparse p2g + gravity")
    g_dt = np.array(sc.GRAVITY) * sc.DT
    vel = cells["vel"].reshape(sc.SIZE[2], sc.SIZE[1], sc.SIZE[0], 3)
    implicit, explicit = [], []
    for tz in range(0, sc.SIZE[2], 8):
        for ty in range(0, sc.SIZE[1], 8):
            for tx in range(0, sc.SIZE[0], 8):
                tile = vel[tz:tz + 8, ty:ty + 8, tx:tx + 8]
                (implicit if (tile == g_dt).all() else explicit).append((tx // 8, ty // 8, tz // 8))
    print("implicit tiles", len(implicit), "explicit tiles", len(explicit))
    assert implicit and explicit
    # the lattice sits on a face between the two kinds: some point's block reads both within one sample
    kinds = np.zeros((-(-sc.SIZE[2] // 8), -(-sc.SIZE[1] // 8), -(-sc.SIZE[0] // 8)), dtype=bool)
    for t in implicit:
        kinds[t[2], t[1], t[0]] = True
    fi, inside = sc.classify(POINTS)
    c = sc.cells_of(fi[inside])
    n = np.array(sc.SIZE)
    lo, hi = np.maximum(c - 1, 0) >> 3, np.minimum(c + 1, n - 1) >> 3
    mixed = np.zeros(len(c), dtype=bool)
    for corner in np.ndindex(2, 2, 2):
        t = np.where(np.array(corner), hi, lo)
        mixed |= kinds[t[:, 2], t[:, 1], t[:, 0]] != kinds[lo[:, 2], lo[:, 1], lo[:, 0]]
    assert mixed.sum() > 100
    sim.close()


@pytest.mark.parametrize("method,blend", [(lfa.APIC, 1.0), (lfa.FLIP_BLEND, 0.95)], ids=["apic", "flip095"])
def test_stepped(method, blend):
    sim = make_sim(method=method, blending=blend)
    sim.upload_particles(sc.sparse_particles())
    for step in range(3):
        sim.time_step(sc.DT)
    cells = check(sim, "three steps")
    assert np.abs(cells["vel"]).max() > 0.0
    sim.close()


def test_sizes():
    sim = make_sim()
    sim.upload_cells(sc.random_field())
    # the prefix of the set is the lattice; the outside block sits at its end: a prefix with outside points as well
    mixed = np.concatenate([POINTS[-14:], POINTS])
    for n in (0, 1, 63, 64, 65, 257, len(mixed)):
        check(sim, f"prefix of {n}", mixed[:n])
    for n in (0, 1, 63, 64, 65, 257, len(POINTS)):
        check(sim, f"prefix of {n}", POINTS[:n])
    sim.close()


def test_arguments():
    sim = make_sim()
    sim.upload_cells(sc.random_field())
    lib, n = sim.lib, len(POINTS)
    ms = C.c_double(-1.0)
    assert lib.lfa_sample_velocity_time(sim.h, C.byref(ms)) == -1  # LFA_E_INVALID: nothing has run yet
    full = sim.sample_velocity(POINTS, types=True)
    vel = np.full((n, 3), np.nan)
    assert lib.lfa_sample_velocity(sim.h, POINTS.ctypes.data_as(C.c_void_p), n, vel.ctypes.data_as(C.c_void_p), None, None) == 0
    assert vel.tobytes() == full[0].tobytes()
    assert sim.sample_velocity(POINTS)[0].tobytes() == full[0].tobytes()  # types=NULL, a count
    assert lib.lfa_sample_velocity_time(sim.h, C.byref(ms)) == 0 and ms.value >= 0.0
    assert sim.sample_velocity_ms() >= 0.0
    # n == 0: LFA_OK, nothing written but the count
    out = C.c_uint64(77)
    assert lib.lfa_sample_velocity(sim.h, None, 0, None, None, C.byref(out)) == 0 and out.value == 0
    assert lib.lfa_sample_velocity(sim.h, None, 0, None, None, None) == 0
    # n >= 2^32: LFA_E_INVALID before anything is read
    assert lib.lfa_sample_velocity(sim.h, POINTS.ctypes.data_as(C.c_void_p), 1 << 32, vel.ctypes.data_as(C.c_void_p), None, None) == -1
    assert lib.lfa_sample_velocity(sim.h, None, 5, vel.ctypes.data_as(C.c_void_p), None, None) == -1
    assert vel.tobytes() == full[0].tobytes()
    sim.close()
