"""GPU tests (-m gpu) of the kernels that only stream particles - k_advect_collide, k_advect_collide_count, k_tile_scatter,
k_cell_count, k_build_fine_index (through lfa_time_step) and k_g2p - on the designed clouds of tests/streaming_tail_cases.py. Each
of them but the scatter issues a thread's loads up front, clamped at the end of the array or the tile, and its stores last; the clouds sit
on the tails: particle counts around a chunk, a wave and a workgroup, waves whose lanes take different paths, tiles of one round
more or less than the G2P loop's stride, and tiles that lose exactly as many particles as their leaver list holds.
tests/test_streaming_tail_cases.py shows that the clouds hold what they are named for.

Every comparison is device against oracle on the same input, at the bars these stages have: positions 2e-5 h
(tests/test_gpu_move_edges.py), keys, counts and fluid cells exact (tests/test_gpu_binning_edges.py), velocities VEL_REL (FLIP: twice)
and C 5e-5 (tests/test_gpu_transfer_edges.py). Every comparison with a bar prints `MARGIN <what> <error / bar>` before it asserts."""
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import binning_cases as bc
from tests import move_cases as mc
from tests import streaming_tail_cases as sc
from tests import transfer_cases as tc
from tests.test_gpu_binning_edges import blank
from tests.test_gpu_move_edges import close as close_pos
from tests.test_gpu_move_edges import make_sim as make_move_sim
from tests.test_gpu_parity import cells_from
from tests.test_gpu_transfer_edges import C_REL, c_of, g2p_bar
from tests.test_gpu_transfer_edges import close as close_rel
from tests.test_gpu_transfer_edges import make_sim as make_transfer_sim

pytestmark = pytest.mark.gpu


def per_tile(size, counts):
    """Cell counts (x fastest) summed over the 8^3 tiles."""
    nx, ny, nz = size
    c = np.zeros([8 * t for t in bc.tiles_of(size)][::-1], dtype=np.int64)
    c[:nz, :ny, :nx] = np.asarray(counts, dtype=np.int64).reshape(nz, ny, nx)
    nt = bc.tiles_of(size)
    return c.reshape(nt[2], 8, nt[1], 8, nt[0], 8).sum(axis=(1, 3, 5))


def check_binned(s, cloud, want, what):
    """Positions at the move tests' bar; keys, cell counts, per-tile counts and fluid cells exactly the oracle's."""
    size, parts, solid, meta = cloud
    out = s.download_particles(into=blank(len(parts)), write_positions=True)
    close_pos(out["pos"], want["pos"], meta["h"], what)
    assert np.array_equal(out["raw"], want["raw"]), what
    assert np.array_equal(out["cx"][:, 0], np.arange(len(parts))), what  # FLIP carries C, and with it the id, along
    counts = s.cell_counts()
    assert np.array_equal(counts, want["counts"]), what
    assert np.array_equal(per_tile(size, counts), per_tile(size, want["counts"])) and counts.sum() == len(parts), what
    assert np.array_equal(s.fluid_cells(), want["fluid_cells"]), what
    assert s.counts()["particle_tiles"] == int((per_tile(size, want["counts"]) > 0).sum()), what


def run_move_then_step(name, source=None):
    cloud = sc.build(name)
    want = sc.oracle_moves(name)
    # advect_collide + hash: k_advect_collide, then the binning's own count pass, the scatter and the cell counts
    s = make_move_sim(cloud)
    s.advect_collide(cloud[3]["dt"])
    s.hash()
    check_binned(s, cloud, want["move"], f"{name} advect_collide,hash")
    s.close()
    # one time_step from the upload: k_advect_collide_count ranks on the way, the binning takes its counts as they are; the
    # correction (k_build_fine_index and the pair kernel) moves nobody - the clouds keep everybody out of its reach
    s = make_move_sim(cloud)
    res, it, rc = s.time_step(cloud[3]["dt"])
    assert rc >= 0
    out = s.download_particles(into=blank(len(cloud[1])), write_positions=True)
    close_pos(out["pos"], want["step"]["pos"], cloud[3]["h"], f"{name} time_step")
    assert np.array_equal(out["raw"], want["step"]["raw"])  # the keys of the binning inside the step
    s.hash()
    check_binned(s, cloud, want["step"], f"{name} time_step,hash")
    s.close()


@pytest.mark.parametrize("n", sc.COUNTS)
def test_particle_counts_around_a_chunk_a_wave_and_a_workgroup(n):
    """n = 1, 63, 64, 65, 511, 512, 513 and 64 AC_CHUNKS k +- 1 on 24 x 17 x 17: the last wave of the advection and of the
    scatter is partly filled (its loads are clamped to n - 1, its results dropped), and every wave of 64 or more mixes lanes that
    take the open-water short cut with lanes that march."""
    run_move_then_step(f"lattice_n{n}")


def test_mixed_lanes_in_every_chunk():
    """mixed: open-water lanes, lanes in a plate's skin, lanes that hit it, moves of exactly 7 cells and particles on the max face
    in every wave - the general collide() march keeps its dependent loads while the other lanes' values wait in registers."""
    run_move_then_step("mixed")


def test_mixed_lanes_with_a_coercing_source():
    """k_advect_collide<true> on the same cloud: the coerced particles take the source's velocity and C = 0, stored after the move
    with the keys and fractions; nobody else's velocity or C is touched."""
    source, cloud = sc.mixed_source()
    size, parts, solid, meta = cloud
    want = mc.run_cpu(cloud, "oracle", source)
    s = make_move_sim(cloud, source)
    s.advect_collide(meta["dt"])
    out = s.download_particles(into=parts.copy(), write_positions=True)
    s.close()
    close_pos(out["pos"], want["collide"], meta["h"], "mixed coerced advect_collide")
    assert np.array_equal(out["vel"], want["vel"])
    taken = (want["vel"] == np.asarray(source[1])).all(axis=1)
    assert 50 <= taken.sum() <= len(parts) - 50
    assert not out["cx"][taken].any() and np.array_equal(out["cx"][~taken], parts["cx"][~taken])
    assert np.array_equal(out["vel"][~taken], parts["vel"][~taken])


def test_holes_of_a_slab_drop_in_every_chunk():
    """Two virtual slab ranks split at z = 8, each handed the whole shuffled lattice: the other rank's particles are holes (key
    0xFFFFFFFF) lane by lane in every chunk of every wave. The move and the scatter load a hole's slot like any other and must
    neither move, rank nor store it: after advect_collide + hash every particle is held by exactly one rank, at the oracle's
    position, under the oracle's key, and the ranks' cell counts add up to the oracle's."""
    name = f"lattice_n{sc.SLAB_N}"
    cloud = sc.build(name)
    size, parts, solid, meta = cloud
    want = sc.oracle_moves(name)["move"]
    hub = lfa.LocalHub(2)
    sims = []
    for r in range(2):
        s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=mc.BLEND)
        s.init_local_slab(hub.h, r, list(sc.SLAB_BOUNDS))
        s.upload_particles(parts)
        sims.append(s)
    got, errors = [None, None], []

    def worker(r):
        try:
            sims[r].advect_collide(meta["dt"])
            sims[r].hash()
            got[r] = (sims[r].download_particles(), sims[r].particle_ids(), sims[r].cell_counts())
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    alive = any(t.is_alive() for t in threads)
    if not alive:
        for s in sims:
            s.close()
        hub.close()
    assert not errors, errors
    assert not alive, "slab threads hung"
    ids = np.concatenate([g[1] for g in got])
    rec = np.concatenate([g[0] for g in got])
    assert np.array_equal(np.sort(ids), np.arange(len(parts)))  # nobody twice, nobody lost
    assert all(len(g[1]) >= 64 for g in got)
    back = np.empty(len(parts), dtype=np.int64)
    back[ids] = np.arange(len(ids))
    rec = rec[back]
    close_pos(rec["pos"], want["pos"], meta["h"], f"{name} two slab ranks advect_collide,hash")
    assert np.array_equal(rec["raw"], want["raw"])
    assert np.array_equal(rec["vel"], parts["vel"]) and np.array_equal(rec["cx"][:, 0], np.arange(len(parts)))
    nz = [8 * b for b in sc.SLAB_BOUNDS]
    shape = size[::-1]
    for r in range(2):  # a rank counts its own cell layers
        z = slice(nz[r], min(nz[r + 1], size[2]))
        assert np.array_equal(got[r][2].reshape(shape)[z], want["counts"].reshape(shape)[z])


FLIP_BINNINGS = ("deferred", "completed")
G2P_RUNS = [(tc.PIC, "deferred"), (tc.APIC, "deferred")] + [(tc.FLIP, b) for b in FLIP_BINNINGS]


@pytest.mark.parametrize("method,binning", G2P_RUNS, ids=[f"{tc.method_id(m)}-{b}" for m, b in G2P_RUNS])
def test_g2p_on_tiles_around_its_loop_stride(method, binning):
    """Tiles of 1, 255, 256, 257 and 4 097 particles (and tiles of none): the G2P loop prefetches its next round's particle, past
    the end of the tile the tile's last slot. FLIP reads the velocity of before the step through the binning's source index while
    the binning is deferred, and in place - the arrays it writes - once a download has completed it."""
    cloud = sc.build("g2p_tiles")
    size, parts, solid, meta = cloud
    want = tc.staged_cloud(cloud, method)
    label = f"g2p_tiles {tc.method_id(method)} {binning}"
    s = make_transfer_sim(cloud, method)
    s.hash()
    if binning == "completed":
        s.download_particles()
    if method == tc.FLIP:
        s.p2g()
    s.upload_cells(cells_from(want["extrap_vel"], want["extrap_type"]))
    s.g2p()
    cfl = s.cfl()
    out = s.download_particles(into=parts.copy())
    s.close()
    close_rel(out["vel"], want["g2p_vel"], g2p_bar(method), f"{label} g2p_vel")
    if method == tc.APIC:
        close_rel(c_of(out), want["g2p_c"], C_REL, f"{label} g2p_c")
    else:  # PIC and FLIP carry C through unchanged
        assert np.array_equal(c_of(out).astype(np.float32), c_of(parts).astype(np.float32))
    assert np.isfinite(want["cfl"]) and abs(cfl - want["cfl"]) <= 1e-4 * want["cfl"], (label, cfl, want["cfl"])


@pytest.mark.parametrize("method", tc.ALL_METHODS, ids=tc.method_id)
def test_stale_g2p_with_exactly_as_many_leavers_as_the_tile_list_holds(method):
    """A G2P on the order of the last binning after a move: one tile loses G2P_LV_CAP + 44 particles (the 44 go to the global
    list one by one), one exactly G2P_LV_CAP (the list is full, nothing overflows), one none. The oracle transfers the device's
    own downloaded positions (cell + fp32 fraction: exact in fp64 at cell size 1) on the device's own grid; FLIP's old grid is the
    oracle's P2G of the particles as uploaded."""
    cloud = sc.build("stale_leavers")
    size, parts, solid, meta = cloud
    stages = tc.staged_cloud(cloud, method)
    s = make_transfer_sim(cloud, method)
    s.hash()
    s.p2g()
    s.upload_cells(cells_from(stages["extrap_vel"], stages["extrap_type"]))
    grid = s.cells()
    s.advect_collide(meta["dt"])  # moves the particles in the binning's order; nothing bins again before the transfer
    s.g2p()
    cfl = s.cfl()
    got = s.download_particles(into=parts.copy(), write_positions=True)
    s.close()
    t0, t1 = sc.tile_of(size, parts["pos"]), sc.tile_of(size, got["pos"])
    left = (t0 != t1).any(axis=1)
    assert np.array_equal(left, meta["leaves"])
    lost = sorted(int(left[(t0 == k).all(axis=1)].sum()) for k in np.unique(t0, axis=0))
    assert lost == [0, sc.G2P_LV_CAP, sc.G2P_LV_CAP + 44]
    o = orc.CpuSim(size, method=method, blending=tc.BLEND[method])
    o.set_particles(parts)
    o.hash(); o.p2g()
    moved = parts.copy()
    moved["pos"] = got["pos"]
    o.set_particles(moved)
    o.set_cells(grid)
    o.g2p()
    want = o.particles()  # (no hash since: the order of `moved`)
    want_cfl = o.cfl()
    o.close()
    assert np.array_equal(want["pos"], got["pos"])
    label = f"stale_leavers g2p {tc.method_id(method)}"
    close_rel(got["vel"], want["vel"], g2p_bar(method), f"{label} g2p_vel")
    close_rel(got["vel"][left], want["vel"][left], g2p_bar(method), f"{label} g2p_vel_leavers")
    if method == tc.APIC:
        close_rel(c_of(got), c_of(want), C_REL, f"{label} g2p_c")
        close_rel(c_of(got)[left], c_of(want)[left], C_REL, f"{label} g2p_c_leavers")
    else:
        assert np.array_equal(c_of(got).astype(np.float32), c_of(parts).astype(np.float32))
    assert abs(cfl - want_cfl) <= 1e-4 * want_cfl, (cfl, want_cfl)
    assert np.abs(got["vel"] - parts["vel"]).max() > 1e-2 * np.abs(got["vel"]).max()  # the transfer did change velocities
