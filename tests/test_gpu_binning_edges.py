"""GPU tests (-m gpu) of the binning (k_tile_count / lfa_wave_tile_ranks, k_tile_flags, k_tile_scatter, k_gather_vc, k_cell_count,
k_dilate_slots, the tile lists and lfa_exclusive_scan_u32; through lfa_time_step also k_advect_collide_count) on the designed
clouds of tests/binning_cases.py, against the numpy model beside them. tests/test_binning_cases.py pins that model to the oracle
and to the compiled reference on these very inputs and shows that the cases hold what they are there for.

The contract of a binning, stated without a word about the order inside a tile: every particle keeps its id, its position, its
velocity and its C; its key is its cell; the counts, the fluid cells and the numbers of particle tiles and processed tiles are the
model's. Positions are dyadic and velocities and C small integers that name the particle, so every comparison is np.array_equal -
nothing in this file takes a tolerance except the positions after a whole time step, which have the move tests' bar."""
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import binning_cases as bc
from tests import move_cases as mc
from tests.test_gpu_move_edges import close

pytestmark = pytest.mark.gpu

METHODS = [lfa.APIC, lfa.FLIP_BLEND]
METHOD_IDS = ["apic", "flip"]
BLEND = 0.95


def make_sim(cloud, method, slab=None):
    """slab = (hub, rank, layer bounds): a rank of a z-slab decomposition, handed the whole cloud like every rank."""
    size, parts, solid, meta = cloud
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=method, blending=BLEND)
    if solid is not None:
        s.set_solid_cells(solid)
    if slab is not None:
        s.init_local_slab(slab[0].h, slab[1], slab[2])
    s.upload_particles(parts)
    return s


def blank(n):
    """Records no device wrote: whatever a download leaves alone is recognisable."""
    out = np.zeros(n, dtype=lfa.PARTICLE_DTYPE)
    out["pos"], out["old_pos"] = -7.25, -9.5
    out["vel"], out["cx"], out["cy"], out["cz"] = -1.0, -2.0, -3.0, -4.0
    out["raw"] = 1 << 62
    return out


def check_records(s, parts, want):
    """Every record under its id: key, velocity, C; then the position the device rebuilds."""
    n = len(parts)
    out = s.download_particles(into=blank(n))
    assert np.array_equal(out["raw"], want["raw"])
    assert np.array_equal(out["pos"], blank(n)["pos"]) and np.array_equal(out["old_pos"], blank(n)["old_pos"])  # untouched
    assert np.array_equal(out["vel"], parts["vel"])
    assert np.array_equal(bc.c_of(out), bc.c_of(parts))
    rec = s.download_particles()
    assert np.array_equal(rec["pos"], parts["pos"]) and np.array_equal(rec["old_pos"], parts["pos"])
    assert np.array_equal(rec["vel"], parts["vel"]) and np.array_equal(bc.c_of(rec), bc.c_of(parts))
    assert np.array_equal(rec["raw"], want["raw"])


def check_grid(s, want, n):
    assert np.array_equal(s.cell_counts(), want["counts"])
    assert np.array_equal(s.fluid_cells(), want["fluid_cells"])
    c = s.counts()
    assert (c["particles"], c["unknowns"]) == (n, len(want["fluid_cells"]))
    assert (c["particle_tiles"], c["processed_tiles"]) == (want["particle_tiles"], want["processed_tiles"])


def check_contract(s, cloud, want):
    check_records(s, cloud[1], want)
    check_grid(s, want, len(cloud[1]))


# ------------------------------------------------------------------------------------------- the contract after hash()
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("name", bc.SMALL)
def test_contract_after_hash(name, method):
    cloud = bc.build(name)
    s = make_sim(cloud, method)
    s.hash()
    check_contract(s, cloud, bc.expected(name))
    s.close()


@pytest.mark.parametrize("name", bc.PRIMES)
def test_one_tile_prime_and_its_twin(name):
    """1 000 003 particles in one tile: `cnt % 1000003u != 0` (core.hip:989) is false and the rank must stay the slot - r 1000003
    mod cnt is 0 for every r. 1 000 002 beside it is shuffled. Once, APIC: 152 MB each way."""
    cloud = bc.build(name)
    s = make_sim(cloud, lfa.APIC)
    s.hash()
    check_contract(s, cloud, bc.expected(name))
    s.close()


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("size", bc.SINGLETON_SIZES)
def test_singletons_alone_on_one_handle(size, method):
    """Each particle of a singletons cloud alone, one upload after the other on ONE handle: its tile's clipped neighbourhood of 8,
    12 or 27 tiles is all that is processed - nothing of the upload before stays flagged, no other tile covers a neighbour that
    k_dilate_slots (core.hip:1072-1076) fails to mark."""
    name = "singletons_%dx%dx%d" % size
    cloud = bc.build(name)
    s = make_sim(cloud, method)
    s.hash()
    seen = []
    for i in range(len(cloud[1])):
        one = bc.lone(cloud, i)
        want = bc.model_of(one)
        s.upload_particles(one[1])
        s.hash()
        check_contract(s, one, want)
        seen.append(want["processed_tiles"])
    s.close()
    if size == (24, 40, 56):
        assert sorted(seen) == [8] * 8 + [12] * 12 + [27]


# ------------------------------------------------------------------------------------------- binning on top of binning
def hash_twice(s):
    s.hash(); s.hash()


def hash_download_hash(s):
    s.hash()
    s.download_particles()
    s.hash()


def hash_p2g_hash(s):
    s.hash(); s.p2g(); s.hash()


SEQUENCES = {"hash_hash": hash_twice, "hash_download_hash": hash_download_hash, "hash_p2g_hash": hash_p2g_hash}


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("name", bc.REBIN)
def test_binning_on_binning(name, seq, method):
    """The first hash() defers v and C behind from[] (lfa_sim::vc_pending, core.hip:1254); the second must complete it first
    (lfa_particles_materialize, core.hip:1141) - at once, after a download has completed it already, or after a P2G has read
    through it - and FLIP's C stays in its home array under the id (core.hip:1240-1244)."""
    cloud = bc.build(name)
    s = make_sim(cloud, method)
    SEQUENCES[seq](s)
    check_contract(s, cloud, bc.expected(name))
    s.close()


@pytest.mark.parametrize("first,second", [(lfa.APIC, lfa.FLIP_BLEND), (lfa.FLIP_BLEND, lfa.APIC)], ids=["apic_flip", "flip_apic"])
@pytest.mark.parametrize("name", bc.REBIN)
def test_binning_across_a_change_of_method(name, first, second):
    """hash() under one method, set_params to the other, hash(): C moves to its home array (core.hip:1240) or back into particle
    order (lfa_c_home_restore, core.hip:424 and :1246) with a deferred binning in between."""
    cloud = bc.build(name)
    s = make_sim(cloud, first)
    s.hash()
    s.set_params(simulation_method=second)
    s.hash()
    check_contract(s, cloud, bc.expected(name))
    s.set_params(simulation_method=first)
    check_contract(s, cloud, bc.expected(name))
    s.close()


# ------------------------------------------------------------------------------------------- the counting advection
@pytest.mark.parametrize("name", [n for n in bc.ROUND_ROBIN if "stride" not in n])
def test_time_step_counts_while_it_advects(name):
    """lfa_time_step straight after an upload: k_advect_collide_count (particles.hip:242-) ranks the MOVED particles in upload
    order, a wave of 512 tiles, and the binning that follows takes its counts and ranks as they are (core.hip:1151). Positions per
    id against the oracle's own time_step at the move tests' bar; then a hash() whose keys, counts and tile numbers must be the
    model's for the positions the device itself reports."""
    cloud, dt = bc.with_moves(bc.build(name))
    size, parts, solid, meta = cloud
    meta = dict(meta, skin=mc.SKIN_WORLD / meta["h"])
    want_pos = mc.run_cpu_time_step((size, parts, solid, meta))
    s = make_sim(cloud, lfa.FLIP_BLEND)
    res, it, rc = s.time_step(dt)
    assert rc >= 0
    out = s.download_particles(into=blank(len(parts)), write_positions=True)
    close(out["pos"], want_pos, meta["h"], f"{name} time_step")
    assert np.array_equal(out["cx"][:, 0], np.arange(len(parts)))  # FLIP carries C, and with it the id, through the step
    want = bc.model(size, out["pos"], meta["h"], meta["off"])
    assert np.array_equal(out["raw"], want["raw"])  # the keys of the binning inside the step
    s.hash()
    again = s.download_particles(into=blank(len(parts)), write_positions=True)
    assert np.array_equal(again["pos"], out["pos"]) and np.array_equal(again["raw"], want["raw"])
    assert np.array_equal(again["vel"], out["vel"]) and np.array_equal(bc.c_of(again), bc.c_of(out))
    check_grid(s, want, len(parts))
    s.close()


# ------------------------------------------------------------------------------------------- storage order (slab handles)
def storage_records(s):
    """(records in storage order, their ids) of a slab handle."""
    return s.download_particles(), s.particle_ids()


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("name", bc.REBIN)
def test_storage_order_on_a_one_rank_slab(name, method):
    """A slab handle downloads in storage order: the records are sorted by tile (tile_start, core.hip:991), the ids are a
    permutation, and record k carries the data of particle ids[k] - after the first, shuffled binning and after a second."""
    cloud = bc.build(name)
    size, parts, solid, meta = cloud
    want = bc.expected(name)
    hub = lfa.LocalHub(1)
    s = make_sim(cloud, method, slab=(hub, 0, [0, bc.tiles_of(size)[2]]))
    for _ in range(2):
        s.hash()
        rec, ids = storage_records(s)
        assert np.array_equal(np.sort(ids), np.arange(len(parts)))
        assert (np.diff(want["tile"][ids]) >= 0).all()
        assert np.array_equal(rec["raw"], want["raw"][ids]) and np.array_equal(rec["pos"], parts["pos"][ids])
        assert np.array_equal(rec["vel"], parts["vel"][ids]) and np.array_equal(bc.c_of(rec), bc.c_of(parts)[ids])
        assert np.array_equal(s.cell_counts(), want["counts"]) and np.array_equal(s.fluid_cells(), want["fluid_cells"])
    s.close()
    hub.close()


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("name", ["round_robin_n2049", "round_robin_stride201_n4097"])
def test_two_slab_ranks_share_every_wave(name, method):
    """Two virtual ranks split at tile layer 4, each handed the whole cloud: k_ingest gives the other rank's particles the key
    0xFFFFFFFF (core.hip:546), which k_tile_count (core.hip:940) and the scatter (core.hip:986) must skip - in every wave, half of
    the lanes (stride 201: lane by lane). Each rank's records are sorted by tile and are its own particles; together they are the
    upload."""
    cloud = bc.build(name)
    size, parts, solid, meta = cloud
    want = bc.expected(name)
    bounds = [0, 4, 8]
    hub = lfa.LocalHub(2)
    sims = [make_sim(cloud, method, slab=(hub, r, bounds)) for r in range(2)]
    got, errors = [None, None], []

    def worker(r):
        try:
            sims[r].hash()
            got[r] = storage_records(sims[r]) + (sims[r].cell_counts(),)
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
    layer = want["tile"] // 64
    for r, (rec, ids, counts) in enumerate(got):
        mine = np.flatnonzero((layer >= bounds[r]) & (layer < bounds[r + 1]))
        assert np.array_equal(np.sort(ids), mine) and len(rec) == len(mine) > 0
        assert (np.diff(want["tile"][ids]) >= 0).all()
        assert np.array_equal(rec["raw"], want["raw"][ids]) and np.array_equal(rec["pos"], parts["pos"][ids])
        assert np.array_equal(rec["vel"], parts["vel"][ids]) and np.array_equal(bc.c_of(rec), bc.c_of(parts)[ids])
        z = slice(bounds[r] * 8, bounds[r + 1] * 8)  # a rank counts its own cell layers (its ghost layers belong to the neighbour)
        assert np.array_equal(counts.reshape(size[::-1])[z], want["counts"].reshape(size[::-1])[z])
    ids = np.concatenate([g[1] for g in got])
    rec = np.concatenate([g[0] for g in got])
    back = np.empty(len(parts), dtype=np.int64)
    back[ids] = np.arange(len(ids))
    rec = rec[back]
    for f in ("pos", "vel", "cx", "cy", "cz"):
        assert np.array_equal(rec[f], parts[f])
