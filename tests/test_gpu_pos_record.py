"""GPU tests (-m gpu) of the particle position record: key and the three in-cell fractions travel as one 16-byte record
(libfluid_amd/csrc/common.h, PosRec), read and written whole by the advection, the tile scatter, P2G, the fine index, the
correction's three kernels and G2P; the keys alone, in binned order, sit in lfa_sim::bkey for the cell count, the correction's
fallback pass and the undo. The clouds are those of tests/streaming_tail_cases.py and tests/correction_output_cases.py plus
tests/pos_record_cases.py; tests/test_pos_record_cases.py shows that they hold what they are chosen for.

Every comparison is device against oracle on the same input at the bars these stages have: positions 2e-5 h
(tests/test_gpu_move_edges.py), the correction's flat bar (tests/test_gpu_correction_output.py); keys, counts and fluid cells
exact. Round trips compare the device with what was uploaded, bit for bit: the positions are dyadic, h = 1, no offset, so
cell + fp32 fraction is exact. Every comparison with a bar prints `MARGIN <what> <error / bar>` before it asserts."""
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import correction_cases as cc
from tests import correction_output_cases as oc
from tests import move_cases as mc
from tests import pos_record_cases as pc
from tests import streaming_tail_cases as sc
from tests import test_gpu_correction_output as go
from tests.test_gpu_binning_edges import blank
from tests.test_gpu_move_edges import close as close_pos
from tests.test_gpu_move_edges import make_sim as make_move_sim
from tests.test_gpu_streaming_tails import check_binned

pytestmark = pytest.mark.gpu

METHODS = {"apic": (lfa.APIC, orc.APIC), "flip": (lfa.FLIP_BLEND, orc.FLIP), "pic": (lfa.PIC, orc.PIC)}


def raw_of(size, pos):
    """The reference's cell index (x fastest) of exact positions."""
    c = np.minimum(np.floor(pos).astype(np.int64), np.asarray(size) - 1)
    return (c[:, 0] + size[0] * (c[:, 1] + size[1] * c[:, 2])).astype(np.uint64)


def counts_of(size, raw):
    return np.bincount(np.asarray(raw, dtype=np.int64), minlength=int(np.prod(size))).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("n", pc.ROUND_TRIP_COUNTS)
def test_upload_then_download_is_bit_exact(n):
    """n = 1, 3, 4, 5, 255, 257 on the ragged 24 x 17 x 17 grid: the last records of a 16-byte store and load."""
    size, parts, solid, meta = sc.lattice(n)
    s = make_move_sim((size, parts, solid, meta))
    out = s.download_particles(into=blank(n), write_positions=True)
    assert np.array_equal(out["pos"], parts["pos"]) and np.array_equal(out["raw"], raw_of(size, parts["pos"]))
    assert np.array_equal(out["vel"], parts["vel"]) and np.array_equal(out["cx"][:, 0], np.arange(n))
    s.hash()  # the scatter moves the records; a download puts them back under their ids
    out = s.download_particles(into=blank(n), write_positions=True)
    s.close()
    assert np.array_equal(out["pos"], parts["pos"]) and np.array_equal(out["raw"], raw_of(size, parts["pos"]))
    assert np.array_equal(out["vel"], parts["vel"]) and np.array_equal(out["cx"][:, 0], np.arange(n))


# ---------------------------------------------------------------------------------------------------------------------- hash
def test_hash_with_tile_starts_of_every_residue_mod_4():
    """Tiles of 1, 2, 3, 5, 1, 2, 3, 5 particles: the binned records of a tile, and its keys in bkey, start at every phase of a
    16-byte quad. Per-tile counts, cell counts (read from bkey) and fluid cells are the oracle's, the records come back exact."""
    cloud = pc.build("residues")
    size, parts, solid, meta = cloud
    want = pc.oracle_hash("residues")
    s = make_move_sim(cloud)
    s.hash()
    check_binned(s, cloud, want, "residues hash")
    out = s.download_particles(into=blank(len(parts)), write_positions=True)
    assert np.array_equal(out["pos"], parts["pos"])
    assert np.array_equal(s.cell_counts(), counts_of(size, out["raw"]))
    s.hash()  # and once more, from the binned order (no shuffle inside the tiles this time)
    check_binned(s, cloud, want, "residues hash,hash")
    s.close()


# --------------------------------------------------------------------------------------------------------------------- holes
def test_the_hole_marker_survives_a_time_step_on_two_slab_ranks():
    """The largest lattice on two virtual slab ranks: to each rank the other's particles are holes, key 0xFFFFFFFF in the record,
    lane by lane in every chunk of k_advect_collide_count. A hole whose key came back changed by a single bit would be a particle:
    after one time_step and a hash every particle is held by exactly one rank at the oracle's position under the oracle's key."""
    name = f"lattice_n{sc.SLAB_N}"
    cloud = sc.build(name)
    size, parts, solid, meta = cloud
    want = sc.oracle_moves(name)["step"]
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
            _, _, rc = sims[r].time_step(meta["dt"])
            assert rc >= 0
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
    assert np.array_equal(np.sort(ids), np.arange(len(parts)))  # nobody twice, nobody lost, no hole turned particle
    assert all(len(g[1]) >= 64 for g in got)
    back = np.empty(len(parts), dtype=np.int64)
    back[ids] = np.arange(len(ids))
    rec = rec[back]
    close_pos(rec["pos"], want["pos"], meta["h"], f"{name} two slab ranks time_step,hash")
    assert np.array_equal(rec["raw"], want["raw"])
    nz = [8 * b for b in sc.SLAB_BOUNDS]
    shape = size[::-1]
    for r in range(2):  # a rank counts its own cell layers
        z = slice(nz[r], min(nz[r + 1], size[2]))
        assert np.array_equal(got[r][2].reshape(shape)[z], want["counts"].reshape(shape)[z])


# ---------------------------------------------------------------------------------------------------------------- whole step
@pytest.mark.parametrize("method", METHODS)
def test_one_time_step_per_method(method):
    """APIC, FLIP and PIC (the last two keep C in its home array: their scatter moves the record and the id alone) on `mixed`:
    marching lanes beside open-water ones, and particles ON the max face, whose fraction 1.0f comes back exactly from an upload
    and a hash. The positions after a step do not depend on the method: the move takes the velocities of before the step, and
    nobody is within the correction's reach."""
    cloud = sc.build("mixed")
    size, parts, solid, meta = cloud
    want = sc.oracle_moves("mixed")["step"]
    dev, _ = METHODS[method]
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=dev, blending=mc.BLEND)
    s.set_solid_cells(solid)
    s.upload_particles(parts)
    s.hash()
    out = s.download_particles(into=blank(len(parts)), write_positions=True)
    face = np.array([k == "max_face" for k in meta["kind"]])
    assert np.array_equal(out["pos"], parts["pos"]) and (out["pos"][face, 1] == size[1]).all()  # t == 1.0f, exactly
    assert np.array_equal(out["raw"], raw_of(size, parts["pos"]))
    res, it, rc = s.time_step(meta["dt"])
    assert rc >= 0
    out = s.download_particles(into=blank(len(parts)), write_positions=True)
    close_pos(out["pos"], want["pos"], meta["h"], f"mixed {method} time_step")
    assert np.array_equal(out["raw"], want["raw"])
    assert np.isfinite(out["vel"]).all()
    s.hash()
    out = s.download_particles(into=blank(len(parts)), write_positions=True)
    close_pos(out["pos"], want["pos"], meta["h"], f"mixed {method} time_step,hash")
    assert np.array_equal(out["raw"], want["raw"])
    assert np.array_equal(s.cell_counts(), want["counts"]) and np.array_equal(s.fluid_cells(), want["fluid_cells"])
    s.close()


# ------------------------------------------------------------------------------------------- second pass and fallback kernel
@pytest.mark.parametrize("module,name", [("output", "second_pass"), ("output", "second_pass_spread"), ("edges", "cap_edge")],
                         ids=["second_pass", "second_pass_spread", "cap_edge"])
def test_second_pass_and_fallback_store_whole_records(module, name):
    """second_pass: the crowded tile's parts go through k_correct_fine<FINE_CAP_BIG, true>; cap_edge: parts beyond that go through
    k_correct_collide, which takes the keys of before the correction from bkey. (The device run is the one
    tests/test_gpu_correction_output.py shares.)"""
    mod = go.MODULES[module]
    cloud = mod.build(name)
    out, (to_gather, total, to_second) = go.device_fused(module, name)
    assert to_second > 0 and (to_gather > 0) == (name == "cap_edge")
    go.close(out, mod.oracle(name)["collide"], cc.FLAT_BAR * cloud[3]["h"], f"pos record {name} correct_collide", go.keep_of(cloud))


# ---------------------------------------------------------------------------------------------------------------------- undo
@pytest.mark.parametrize("name", ["empty_part", "second_pass", "last_tile"])
def test_undo_restores_keys_and_fractions_bit_for_bit(name):
    """correct_collide_begin, correct_collide_undo: every record is what it was (the fractions from the fine index, the keys from
    bkey). Then begin, end, hash: the cell counts, which the binning reads from bkey, are the histogram of the downloaded keys."""
    cloud = oc.build(name)
    size, parts, solid, meta = cloud
    s = go.make_sim(cloud)
    s.hash()
    before = go.positions(s, parts)
    s.correct_collide_begin(cc.DT)
    s.correct_collide_undo()
    after = go.positions(s, parts)
    assert np.array_equal(after["pos"], before["pos"]) and np.array_equal(after["raw"], before["raw"])
    assert np.array_equal(before["pos"], parts["pos"])  # (dyadic starts: exact)
    s.correct_collide_begin(cc.DT)
    s.correct_collide_end()
    moved = go.positions(s, parts)
    go.close(moved["pos"], oc.oracle(name)["collide"], cc.FLAT_BAR * meta["h"], f"pos record {name} begin,end", go.keep_of(cloud))
    assert (moved["pos"] != before["pos"]).any()
    s.hash()
    binned = go.positions(s, parts)
    assert np.array_equal(binned["pos"], moved["pos"]) and np.array_equal(binned["raw"], moved["raw"])
    assert np.array_equal(s.cell_counts(), counts_of(size, binned["raw"]))
    s.close()


# ------------------------------------------------------------------------------------------------------------- source append
def test_a_source_appends_after_a_binning():
    """A source over an empty corner of `residues` tops its cells up behind the binned records; the hash and the time_step that
    follow take old and new records alike. (Without the pcg32 mode the new positions are the device's own draws: what is checked
    is that the old records are untouched, every new one lies in its source cell, and the counts are the keys' histogram.)"""
    cloud = pc.build("residues")
    size, parts, solid, meta = cloud
    n = len(parts)
    cells = np.array([(x, y, 16) for x in range(17, 22) for y in range(9, 12)], dtype=np.int32)  # tile (2, 1, 2): no particle yet
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=mc.BLEND)
    s.add_source(cells, (0.0, 0.0, 0.0), 2, True, False)
    s.upload_particles(parts)
    s.hash()
    made = s.update_sources()
    assert made == 8 * len(cells) and s.num_particles == n + made
    s.hash()
    out = s.download_particles(into=blank(n + made), write_positions=True)
    old = np.arange(n + made) < n  # (a download puts record i under its id: the appended ones are n .. n + made - 1)
    assert np.array_equal(out["pos"][old], parts["pos"])  # untouched, bit for bit
    assert np.array_equal(out["cx"][old, 0], np.arange(n)) and not out["cx"][~old].any()
    want_raw = np.sort(np.repeat(raw_of(size, cells.astype(np.float64)), 8))
    assert np.array_equal(np.sort(out["raw"][~old]), want_raw)
    assert np.array_equal(out["raw"], raw_of(size, out["pos"]))  # key and fractions of a record belong together
    assert np.array_equal(s.cell_counts(), counts_of(size, out["raw"]))
    res, it, rc = s.time_step(1e-3)
    assert rc >= 0
    s.hash()
    out = s.download_particles(into=blank(n + made), write_positions=True)
    assert np.isfinite(out["pos"]).all() and (out["pos"] >= 0).all() and (out["pos"] <= np.asarray(size)).all()
    assert np.array_equal(out["raw"], raw_of(size, out["pos"]))
    assert np.array_equal(s.cell_counts(), counts_of(size, out["raw"])) and s.cell_counts().sum() == n + made
    s.close()
