"""CPU tests of tests/binning_cases.py: the numpy model the GPU tests compare the device with IS the oracle and the compiled
reference on exactly these inputs (a live oracle/_ref where it is present, its recorded counts and digests in
tests/golden/binning.npz where not), and every case holds what it is there for. Bit for bit throughout; there is no tolerance in
this file except where it says that a time step's correction moves nothing."""
import os

import numpy as np
import pytest

from oracle import loader as orc
from tests import binning_cases as bc
from tests import move_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binning.npz")
needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")


@pytest.fixture(scope="module")
def golden():
    """case -> (counts int64[4], digests uint8[3, 32]) of the compiled reference."""
    with np.load(GOLDEN) as z:
        return {str(k): (c, s) for k, c, s in zip(z["ids"], z["counts"], z["sha"])}


def same_as_model(name, got):
    want = bc.expected(name)
    raw, counts, fluid = got
    assert raw.dtype == np.uint64 and np.array_equal(raw, want["raw"])
    assert np.array_equal(counts, want["counts"])
    assert np.array_equal(fluid, want["fluid_cells"])


# ------------------------------------------------------------------------------------------- model == oracle == reference
@pytest.mark.parametrize("name", bc.NAMES)
def test_model_is_the_oracle(name):
    same_as_model(name, bc.run_cpu(bc.build(name), "oracle"))


@needs_ref
@pytest.mark.parametrize("name", bc.NAMES)
def test_model_is_the_live_reference(name):
    same_as_model(name, bc.run_cpu(bc.build(name), "ref"))


@pytest.mark.parametrize("name", bc.GOLDEN)
def test_model_matches_reference_golden(golden, name):
    want = bc.expected(name)
    counts, sha = bc.summary(want["raw"], want["counts"], want["fluid_cells"])
    assert np.array_equal(counts, golden[name][0])
    assert np.array_equal(sha, golden[name][1])


def test_golden_holds_digests_and_counts_only(golden):
    assert sorted(golden) == sorted(bc.GOLDEN)
    with np.load(GOLDEN) as z:
        assert sorted(z.files) == ["counts", "ids", "sha"]
        assert z["counts"].shape == (len(bc.GOLDEN), 4) and z["sha"].shape == (len(bc.GOLDEN), 3, 32)
    assert os.path.getsize(GOLDEN) < 8 * 1024


# ------------------------------------------------------------------------------------------- what every case holds
@pytest.mark.parametrize("name", bc.NAMES)
def test_positions_are_dyadic_and_records_name_their_particle(name):
    """(p - off) / h is cell + k / 16 exactly, the fp32 fraction is exact, the rebuilt position is the uploaded one; velocity and C
    are integers that fp32 holds and differ from particle to particle."""
    size, parts, solid, meta = bc.build(name)
    g = (parts["pos"] - np.asarray(meta["off"])) / meta["h"]
    assert np.array_equal(g, meta["cell"] + meta["k16"] / 16.0)
    cell = np.minimum(np.floor(g).astype(np.int64), np.asarray(size) - 1)
    t = (g - cell).astype(np.float32)
    assert np.array_equal(t.astype(np.float64), g - cell) and (t <= 1).all()
    assert np.array_equal(np.asarray(meta["off"]) + (cell + t.astype(np.float64)) * meta["h"], parts["pos"])
    n = len(parts)
    for f in (parts["vel"], bc.c_of(parts)):
        assert np.array_equal(f.astype(np.float32).astype(np.float64), f) and np.array_equal(f, np.rint(f))
    assert np.array_equal(parts["vel"][:, 0], np.arange(n)) and np.array_equal(parts["cx"][:, 0], np.arange(n))
    m = bc.expected(name)
    assert m["tile_counts"].sum() == n == m["counts"].sum() and m["particle_tiles"] == (m["tile_counts"] > 0).sum()
    assert np.array_equal(m["tile_counts"], np.bincount(m["tile"], minlength=len(m["tile_counts"])))


@pytest.mark.parametrize("name", bc.ROUND_ROBIN)
def test_round_robin_every_wave_holds_512_distinct_tiles(name):
    size, parts, solid, meta = bc.build(name)
    tile = bc.expected(name)["tile"]
    n = len(tile)
    assert n in bc.RR_NS and size == bc.RR_SIZE
    for w0 in range(0, n, bc.WAVE_PARTICLES):
        w = tile[w0:w0 + bc.WAVE_PARTICLES]
        assert len(np.unique(w)) == len(w)  # (the last wave of n = 2 047 holds 511, of 2 049 and 4 097 one)
    for i0 in range(0, n - bc.WAVE_PARTICLES + 1, 97):  # and so does every other run of 512 consecutive uploads
        assert len(np.unique(tile[i0:i0 + bc.WAVE_PARTICLES])) == bc.WAVE_PARTICLES
    if meta["stride"] == 1:
        assert np.array_equal(tile, np.arange(n) % 512)
    # n sits on the wave's and the workgroup's edges (core.hip:1154: one workgroup per 2 048 particles)
    assert {512: (1, 1), 2047: (4, 1), 2048: (4, 1), 2049: (5, 2), 4097: (9, 3)}[n] == \
        (-(-n // bc.WAVE_PARTICLES), -(-n // bc.GROUP_PARTICLES))


def test_round_robin_stride_interleaves_two_slab_ranks_lane_by_lane():
    """Split at tile layer 4, neighbouring lanes of a wave belong to different ranks again and again: each rank's wave holds its
    own keys and 0xFFFFFFFF side by side."""
    tile = bc.expected("round_robin_stride201_n4097")["tile"]
    upper = tile // 64 >= 4
    for w0 in range(0, 4096, 64):
        assert 8 <= np.count_nonzero(np.diff(upper[w0:w0 + 64].astype(np.int8)))
    assert np.count_nonzero(upper[:4096]) == 2048


def test_two_tiles_alternating_carries_the_base_across_all_chunks():
    size, parts, solid, meta = bc.build("two_tiles_alternating")
    m = bc.expected("two_tiles_alternating")
    n = len(parts)
    assert np.array_equal(m["tile"], (np.arange(n) % 2) * 2) and m["particle_tiles"] == 2 and m["processed_tiles"] == 3
    assert n % 2 == 1 and n > 2 * bc.GROUP_PARTICLES and n % 64 != 0
    for c0 in range(0, n - 63, 64):  # every full chunk of 64 lanes holds 32 of each tile
        assert np.bincount(m["tile"][c0:c0 + 64], minlength=3).tolist() == [32, 0, 32]
    assert m["tile_counts"].tolist() == [(n + 1) // 2, 0, n // 2]
    assert (m["counts"].reshape(8, 8, 24)[:, :, 8:16] == 0).all() and m["counts"].max() >= 5


@pytest.mark.parametrize("name,n", [("one_tile_prime", 1000003), ("one_tile_prime_twin", 1000002)])
def test_one_tile_prime_count(name, n):
    size, parts, solid, meta = bc.build(name)
    m = bc.expected(name)
    assert m["tile_counts"].tolist() == [n] and len(parts) == n and bc.PRIME == 1000003
    assert (n % bc.PRIME == 0) == (name == "one_tile_prime")
    assert all(n % p for p in range(2, 1001)) == (name == "one_tile_prime")  # 1 000 003 is prime (1 001^2 > n)
    assert (m["counts"] >= n // 512 - 50).all() and len(m["fluid_cells"]) == 512
    g = (parts["pos"] - np.asarray(meta["off"])) / meta["h"]
    on = (g == 8.0)
    assert on.any(axis=0).all() and (on.sum(axis=1) == 2).sum() > 1000 and on.any(axis=1).sum() == len(meta["on_face"])
    assert (m["raw"][on[:, 0]] % 8 == 7).all()  # clamped into the last cell


@pytest.mark.parametrize("size", bc.SINGLETON_SIZES)
def test_singletons_tiles_and_clipped_neighbourhoods(size):
    name = "singletons_%dx%dx%d" % size
    _, parts, solid, meta = bc.build(name)
    m = bc.expected(name)
    nt = bc.tiles_of(size)
    tiles = meta["tiles"]
    assert m["particle_tiles"] == len(parts) == len(tiles) and m["tile_counts"].max() == 1
    assert np.array_equal(np.sort(m["tile"]), np.sort(tiles[:, 0] + nt[0] * (tiles[:, 1] + nt[1] * tiles[:, 2])))
    # the union of the clipped 27-neighbourhoods, tile by tile
    near = set()
    for t in tiles.tolist():
        for d in np.ndindex(3, 3, 3):
            q = tuple(t[a] + d[a] - 1 for a in range(3))
            if all(0 <= q[a] < nt[a] for a in range(3)):
                near.add(q)
    assert m["processed_tiles"] == len(near)
    if size == (24, 40, 56):
        assert nt == (3, 5, 7) and len(tiles) == 8 + 12 + 1
        sizes = sorted(sum(all(0 <= t[a] + d[a] - 1 < nt[a] for a in range(3)) for d in np.ndindex(3, 3, 3)) for t in tiles.tolist())
        assert sizes == [8] * 8 + [12] * 12 + [27]
        # together the 21 neighbourhoods cover the grid, so a neighbour one tile fails to mark is marked by another: the GPU test
        # also bins every particle ALONE (bc.lone), where the model counts 8, 12 or 27 processed tiles
        assert m["processed_tiles"] == 105 == nt[0] * nt[1] * nt[2]
        lone = [bc.model_of(bc.lone(bc.build(name), i)) for i in range(len(parts))]
        assert sorted(x["processed_tiles"] for x in lone) == sizes and all(x["particle_tiles"] == 1 for x in lone)
    else:
        assert any(s % 8 for s in size) and m["processed_tiles"] == nt[0] * nt[1] * nt[2]
        assert (np.asarray(size) - 1).tolist() in meta["cell"].tolist()  # the far corner cell of the cut tile


@pytest.mark.parametrize("nt", sorted(bc.SCAN_GRIDS))
def test_scan_tiles_lengths_and_forms(nt):
    name = f"scan_tiles_nt{nt}"
    size, parts, solid, meta = bc.build(name)
    m = bc.expected(name)
    assert bc.SCAN_TILE == 2048 and bc.SCAN_SERIAL_MAX == 8192  # core.hip:31, core.hip:93
    assert len(m["tile_counts"]) == nt and max(size) <= 4096
    assert (bc.scan_form(nt + 1), bc.scan_form(nt)) == bc.SCAN_FORMS[nt]
    # the scanned arrays are not constant, and the designed tiles are occupied
    assert 0.4 * nt < m["particle_tiles"] < 0.6 * nt and set(np.unique(m["tile_counts"])) == {0, 1, 2, 3}
    assert (m["tile_counts"][meta["forced"]] > 0).all() and {0, nt - 1} <= set(meta["forced"])
    for b in range(bc.SCAN_TILE, nt + 1, bc.SCAN_TILE):
        assert b - 1 in meta["forced"] and (b == nt or b in meta["forced"])
    assert len(np.unique(m["tile"][:64])) > 32  # uploaded in no order


def test_scan_forms_on_their_boundaries():
    """scan_rec (core.hip:118-138) restated: the lengths at which it changes its form."""
    assert [bc.scan_form(n) for n in (0, 1, 2047, 2048, 2049, 8191, 8192, 8193)] == \
        ["none", "local", "local", "local", "serial", "serial", "serial", "reduce+local"]
    assert bc.scan_form(2048 * 2048) == "reduce+local" and bc.scan_form(2048 * 2048 + 1) == "reduce+serial"
    assert bc.scan_form(2048 * 8192) == "reduce+serial" and bc.scan_form(2048 * 8192 + 1) == "reduce+reduce+local"
    lengths = sorted({n for nt in bc.SCAN_GRIDS for n in (nt, nt + 1)})
    assert lengths == [2046, 2047, 2048, 2049, 8190, 8191, 8192, 8193]
    assert all(8191 % p for p in range(2, 91))  # prime: no grid has 8 191 tiles


def test_scan_recursion_scans_more_than_2048_blocks():
    size, parts, solid, meta = bc.build("scan_recursion")
    m = bc.expected("scan_recursion")
    nc = size[0] * size[1] * size[2]
    assert meta["scanned"] == nc == len(m["counts"]) == 4300800 > 2048 * 2048
    assert bc.scan_form(nc) == "reduce+serial" and -(-nc // bc.SCAN_TILE) == 2100
    assert bc.scan_form(len(m["tile_counts"]) + 1) == "reduce+local" and len(m["tile_counts"]) == 8400
    flags = m["counts"] > 0
    k = np.arange(1, 2100) * bc.SCAN_TILE
    assert flags[0] and flags[nc - 1] and flags[k - 1].all() and flags[k].all()
    assert set(np.unique(m["counts"])) >= {0, 1, 2} and 6000 < flags.sum() == len(m["fluid_cells"]) < 8000
    per_block = np.add.reduceat(flags.astype(np.int64), np.arange(0, nc, bc.SCAN_TILE))
    assert len(np.unique(per_block)) >= 4 and per_block[:2048].sum() < flags.sum()  # the inner scan's second tile adds a carry


def test_with_solids_counts_and_lists_particles_in_solid_cells():
    size, parts, solid, meta = bc.build("with_solids")
    m = bc.expected("with_solids")
    mask = np.zeros(size[0] * size[1] * size[2], dtype=bool)
    mask[solid[:, 0] + size[0] * (solid[:, 1] + size[1] * solid[:, 2])] = True
    inside = mask[m["raw"].astype(np.int64)]
    assert inside[meta["inside"]].all() and 80 <= inside.sum() < len(parts) - 80
    assert m["counts"][mask].sum() == inside.sum()
    in_list = np.isin(m["raw"], m["fluid_cells"])
    assert in_list.all()  # the oracle and the reference agree (test_model_is_the_*): _fluid_cells does not look at cell types
    assert len(m["fluid_not_solid"]) == len(m["fluid_cells"]) - len(np.unique(m["raw"][inside])) < len(m["fluid_cells"])


# ------------------------------------------------------------------------------------------- the time step's binning
@pytest.mark.parametrize("name", [n for n in bc.ROUND_ROBIN if "stride" not in n])
def test_round_robin_with_moves_is_isolated(name):
    """The oracle's own time_step ends every particle at its clamped free flight: at least 2 cells apart before and after, the
    position correction moves none (1e-9 h: the clamp bounds are not dyadic). Some particles change tiles."""
    cloud, dt = bc.with_moves(bc.build(name))
    size, parts, solid, meta = cloud
    a, b, clamped = mc.free_flight(dict_cloud(cloud))
    for x in (a, clamped):
        for r0 in range(0, len(x), 512):  # largest coordinate difference of every pair, 512 rows at a time
            d = np.abs(x[r0:r0 + 512, None, :] - x[None, :, :]).max(axis=2)
            d[np.arange(len(d)), r0 + np.arange(len(d))] = 9.0
            assert d.min() > 2.0
    got = mc.run_cpu_time_step(dict_cloud(cloud))
    assert np.abs(mc.cells_of(got, meta) - clamped).max() < 1e-9
    before = bc.model(size, parts["pos"], meta["h"], meta["off"])["tile"]
    after = bc.model(size, got, meta["h"], meta["off"])["tile"]
    assert 0 < np.count_nonzero(before != after) < len(parts) // 4


def dict_cloud(cloud):
    """The cloud as tests/move_cases.py takes it (meta with h, off, dt and the wall skin in cells)."""
    size, parts, solid, meta = cloud
    return size, parts, solid, dict(meta, skin=mc.SKIN_WORLD / meta["h"])
