"""CPU tests of tests/correction_output_cases.py: the oracle is the reference on exactly these inputs, the all-pairs fp64
restatement agrees with both, and every case holds what it is there for - counted with the numpy restatement of the half-cell index
and block of tests/correction_halfcell_cases.py (layout: rows of 26 half cells)."""
import numpy as np
import pytest

from oracle import loader as orc
from tests import correction_cases as cc
from tests import correction_halfcell_cases as hc
from tests import correction_output_cases as oc
from tests.correction_cases import FB, FINE_CAP, FINE_CAP_BIG, FT, FT_PL

FBX = hc.FBX


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name", oc.NAMES)
def test_oracle_is_the_reference_on_the_output_clouds(name):
    cloud = oc.build(name)
    want, got = cc.run_cpu(cloud, "ref"), oc.oracle(name)
    for k in ("correct", "collide"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * cloud[3]["h"], k


@pytest.mark.parametrize("name", oc.NAMES)
def test_brute_force_is_the_oracle(name):
    cloud = oc.build(name)
    assert len(cloud[1]) <= 16000
    brute = cc.brute_rows(cloud, np.arange(len(cloud[1])))
    assert np.abs(brute - oc.oracle(name)["correct"]).max() <= 1e-12 * cloud[3]["h"]


@pytest.mark.parametrize("name", oc.NAMES)
def test_inputs_are_exact_in_fp32_and_the_grids_are_small(name):
    size, parts, solid, meta = oc.build(name)
    assert size in ((17, 17, 17), (24, 17, 17)) and solid is None and meta["h"] == 1.0 and meta["off"] == (0.0, 0.0, 0.0)
    assert np.array_equal(parts["pos"], meta["q"] / cc.Q)
    assert (meta["q"] >= 0).all() and (meta["q"] <= np.asarray(size) * cc.Q).all()
    cell = np.minimum(meta["q"] // cc.Q, np.asarray(size) - 1)
    t = (meta["q"] - cell * cc.Q) / cc.Q
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t)


@pytest.mark.parametrize("name", oc.NAMES)
def test_most_particles_move_by_many_bars(name):
    """A record that is not written leaves the particle where it was: that has to show."""
    cloud = oc.build(name)
    moved = np.abs(oc.oracle(name)["collide"] - cloud[1]["pos"]).max(axis=1)
    alone = [i for g in cloud[3]["groups"] if g.get("kind") == "alone" for i in g["ids"]]
    keep = np.ones(len(moved), dtype=bool)
    keep[alone] = False
    print(name, "moved by less than 20 bars:", int((moved[keep] < 20 * cc.FLAT_BAR).sum()), "of", int(keep.sum()))
    # (all but the particle on the max face, which is pushed outwards and clamped back, and a few of a dense tile whose springs cancel)
    assert (moved[keep] >= 20 * cc.FLAT_BAR).mean() >= 0.85
    assert (moved[alone] == 0).all()


def test_empty_part_owns_nothing_and_still_stages():
    cloud = oc.build("empty_part")
    own, staged, lay = oc.own_counts(cloud), oc.staged(cloud), hc.layout(cloud)
    assert oc.tile_counts(cloud) == {oc.EMPTY_PART_TILE: 8 * 8 * 8 * 4}
    assert own == {(oc.EMPTY_PART_TILE, 0): 2048}  # part 1 owns no particle
    assert 0 < staged[(oc.EMPTY_PART_TILE, 1)] < staged[(oc.EMPTY_PART_TILE, 0)] == 2048
    counts = lay[(oc.EMPTY_PART_TILE, 1)]  # rows r = by + 13 bz: only block layer 0 (fine layer FT_PL - 1) holds records
    assert counts[FB:].sum() == 0 and counts[:FB, 2:FBX - 2].sum() == staged[(oc.EMPTY_PART_TILE, 1)]


def test_window_tiles_hold_exactly_the_window_and_one_more():
    cloud = oc.build("window")
    assert oc.WINDOW == 4224
    assert oc.tile_counts(cloud) == {oc.WINDOW_TILES[0]: oc.WINDOW, oc.WINDOW_TILES[1]: oc.WINDOW + 1}
    staged = oc.staged(cloud)
    assert len(staged) == 4 and max(staged.values()) <= FINE_CAP
    assert hc.prediction(cloud) == (set(), set())
    own = oc.own_counts(cloud)
    assert all(own[(t, 0)] > 0 and own[(t, 1)] > 0 for t in oc.WINDOW_TILES)


def test_second_pass_takes_the_crowded_tile_only():
    cloud = oc.build("second_pass")
    staged = oc.staged(cloud)
    second, gather = hc.prediction(cloud)
    assert gather == set() and second and all(t == oc.CROWD_TILE for t, part in second)
    assert all(FINE_CAP < staged[k] <= FINE_CAP_BIG for k in second)
    assert all(0 < staged[(oc.NORMAL_TILE, part)] <= FINE_CAP for part in (0, 1))
    assert oc.tile_counts(cloud) == {oc.CROWD_TILE: 18 * 512, oc.NORMAL_TILE: 8 * 512}


def test_second_pass_spread_mixes_the_two_orders_of_work_items():
    cloud = oc.build("second_pass_spread")
    counts = oc.tile_counts(cloud)
    assert len(counts) == 10 and len(counts) % 8 != 0 and len(counts) > 8  # eight tiles in the paired order, two in the plain one
    assert all(counts[t] == 2 for t in oc.SPREAD_TILES)
    raw = sorted(t[0] + 3 * (t[1] + 3 * t[2]) for t in counts)  # 3 x 3 x 3 tiles, in the order of their raw index
    assert raw.index(0) < 8  # the crowded tile is among the first eight
    # the pairs change nothing for the dense tiles: the same parts go to the second pass
    assert hc.prediction(cloud) == hc.prediction(oc.build("second_pass"))
    assert {k: v for k, v in oc.staged(cloud).items() if k[0] in (oc.CROWD_TILE, oc.NORMAL_TILE)} == oc.staged(oc.build("second_pass"))


def test_last_tile_is_one_cell_wide_and_a_particle_lies_on_the_max_face():
    size, parts, solid, meta = cloud = oc.build("last_tile")
    assert size[0] == 17
    x = meta["q"][:, 0]
    kinds = {g["kind"]: [] for g in meta["groups"]}
    for g in meta["groups"]:
        kinds[g["kind"]].append(x[list(g["ids"])])
    (a, b), = kinds["max_face"]
    assert a == 17 * cc.Q and 16 * cc.Q < b < a  # on the face, partner inside the last tile
    on_face = [g for g in meta["groups"] if g["kind"] == "max_face"][0]["ids"][0]
    assert hc.fine_coords(meta["q"], size)[on_face, 0] == 2 * hc.FTX + 2  # t == 1 in cell 0 of tile 2: half cell (int)(1 * 2.75)
    (c, d), = kinds["inside"]
    assert 16 * cc.Q < c < d < 17 * cc.Q
    assert len(kinds["across"]) == 2 and all((p.min() < 16 * cc.Q < p.max()) for p in kinds["across"])
    assert {t[0] for t, part in hc.layout(cloud)} == {1, 2}  # the last tile of x and the one before it


def test_lone_tile_has_no_neighbour_on_any_side():
    cloud = oc.build("lone_tile")
    assert oc.tile_counts(cloud) == {oc.LONE_TILE: 4096}
    lay = hc.layout(cloud)
    assert set(lay) == {(oc.LONE_TILE, 0), (oc.LONE_TILE, 1)}
    for (t, part), counts in lay.items():
        nzb = hc.OWN_LAYERS[part] + 2
        rows = counts.reshape(nzb, FB, FBX)
        assert rows[:, :, :2].sum() == 0 and rows[:, :, FBX - 2:].sum() == 0        # the x-1 and x+1 runs of every row
        assert rows[:, 0].sum() == 0 and rows[:, FB - 1].sum() == 0                  # the y-1 and y+1 tiles: rows empty in a row
        assert rows[0 if part == 0 else nzb - 1].sum() == 0                          # the z-1 (part 0) / z+1 (part 1) tile
        assert rows[nzb - 1 if part == 0 else 0].sum() > 0                           # the other part's layer of the own tile
        assert (rows[1:nzb - 1, 1:FB - 1, 2:FBX - 2].sum(axis=2) > 0).all()          # every own row holds particles


def test_single_particle_tiles():
    cloud = oc.build("single")
    assert oc.tile_counts(cloud) == {(0, 0, 0): 1, (1, 0, 0): 1, (2, 1, 1): 1}
    want = oc.oracle("single")["collide"]
    moved = np.abs(want - cloud[1]["pos"]).max(axis=1)
    assert (moved[:2] > 1000 * cc.FLAT_BAR).all() and moved[2] == 0
