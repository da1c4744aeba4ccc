"""CPU tests of tests/correction_row_cases.py: the oracle is the reference on exactly these inputs, the all-pairs fp64 restatement
agrees with both, the inputs are dyadic, and every case holds what it is there for - counted with a numpy restatement of the
block layout (correction_row_cases.layout: rows (by, bz) of the 13 x 13 x (own layers + 2) block, records per row and segment)."""
import numpy as np
import pytest

from oracle import loader as orc
from tests import correction_cases as cc
from tests import correction_row_cases as rc


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_is_the_reference_on_the_row_clouds(name):
    cloud = rc.build(name)
    want, got = cc.run_cpu(cloud, "ref"), rc.oracle(name)
    for k in ("correct", "collide"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * cloud[3]["h"], k


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name", rc.ISOLATED)
def test_oracle_time_step_is_the_reference_on_the_isolated_clouds(name):
    cloud = rc.build(name)
    assert np.abs(rc.oracle_time_step(name) - rc.run_cpu_time_step(cloud, "ref")).max() <= 1e-13 * cloud[3]["h"]


@pytest.mark.parametrize("name", rc.NAMES)
def test_brute_force_is_the_oracle_and_the_reference(name):
    cloud = rc.build(name)
    assert len(cloud[1]) <= 12500
    brute = cc.brute_rows(cloud, np.arange(len(cloud[1])))
    assert np.abs(brute - rc.oracle(name)["correct"]).max() <= 1e-12 * cloud[3]["h"]
    if orc.have_ref():
        assert np.abs(brute - cc.run_cpu(cloud, "ref")["correct"]).max() <= 1e-12 * cloud[3]["h"]


@pytest.mark.parametrize("name", rc.NAMES)
def test_inputs_are_dyadic_and_small(name):
    size, parts, solid, meta = rc.build(name)
    assert max(size) <= 24 and solid is None and meta["h"] == 1.0 and meta["off"] == (0.0, 0.0, 0.0)
    assert (meta["q"] % cc.U == 0).all()
    assert np.array_equal(parts["pos"], meta["q"] / cc.Q)  # exact: multiples of 2^-16 below 32
    assert (meta["q"] > 0).all() and (meta["q"] < np.asarray(size) * cc.Q).all()


@pytest.mark.parametrize("name", rc.ISOLATED)
def test_groups_are_isolated_and_every_partner_is_worth_a_hundred_bars(name):
    """Nothing but a group's own particles within 2 cells (Chebyshev); leaving one designed partner out moves a particle by at
    least 100 bars."""
    cloud = rc.build(name)
    size, parts, solid, meta = cloud
    c = meta["q"] / cc.Q
    group = np.empty(len(c), dtype=np.int64)
    for k, g in enumerate(meta["groups"]):
        group[list(g["ids"])] = k
    d = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2)
    assert d[group[:, None] != group[None, :]].min() >= 2.0
    i, j = np.concatenate([meta["pairs"], meta["pairs"][:, ::-1]]).T
    worth = np.abs(cc.brute_rows(cloud, i) - cc.brute_rows(cloud, i, skip=j)).max(axis=1)
    print(name, "the least a designed partner is worth:", worth.min() / cc.FLAT_BAR, "bars")
    assert worth.min() >= 100 * cc.FLAT_BAR


def test_sparse_rows_spans_many_rows_per_wave_with_runs_of_empty_rows():
    cloud = rc.build("sparse_rows")
    lay = rc.layout(cloud)
    assert (0, 0, 0) in {t for t, _ in lay} and (2, 1, 2) in {t for t, _ in lay}  # the grid's corner tiles (21 x 13 x 24: ragged)
    assert cloud[0] == (21, 13, 24)
    for part, rows in ((0, 48), (1, 42)):  # both part sizes: 6 and 5 own layers
        counts = lay[(rc.SPARSE_TILE, part)]
        per_row = counts.sum(axis=1)
        assert len(per_row) == rc.FB * (rc.OWN_LAYERS[part] + 2)
        assert (per_row > 0).sum() == rows >= 40 and per_row.max() <= 2
        first, last = rc.wave_spans(counts)[0]
        assert last - first > 32                       # 64 consecutive slots span more than 32 rows
        assert max(rc.empty_runs(counts)) >= 3         # several empty rows in a row
        only_lo = (counts[:, 0] > 0) & (counts[:, 1] == 0) & (counts[:, 2] == 0)
        only_hi = (counts[:, 2] > 0) & (counts[:, 1] == 0) & (counts[:, 0] == 0)
        assert only_lo.sum() >= 6 and only_hi.sum() >= 6  # rows with records in the x-1 segment only, in the x+1 segment only
        assert rc.own_count(counts, part) > 0
    one = [(k, v) for k, v in lay.items() if (v.sum(axis=1) > 0).sum() == 1 and rc.own_count(v, k[1]) == v.sum() == 2]
    assert one and one[0][0][0] == (0, 1, 2)           # a part whose whole block is one row
    kinds = [g["kind"] for g in cloud[3]["groups"]]
    assert kinds.count("rows") == 39 and kinds.count("corner_low") == kinds.count("corner_high") == 1


def test_sparse_rows_ends_stages_the_first_and_the_last_row_and_nothing_between():
    lay = rc.layout(rc.build("sparse_rows_ends"))
    per_row = lay[((1, 1, 1), 1)].sum(axis=1)
    assert len(per_row) == 91 and per_row[0] == 2 and per_row[-1] == 2 and per_row[1:-1].sum() == 0  # 89 empty rows between
    assert rc.wave_spans(lay[((1, 1, 1), 1)]) == [(0, 90)]
    assert lay[((1, 1, 1), 0)].sum() > 0 and rc.own_count(lay[((1, 1, 1), 0)], 0) == 2  # the tile is a work item


def test_long_rows_holds_whole_waves_inside_one_row_and_a_part_for_the_second_pass():
    cloud = rc.build("long_rows")
    assert len(cloud[1]) <= 12500
    lay = rc.layout(cloud)
    small = lay[(rc.LONG_SMALL, 0)]
    per_row = small.sum(axis=1)
    r = int(per_row.argmax())
    assert per_row[r] >= 192 and per_row[r - 1] == 0 and per_row[r + 1] == 1 and per_row.sum() == per_row[r] + 1 <= rc.FINE_CAP
    assert any(a == b == r for a, b in rc.wave_spans(small))  # a wave whose 64 slots lie in the one row
    big = lay[(rc.LONG_BIG, 0)]
    per_row = big.sum(axis=1)
    assert rc.FINE_CAP < per_row.sum() <= rc.FINE_CAP_BIG
    assert (per_row == 0).sum() >= 20 and per_row.max() >= 192 and max(rc.empty_runs(big)) >= 3
    assert 0 < rc.own_count(big, 0) <= rc.LIST_MAX_BIG  # (the second pass lists them: the descriptors' own-list bases are used)
    assert all(v.sum() <= rc.FINE_CAP for k, v in lay.items() if k != (rc.LONG_BIG, 0))
    second, gather = rc.prediction(cloud)
    assert second == {(rc.LONG_BIG, 0)} and gather == set()
    assert cc.min_distance(cloud[3]["q"]) >= cloud[3]["min_dist"]


@pytest.mark.parametrize("name,axis,across", [("wall_reach_x", 0, 9), ("wall_reach_y", 1, 9), ("wall_reach_thin_x", 0, 24),
                                              ("wall_reach_thin_y", 1, 24), ("wall_reach_thin_z", 2, 24)])
def test_wall_reach_pushes_into_the_skin_of_the_wall_from_the_middle_tile(name, axis, across):
    """P starts in cell 15 - tile 1 of 3 on its axis -, the correction alone leaves it in cell 16 with a fraction above 1 - skin, and
    the reference's collision handling pushes it back by at least 0.03 cells. In the thin grids (24 cells across) P's tile is
    (1, 1, 1): the naive rule "not in the outer tile layer" calls it interior, the kernel's rule by cells does not."""
    size, parts, solid, meta = rc.build(name)
    assert size[axis] == 17 and sorted(size) == sorted([across, across, 17])
    assert -(-size[axis] // 8) == 3
    (g,) = rc.groups_of(name, "into_last_cell")
    tile = tuple(int(c) // 8 for c in parts["pos"][g["ids"][0]])
    naive, by_cells = rc.tile_rules(size, tile)
    assert all(int(parts["pos"][i, a]) // 8 == tile[a] for i in g["ids"] for a in range(3))  # the whole junction in one tile
    assert not by_cells and naive == (across == 24)
    if across == 24:
        assert tile == (1, 1, 1)
    want = rc.oracle(name)
    ref = cc.run_cpu(rc.build(name), "ref") if orc.have_ref() else want
    (g,) = rc.groups_of(name, "into_last_cell")
    p = g["ids"][0]
    start, moved = parts["pos"][p, axis], want["correct"][p, axis]
    assert 15.0 < start < 16.0 and 16.0 + (1.0 - meta["skin"]) + 0.03 <= moved < 17.0
    for out in (want, ref):
        assert out["correct"][p, axis] - out["collide"][p, axis] >= 0.03
        assert abs(out["collide"][p, axis] - (17.0 - meta["skin"])) <= 1e-12
    for g in rc.groups_of(name, "control"):  # the same push, no wall within reach
        p = g["ids"][0]
        assert 0.9 < abs(want["correct"][p, axis] - parts["pos"][p, axis]) < 1.1
        assert np.array_equal(want["collide"][p], want["correct"][p])
    assert len(rc.groups_of(name, "control")) == 2


def test_wall_reach_low_pushes_towards_the_low_walls_and_reaches_none():
    size, parts, solid, meta = rc.build("wall_reach_low")
    want = rc.oracle("wall_reach_low")
    groups = rc.groups_of("wall_reach_low", "towards_low_wall")
    assert sorted(g["axis"] for g in groups) == [0, 1, 2]
    for g in groups:
        p, a = g["ids"][0], g["axis"]
        assert 8.0 < parts["pos"][p, a] < 9.0 and 7.0 < want["correct"][p, a] < 8.0  # from the interior tile's first cell into cell 7
    moved = np.abs(want["correct"] - parts["pos"])
    assert moved.max() < 7.0 and want["correct"].min() >= 1.0
    assert np.array_equal(want["collide"], want["correct"])  # no wall acts
    assert (parts["pos"] >= 8.0).all() and (parts["pos"] < 16.0).all()  # all of tile (1, 1, 1), the interior one
