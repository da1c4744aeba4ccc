"""CPU tests of tests/correction_halfcell_cases.py: the oracle is the reference on exactly these inputs, the all-pairs fp64
restatement agrees with both, and every case holds what it is there for - counted with a numpy restatement of the half-cell index and
block (correction_halfcell_cases.half_coord, layout: rows of 26 half cells)."""
import numpy as np
import pytest

from oracle import loader as orc
from tests import correction_cases as cc
from tests import correction_halfcell_cases as hc


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name", hc.NAMES)
def test_oracle_is_the_reference_on_the_halfcell_clouds(name):
    cloud = hc.build(name)
    want, got = cc.run_cpu(cloud, "ref"), hc.oracle(name)
    for k in ("correct", "collide"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * cloud[3]["h"], k


@pytest.mark.parametrize("name", hc.NAMES)
def test_brute_force_is_the_oracle_and_the_reference(name):
    cloud = hc.build(name)
    assert len(cloud[1]) <= 16000
    brute = cc.brute_rows(cloud, np.arange(len(cloud[1])))
    assert np.abs(brute - hc.oracle(name)["correct"]).max() <= 1e-12 * cloud[3]["h"]
    if orc.have_ref():
        assert np.abs(brute - cc.run_cpu(cloud, "ref")["correct"]).max() <= 1e-12 * cloud[3]["h"]


@pytest.mark.parametrize("name", hc.NAMES)
def test_inputs_are_exact_in_fp32_and_the_grids_are_small(name):
    size, parts, solid, meta = hc.build(name)
    assert size in ((17, 9, 9), (24, 17, 17)) and solid is None and meta["h"] == 1.0 and meta["off"] == (0.0, 0.0, 0.0)
    assert np.array_equal(parts["pos"], meta["q"] / cc.Q)  # exact: multiples of 2^-20 below 32
    assert (meta["q"] >= 0).all() and (meta["q"] <= np.asarray(size) * cc.Q).all()
    cell = np.minimum(meta["q"] // cc.Q, np.asarray(size) - 1)
    t = (meta["q"] - cell * cc.Q) / cc.Q
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t)  # the device's (cell, fp32 fraction) holds them exactly


@pytest.mark.parametrize("name", hc.NAMES)
def test_two_half_cells_are_one_fine_cell_and_five_reach_every_partner(name):
    """The half cells nest in the whole fine cells (the parts stage what they staged before), and every pair closer than re lies
    within two half cells in x and one fine cell in y and z: the walk of [hx - 2, hx + 2] misses nobody."""
    cloud = hc.build(name)
    size, parts, solid, meta = cloud
    g, old = hc.fine_coords(meta["q"], size), cc.fine_coords(meta["q"], size)
    assert np.array_equal(g[:, 0] // 2, old[:, 0]) and np.array_equal(g[:, 1:], old[:, 1:])
    c = meta["q"] / cc.Q
    for lo in range(0, len(c), 1024):
        near = ((c[lo:lo + 1024, None, :] - c[None, :, :]) ** 2).sum(axis=2) < cc.RE2
        d = np.abs(g[lo:lo + 1024, None, :] - g[None, :, :])
        assert (d[near] <= np.array([2, 1, 1])).all()


@pytest.mark.parametrize("name", hc.ISOLATED)
def test_groups_are_isolated_and_the_near_partners_are_worth_a_hundred_bars(name):
    cloud = hc.build(name)
    size, parts, solid, meta = cloud
    c = meta["q"] / cc.Q
    group = np.empty(len(c), dtype=np.int64)
    for k, g in enumerate(meta["groups"]):
        group[list(g["ids"])] = k
    d = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2)
    assert d[group[:, None] != group[None, :]].min() >= 2.0
    ids = [g["ids"] for g in meta["groups"] if g["kind"] not in ("reach_in", "reach_out")]
    pairs = np.array([(a, b) for g in ids for a in g for b in g if a != b and abs(c[a, 0] - c[b, 0]) < 0.6
                      and c[a, 0] < size[0]])  # (the particle on the max face is pushed outwards and clamped back: worth nothing to it)
    worth = np.abs(cc.brute_rows(cloud, pairs[:, 0]) - cc.brute_rows(cloud, pairs[:, 0], skip=pairs[:, 1])).max(axis=1)
    print(name, "the least a near partner is worth:", worth.min() / cc.FLAT_BAR, "bars")
    assert worth.min() >= 100 * cc.FLAT_BAR


def _halves(name, g):
    size, parts, solid, meta = hc.build(name)
    return hc.fine_coords(meta["q"][list(g["ids"])], size)[:, 0]


@pytest.mark.parametrize("name", ("reach", "faces"))
def test_reach_pairs_sit_on_both_sides_of_re_and_a_partner_is_two_half_cells_away_at_the_most(name):
    size, parts, solid, meta = hc.build(name)
    want = hc.oracle(name)
    assert 0.0 < hc.RE - hc.D_IN / cc.Q < 1.5e-6 and 0.0 < hc.D_OUT / cc.Q - hc.RE < 1.5e-6
    far = []
    for g in hc.groups_of(name, "reach_in"):
        a, b = g["ids"]
        h = _halves(name, g)
        assert abs(parts["pos"][a, 0] - parts["pos"][b, 0]) < hc.RE and np.array_equal(parts["pos"][a, 1:], parts["pos"][b, 1:])
        assert abs(int(h[1]) - int(h[0])) <= 2
        far.append(abs(int(h[1]) - int(h[0])))
    assert 2 in far and (1 in far or name == "faces")  # from a half cell's far edge the partner is two away, from its near edge one
    for g in hc.groups_of(name, "reach_out"):
        a, b = g["ids"]
        assert abs(parts["pos"][a, 0] - parts["pos"][b, 0]) > hc.RE
        assert np.array_equal(want["correct"][[a, b]], parts["pos"][[a, b]])  # nobody within reach: nobody moves
    for g in hc.groups_of(name, "near2"):
        h = _halves(name, g)
        assert abs(int(h[1]) - int(h[0])) == 2 and abs(parts["pos"][g["ids"][0], 0] - parts["pos"][g["ids"][1], 0]) < 0.37


def test_reach_covers_the_edges_and_the_middle_of_a_half_cell_of_both_parities():
    size, parts, solid, meta = hc.build("reach")
    seen = set()
    for g in hc.groups_of("reach", "reach_in") + hc.groups_of("reach", "reach_out"):
        h = int(_halves("reach", g)[0]) % hc.FTX
        assert h == g["half"]
        x = parts["pos"][g["ids"][0], 0] % 8
        lo, hi = float(h * hc.W), float((h + 1) * hc.W)
        assert {"left": x - lo < 2.0 ** -15, "right": hi - x < 2.0 ** -15, "mid": abs(x - (lo + hi) / 2) < 2.0 ** -15}[g["where"]]
        seen.add((g["kind"], g["where"], g["sign"], h % 2))
    assert len(seen) == 2 * 3 * 2 * 2
    assert len(hc.groups_of("reach", "near2")) == 2


def test_faces_pairs_straddle_the_tile_faces_in_the_outer_two_half_cells():
    size, parts, solid, meta = hc.build("faces")
    assert size == (17, 9, 9)
    seen = set()
    for g in meta["groups"]:
        a, b = g["ids"]
        xa, xb = parts["pos"][a, 0], parts["pos"][b, 0]
        face = 8 * g["face"]
        assert min(xa, xb) < face <= max(xa, xb)
        h = _halves("faces", g)
        ta, tb = int(h[0]) // hc.FTX, int(h[1]) // hc.FTX
        assert abs(ta - tb) == 1
        if g["kind"] != "reach_out":
            for hh in h:
                assert int(hh) % hc.FTX in (0, 1, 20, 21)
        seen.add((g["face"], g["kind"], int(h[0]) % hc.FTX))
    for face in (1, 2):
        assert {(face, "reach_in", k) for k in (0, 1, 20, 21)} <= seen and any(s[:2] == (face, "near2") for s in seen)
    assert int(hc.fine_coords(meta["q"], size)[:, 0].max()) <= 2 * hc.FTX + 2  # the last tile: one cell, half cells 0 .. 2


def test_edges_rounding_lands_on_integral_products():
    size, parts, solid, meta = hc.build("edges")
    groups = hc.groups_of("edges", "rounding")
    assert sum(g["exact"] for g in groups) == 2 and sum(not g["exact"] for g in groups) >= 2
    for g in groups:
        q = meta["q"][g["ids"][0], 0]
        l, t = (q // cc.Q) % 8, (q % cc.Q) / cc.Q
        prod = (np.float32(l) + np.float32(t)) * np.float32(2.75)
        assert prod == np.float32(g["half"]) and int(_halves("edges", g)[0]) % hc.FTX == g["half"]
        exact = (int(l) * cc.Q + int(q % cc.Q)) * 11 == 4 * g["half"] * cc.Q
        assert exact == g["exact"]  # the others lie strictly below the face and are rounded onto it
        h = _halves("edges", g)
        assert sorted(int(x) - int(h[0]) for x in h[1:]) == [-2, 2] or sorted(int(x) - int(h[0]) for x in h[1:]) == [-2, 1]


def test_edges_max_face_is_fraction_one_in_cell_seven():
    size, parts, solid, meta = hc.build("edges")
    (g,) = hc.groups_of("edges", "max_face")
    p = g["ids"][0]
    assert parts["pos"][p, 0] == 24.0 == size[0]  # cell 23 = cell 7 of tile 2, t == 1
    h = _halves("edges", g)
    assert int(h[0]) == 2 * hc.FTX + hc.FTX - 1 and int(h[0]) - int(h[1]) == 1  # (half cell 19 is out of reach)
    want = hc.oracle("edges")
    b = g["ids"][1]
    assert want["correct"][p, 0] == 24.0 and parts["pos"][b, 0] - want["correct"][b, 0] > 0.1  # clamped to the box; the partner is pushed away


def test_edges_sparse_rows_hold_one_record_in_one_outer_half_cell():
    cloud = hc.build("edges")
    lay = hc.layout(cloud)
    seen = set()
    for part in (0, 1):
        counts = lay[(hc.SPARSE_TILE, part)]
        for r in np.flatnonzero(counts.sum(axis=1) == 1):
            bx = int(counts[r].argmax())
            if bx in hc.SPARSE_BX and hc.OWN_LAYERS[part] >= r // hc.FB >= 1 and 1 <= r % hc.FB <= hc.FT:
                seen.add(bx)
    assert seen == set(hc.SPARSE_BX)
    size, parts, solid, meta = cloud
    for g in hc.groups_of("edges", "sparse"):
        h = hc.fine_coords(meta["q"][list(g["ids"])], size)
        assert abs(int(h[0, 0]) - int(h[1, 0])) == 2 and abs(int(h[0, 1]) - int(h[1, 1])) == 1 and h[0, 2] == h[1, 2]
        assert int(h[0, 0]) // hc.FTX != 1 and int(h[1, 0]) // hc.FTX == 1  # A in a neighbour tile, B an own particle of (1, 1, 1)


def test_crowded_hands_a_part_to_the_second_pass_and_one_to_the_gather_kernel():
    cloud = hc.build("crowded")
    second, gather = hc.prediction(cloud)
    staged = {k: int(v.sum()) for k, v in hc.layout(cloud).items()}
    print("crowded: staged per part", staged, "particles", len(cloud[1]))
    assert gather == {(hc.CROWD_TILE, 0)} and second == {(hc.CROWD_TILE, 0), (hc.CROWD_TILE, 1)}
    assert staged == {k: s for k, (o, s) in _fine_model(cloud).items()}  # what the whole-cell block staged
    assert cc.min_distance(cloud[3]["q"]) >= cloud[3]["min_dist"]


def _fine_model(cloud):
    """cc.fine_model for a cloud that is no case of correction_cases: {(tile, part): (own, staged)} of the whole-cell block."""
    size, parts, solid, meta = cloud
    g = cc.fine_coords(meta["q"], size)
    out = {}
    for t in np.unique(g // cc.FT, axis=0):
        near = ((g[:, :2] >= cc.FT * t[:2] - 1) & (g[:, :2] <= cc.FT * t[:2] + cc.FT)).all(axis=1)
        own_xy = (g[:, :2] // cc.FT == t[:2]).all(axis=1)
        for part in (0, 1):
            z0 = cc.FT * t[2] + part * cc.FT_PL
            z1 = z0 + hc.OWN_LAYERS[part]
            own = own_xy & (g[:, 2] >= z0) & (g[:, 2] < z1)
            out[(tuple(int(c) for c in t), part)] = (int(own.sum()), int((near & (g[:, 2] >= z0 - 1) & (g[:, 2] <= z1)).sum()))
    return out


def test_five_half_cells_hold_fewer_candidates_than_three_whole_cells():
    """On the one dense cloud: the candidates of the new walk are a subset of the parent's, about a sixth fewer."""
    new, old = hc.candidates(_dense())
    print("candidates per particle: five half cells", new.mean(), "three whole cells", old.mean(), "ratio", new.sum() / old.sum())
    assert (new <= old).all() and 0.75 < new.sum() / old.sum() < 0.90


def _dense():
    """A uniformly filled 16 x 8 x 8 block, 8 per cell on a jittered lattice (not a case: no device run)."""
    import itertools
    rng = np.random.default_rng(79)
    cells = np.array(list(itertools.product(range(4, 20), range(4, 12), range(4, 12))))
    q = cc._fill(rng, cells, (2, 2, 2), 0.2)
    return cc._finish((24, 17, 17), q, None)
