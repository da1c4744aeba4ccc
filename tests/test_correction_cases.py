"""CPU tests of tests/correction_cases.py: the oracle is the reference on exactly these inputs (without that a device-against-
oracle comparison on them proves nothing), an all-pairs fp64 restatement agrees with both, the inputs are dyadic, every case holds
what it is there for - counted with a numpy restatement of the device's fine index -, and every designed partner is worth at
least 100 bars: the GPU comparison cannot pass with one of them missed."""
import numpy as np
import pytest

from oracle import loader as orc
from tests import correction_cases as cc

GROUPED = ("faces", "faces_h05", "faces_h2", "triads", "walls", "solids", "close_pairs", "close_pairs_odd")
FACES = ("faces", "faces_h05", "faces_h2")


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name", [n for n in cc.NAMES if n != "close_pairs"])
def test_oracle_is_the_reference_on_the_adversarial_clouds(name):
    """_correct_positions alone and with _detect_collisions, to 1e-13 (of a cell; positions are O(10)). close_pairs is left
    out: the reference pushes its coincident pairs apart with std::random_device."""
    cloud = cc.build(name)
    assert not len(cloud[3]["twins"]) and len(cc.build("close_pairs")[3]["twins"])
    want, got = cc.run_cpu(cloud, "ref"), cc.oracle(name)
    for k in ("correct", "collide"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * cloud[3]["h"], k


@pytest.mark.parametrize("name", [n for n in cc.NAMES if n not in ("stage_edge", "cap_edge")])
def test_brute_force_is_the_oracle(name):
    """All pairs in fp64 against the oracle's walk over 27 cells: nothing within re is outside them. Every case of at most 7 000
    particles (stage_edge and cap_edge are larger)."""
    cloud = cc.build(name)
    assert len(cloud[1]) <= cc.BRUTE_MAX and all(len(cc.build(n)[1]) > cc.BRUTE_MAX for n in ("stage_edge", "cap_edge"))
    assert np.abs(cc.brute(name) - cc.oracle(name)["correct"]).max() <= 1e-12 * cloud[3]["h"]


def close_pairs_count(q, limit):
    """How many pairs are closer than `limit` cells: a sweep along x (sorted), compared with the next particles while any of them
    is within `limit` in x."""
    c = np.asarray(q, dtype=np.float64)[np.argsort(q[:, 0], kind="stable")] / cc.Q
    count, k = 0, 1
    while k < len(c):
        d = c[k:] - c[:-k]
        if d[:, 0].min() >= limit:
            break
        count += int(((d * d).sum(axis=1) < limit * limit).sum())
        k += 1
    return count


@pytest.mark.parametrize("name", cc.NAMES)
def test_inputs_are_dyadic_and_nobody_is_closer_than_the_case_allows(name):
    size, parts, solid, meta = cc.build(name)
    h, off, q = meta["h"], np.asarray(meta["off"]), meta["q"]
    assert h in (1.0, 0.5, 2.0) and np.array_equal(off * 8, np.rint(off * 8)) and meta["skin"] == 0.1 / h
    cells = (parts["pos"] - off) / h
    assert (cells >= 0).all() and (cells <= np.asarray(size)).all()
    assert np.array_equal(off + cells * h, parts["pos"])  # the round trip is exact
    frac = cells - np.floor(cells)
    assert np.array_equal(frac.astype(np.float32).astype(np.float64), frac)  # the device's fp32 fraction is the fraction
    assert np.array_equal(np.rint(parts["cx"][:, 0]), np.arange(len(parts))) and not parts["vel"].any()
    rel = cells - 8.0 * (np.floor(cells) // 8)  # tile-relative; staged as rel - 8, rel and rel + 8
    staged_exact = all(np.array_equal((rel + s).astype(np.float32).astype(np.float64), rel + s) for s in (-8.0, 0.0, 8.0))
    if name == "close_pairs_odd":
        assert not staged_exact  # the one case where the rounding of the staged positions shows
    else:
        assert np.array_equal(cells * cc.Q, q) and staged_exact
        if meta["q_bits"] == 16:
            assert not (q % cc.U).any()
    # distances
    if name in GROUPED:
        group = np.full(len(parts), -1)
        for k, g in enumerate(meta["groups"]):
            group[list(g["ids"])] = k
        assert (group >= 0).all()
        cheb = np.abs(cells[:, None, :] - cells[None, :, :]).max(axis=2)
        other = group[:, None] != group[None, :]
        assert cheb[other].min() >= 2.0, cheb[other].min()
        i, j = meta["pairs"].T
        d = np.sqrt(((cells[i] - cells[j]) ** 2).sum(axis=1))
        assert (d >= cc.D_MIN - 1e-12).all() and (d <= cc.D_MAX).all(), (d.min(), d.max())
        assert (cc.CORR * cc.kernel(d) >= 0.02).all()
        if not name.startswith("close_pairs"):  # every pair inside a group is a designed one
            assert len(meta["pairs"]) == sum(len(g["ids"]) * (len(g["ids"]) - 1) // 2 for g in meta["groups"])
    else:
        assert meta["min_dist"] >= 2.0 ** -4 and close_pairs_count(q, meta["min_dist"]) == 0


def local_fine(q, axis):
    return cc.fine_coords(q)[:, axis] % cc.FT


@pytest.mark.parametrize("name", FACES)
def test_faces_holds_every_boundary_in_every_orientation_and_mirrored(name):
    size, parts, solid, meta = cc.build(name)
    q, groups = meta["q"], meta["groups"]
    tile = q // (8 * cc.Q)
    seen = {}
    for g in groups:
        i, j = g["ids"]
        key = (g["kind"], g["axis"])
        seen.setdefault(key, []).append(g)
        a = g["axis"]
        if g["kind"].startswith("fine"):
            k = int(g["kind"][4:])
            f = local_fine(q[[i, j]], a)
            assert tile[i, a] == tile[j, a] and f.min() <= k - 1 < k <= f.max()
            if not g["e"]:  # the first end within 2^-16 of the face 8 k / 11
                x = q[i, a] % (8 * cc.Q)
                assert abs(x / cc.Q - 8.0 * k / cc.FT) < 2.0 ** -16 and f[0] == (k if g["mirror"] else k - 1)
        elif g["kind"] in ("tile", "partial"):
            assert tile[i, a] != tile[j, a]
            assert (tile[i, a] > tile[j, a]) == g["mirror"]
        elif g["kind"] == "cell":
            assert tile[i, a] == tile[j, a] and q[i, a] // cc.Q != q[j, a] // cc.Q
        elif g["kind"] == "edge":
            assert all(tile[i, b] != tile[j, b] for b in a)
        elif g["kind"] == "corner":
            assert (tile[i] != tile[j]).all()
        elif g["kind"] == "zpart_side":
            f = local_fine(q[[i, j]], 2)
            assert f[0] == (cc.FT_PL if g["mirror"] else cc.FT_PL - 1)  # within 2^-16 of the boundary between the parts
            assert (f >= cc.FT_PL).all() or (f < cc.FT_PL).all()
            assert abs((q[i, 2] % (8 * cc.Q)) / cc.Q - 8.0 * cc.FT_PL / cc.FT) < 2.0 ** -16
        elif g["kind"] == "inside_partial":
            assert tile[i, a] == tile[j, a] == (size[a] - 1) // 8 and size[a] % 8
        else:
            raise AssertionError(g["kind"])
    for a in range(3):
        for k in range(1, cc.FT):
            gs = seen[(f"fine{k}", a)]
            assert {(g["e"], g["mirror"]) for g in gs} == {(0, False), (0, True), (0.2, False), (0.2, True)}
        fine = [g for k in range(1, cc.FT) for g in seen[(f"fine{k}", a)]]
        assert {g["orient"] for g in fine} == {"axis", "face", "body"}
        assert {g["mirror"] for g in seen[("cell", a)]} == {False, True}
    assert {(0, "tile"), (2, "tile"), (0, "partial"), (1, "partial")} <= {(a, k) for k, a in seen}
    for kind in ("tile", "partial", "zpart_side", "inside_partial"):
        gs = [g for (k, a), v in seen.items() if k == kind for g in v]
        assert {g["orient"] for g in gs} == {"axis", "face", "body"} and {g["mirror"] for g in gs} == {False, True}, kind
    # tile faces 8 and 16 in x and z, 8 in y; the 8 edge lines both ways; the 4 corners, one body diagonal each
    faces_at = {(g["axis"], int(max(q[g["ids"][0], g["axis"]], q[g["ids"][1], g["axis"]]) // (8 * cc.Q)) * 8)
                for g in groups if g["kind"] in ("tile", "partial")}
    assert faces_at == {(0, 8), (0, 16), (1, 8), (2, 8), (2, 16)}
    assert len(seen[("corner", None)]) == 4 and sum(len(v) for (k, a), v in seen.items() if k == "edge") == 16
    # four distinct body-diagonal lines, one per corner: each end sees its partner along one of the eight diagonal directions
    dirs = {tuple(int(x) for x in np.sign(q[g["ids"][1]] - q[g["ids"][0]])) for g in seen[("corner", None)]}
    assert len(dirs) == 4 and len(dirs | {tuple(-x for x in d) for d in dirs}) == 8
    d = np.sqrt((((q[[g["ids"][0] for g in groups]] - q[[g["ids"][1] for g in groups]]) / cc.Q) ** 2).sum(axis=1))
    for want in cc.D_SET:
        assert (np.abs(d - want) < 3e-5).sum() >= 20


def test_corner_and_edge_dumbbells_have_their_mirror_image_in_the_h05_variant():
    """A tile corner holds one dumbbell, an edge line one per diagonal: `faces` and `faces_h05` hold them both ways. Same place
    (relative to the junction), the point reflection of each other; from the FIRST id the partner lies along all eight body
    diagonals and, per pair of edge axes, all four face diagonals."""
    a, b = (cc.build(n)[3] for n in ("faces", "faces_h05"))
    first_to_second = {"corner": set(), "edge": set()}
    count = 0
    for ga, gb in zip(a["groups"], b["groups"]):
        assert ga["kind"] == gb["kind"]
        if ga["kind"] not in ("corner", "edge"):
            continue
        count += 1
        assert ga["mirror"] != gb["mirror"] and ga["axis"] == gb["axis"]
        axes = [0, 1, 2] if ga["kind"] == "corner" else list(ga["axis"])
        ra, rb = (m["q"][list(g["ids"])][:, axes] for m, g in ((a, ga), (b, gb)))
        junction = 8 * cc.Q * np.rint(ra.mean(axis=0) / (8 * cc.Q)).astype(np.int64)
        assert np.array_equal(ra - junction, -(rb - junction))
        for m, g in ((a, ga), (b, gb)):
            i, j = g["ids"]
            first_to_second[g["kind"]].add((g["axis"], tuple(int(x) for x in junction),
                                                tuple(int(x) for x in np.sign(m["q"][j] - m["q"][i]))))
    assert count == 20
    assert len({d for _, _, d in first_to_second["corner"]}) == 8
    assert len(first_to_second["edge"]) == 8 * 4  # 8 edge lines x 4 face-diagonal directions


@pytest.mark.parametrize("name", FACES)
def test_a_lone_dumbbell_moves_by_the_closed_form(name):
    """Each end moves corr (1 - d^2 / re^2)^3 away from the other, along the dumbbell."""
    size, parts, solid, meta = cc.build(name)
    cells = cc.cells_of(parts["pos"], meta)
    i, j = meta["pairs"].T
    axis = cells[i] - cells[j]
    d = np.sqrt((axis ** 2).sum(axis=1))
    want = (cc.CORR * cc.kernel(d) / d)[:, None] * axis
    got = cc.cells_of(cc.brute(name), meta)
    assert np.abs(got[i] - cells[i] - want).max() <= 1e-13 and np.abs(got[j] - cells[j] + want).max() <= 1e-13
    assert np.abs(want).max(axis=1).min() >= 0.02 / np.sqrt(3.0)


def test_triads_sit_in_different_tiles_around_their_junction():
    size, parts, solid, meta = cc.build("triads")
    q = meta["q"]
    kinds = {}
    for g in meta["groups"]:
        ids = list(g["ids"])
        tiles = {tuple(t) for t in q[ids] // (8 * cc.Q)}
        kinds.setdefault(g["kind"], []).append(len(ids))
        assert len(ids) in (3, 4) and g["sides"] >= 2
        if g["kind"] == "corner":
            assert len(tiles) == 4 == len(ids)
        elif g["kind"] == "edge":
            assert len(tiles) == len(ids)
        elif g["kind"] in ("tile", "partial"):
            assert len(tiles) == 2
        elif g["kind"].startswith("fine"):
            a, k = g["axis"], int(g["kind"][4:])
            f = local_fine(q[ids], a)
            assert len(tiles) == 1 and f.min() == k - 1 and f.max() == k
    assert len(kinds["corner"]) == 4 and sorted(kinds["edge"]) == [3] * 8 + [4] * 8
    assert len(kinds["tile"]) == 6 and len(kinds["partial"]) == 4
    assert all(len(kinds[f"fine{k}"]) == 3 for k in range(1, cc.FT))
    # an x-face junction: records of two source tiles in the same fine row of the block, one or two of each
    both = 0
    for g in meta["groups"]:
        ids = list(g["ids"])
        if len({int(t) for t in q[ids, 0] // (8 * cc.Q)}) == 2:
            rows = cc.fine_coords(q[ids])[:, 1:]
            tx = q[ids, 0] // (8 * cc.Q)
            both += any(len({int(t) for t, r in zip(tx, rows) if (r == row).all()}) == 2 for row in rows)
    assert both >= 5


def test_walls_push_against_every_face_edge_and_corner():
    size, parts, solid, meta = cc.build("walls")
    assert solid is None
    n = np.asarray(size)
    combos = {(g["kind"], g["axes"], g["lo"]) for g in meta["groups"]}
    assert sum(c[0] == "face" for c in combos) == 6 and sum(c[0] == "edge" for c in combos) == 12
    assert sum(c[0] == "corner" for c in combos) == 8
    for kind in ("face", "edge", "corner"):
        assert len({g["w"] for g in meta["groups"] if g["kind"] == kind}) == 3
    start = cc.cells_of(parts["pos"], meta)
    free, coll = (cc.cells_of(cc.oracle("walls")[k], meta) for k in ("correct", "collide"))
    outer = np.array([g["ids"][0] for g in meta["groups"]])
    clamped = ((free[outer] == 0.0) | (free[outer] == n)).any(axis=1)
    assert clamped.sum() >= 25 and (~clamped).sum() >= 5  # beyond 0 and beyond n, and some that stay inside
    assert ((free[outer] == 0.0).sum(axis=1) == 3).any() and ((free[outer] == n).sum(axis=1) == 3).any()
    skin = meta["skin"]
    at_skin = (np.abs(coll[outer] - skin) < 1e-12) | (np.abs(coll[outer] - (n - skin)) < 1e-12)
    assert at_skin.any(axis=1).sum() >= 40 and (np.abs(coll - free).max(axis=1) >= 0.02).sum() >= 40
    # z = 24 - 2^-16 in the last cell of a whole tile: l + t = 7.99998, fine cell (int)(7.99998 * 1.375) = 10
    last = meta["q"][:, 2] == 24 * cc.Q - cc.U
    assert last.any() and (cc.fine_coords(meta["q"][last], size)[:, 2] % cc.FT == 10).all()
    assert float(np.float32(8.0 - 2.0 ** -16) * np.float32(1.375)) < 11.0
    assert (start[outer].min(axis=1) < skin).sum() + ((n - start[outer]).min(axis=1) < skin).sum() >= 30


def test_solids_are_hit_and_the_controls_are_not():
    size, parts, solid, meta = cc.build("solids")
    groups = meta["groups"]
    free, coll = (cc.cells_of(cc.oracle("solids")[k], meta) for k in ("correct", "collide"))
    diff = np.abs(coll - free).max(axis=1)
    mask = cc.solid_mask(size, solid)
    tile_has = mask.reshape(3, 8, 3, 8, 3, 8).any(axis=(1, 3, 5))
    assert not tile_has[:2, :2, :2].any()  # tile (0, 0, 0) is clear
    for g in groups:
        p, partner = g["ids"]
        tile = tuple(int(t) for t in meta["q"][p] // (8 * cc.Q))
        target = np.array(g["cell"]) + np.array(g["u"])
        if g["control"]:
            assert diff[p] == 0.0 and diff[partner] == 0.0 and tile == (0, 0, 0)
            assert not mask[tuple(target)]
        else:
            assert diff[p] >= 0.02, (g, diff[p])
            assert mask[tuple(target)]
            same = tuple(target // 8) == tile
            assert same == (g["kind"] == "same_tile")
    kinds = [g["kind"] for g in groups]
    assert kinds.count("same_tile") == 26 and len({g["u"] for g in groups if g["kind"] == "same_tile"}) == 26
    assert kinds.count("tile_face") == 12 and kinds.count("tile_corner") == 1 and kinds.count("control") >= 4
    assert {g["orient"] for g in groups if g["control"]} == {"axis", "face", "body"}
    corner = next(g for g in groups if g["kind"] == "tile_corner")
    assert corner["cell"] == (15, 7, 7) and mask[16, 8, 8] and mask[16:24, 8:16, 8:16].sum() == 1
    # of the 27 tiles around its own tile (1, 0, 0) only the diagonal neighbour (2, 1, 1) holds a solid cell - that one cell:
    # a k_tile_clear that skipped corner neighbours would call the tile clear, and the short cut would miss the hit
    assert tile_has[0:3, 0:2, 0:2].sum() == 1 and tile_has[2, 1, 1] and not tile_has[1, 0, 0]
    twin = next(g for g in groups if g["control"] and g["cell"] == (7, 7, 7))
    rel = lambda g: meta["q"][list(g["ids"])] - np.array(g["cell"]) * cc.Q
    assert np.array_equal(rel(twin)[:, 1:], rel(corner)[:, 1:]) and twin["u"] == corner["u"]  # the same geometry


def test_lone_dense_tile_takes_the_unstaged_and_the_row_offset_paths():
    size, parts, solid, meta = cc.build("lone_dense_tile")
    model = cc.fine_model("lone_dense_tile")
    assert set(model) == {((1, 1, 1), 0), ((1, 1, 1), 1)} and len(parts) == 6144 > cc.FIDX_STAGE
    (own0, staged0), (own1, staged1) = model[((1, 1, 1), 0)], model[((1, 1, 1), 1)]
    print("lone_dense_tile: part 0 owns", own0, "stages", staged0, "- part 1 owns", own1, "stages", staged1)
    assert own0 + own1 == 6144
    assert cc.LIST_MAX < own0 < 3500 and staged0 <= cc.FINE_CAP and 3700 < staged0  # through the row offsets
    assert 2600 < own1 <= cc.LIST_MAX and staged1 <= cc.FINE_CAP                     # listed


def test_stage_edge_holds_the_last_staged_tile_and_the_first_unstaged():
    size, parts, solid, meta = cc.build("stage_edge")
    model = cc.fine_model("stage_edge")
    per_tile = {t: model[(t, 0)][0] + model[(t, 1)][0] for t, _ in model}
    assert per_tile == {(1, 1, 1): cc.FIDX_STAGE, (3, 3, 3): cc.FIDX_STAGE + 1}
    assert max(s for _, s in model.values()) <= cc.FINE_CAP


def test_cap_edge_switches_tiers_exactly_at_the_capacities():
    size, parts, solid, meta = cc.build("cap_edge")
    assert 25000 <= len(parts) <= 35000
    model = cc.fine_model("cap_edge")
    staged = {k: v[1] for k, v in model.items()}
    assert staged[((1, 1, 2), 0)] == cc.FINE_CAP and staged[((1, 1, 2), 1)] == cc.FINE_CAP + 1
    assert staged[((3, 3, 2), 0)] == cc.FINE_CAP_BIG and staged[((3, 3, 2), 1)] == cc.FINE_CAP_BIG + 1
    second, gather = cap_edge_prediction()
    assert second == {((1, 1, 2), 1), ((3, 3, 2), 0), ((3, 3, 2), 1)} and gather == {((3, 3, 2), 1)}
    assert len(model) == 12  # six tiles with particles: two centres, four halo tiles
    assert model[((3, 3, 2), 0)][0] > 2 * 2048  # (the second pass finds these own particles through the row offsets)


def cap_edge_prediction():
    """(parts handed to the second pass, parts handed to the gather kernel) as the model predicts them."""
    staged = {k: v[1] for k, v in cc.fine_model("cap_edge").items()}
    return {k for k, s in staged.items() if s > cc.FINE_CAP}, {k for k, s in staged.items() if s > cc.FINE_CAP_BIG}


def test_close_pairs_straddle_the_coincidence_threshold():
    size, parts, solid, meta = cc.build("close_pairs")
    q = meta["q"]
    assert meta["q_bits"] == 20 and len(meta["groups"]) == 36
    twins = meta["twins"]
    assert len(twins) == 6
    combos = set()
    for g in meta["groups"]:
        i, j, k = g["ids"]
        off = (q[i] - q[j]) / cc.Q
        d2 = float((off ** 2).sum())
        d2_f32 = np.float32(0.0)
        for o in off.astype(np.float32):
            d2_f32 = np.float32(d2_f32 + o * o)
        assert (d2 < 1e-12) == (d2_f32 < np.float32(1e-12)) == g["twin"] == (g["bits"] == 20 and not g["diag"])
        assert (i in twins) == (j in twins) == g["twin"] and k not in twins
        if g["bits"] == 19 and not g["diag"]:
            assert 3.6e-12 < d2 < 3.7e-12
        assert (np.abs(off) == 2.0 ** -g["bits"]).sum() == (3 if g["diag"] else 1)
        f = cc.fine_coords(q[[i, j, k]])
        assert (f[2] != f[0]).any() and (f[2] != f[1]).any()  # the ordinary partner lives in another fine cell
        assert abs(np.sqrt((((q[i] - q[k]) / cc.Q) ** 2).sum()) - 0.4) < 1e-6
        cell, tile = q[[i, j]] // cc.Q, q[[i, j]] // (8 * cc.Q)
        if g["kind"] == "across":
            assert (tile[0] != tile[1]).sum() == (3 if g["diag"] else 1)
        else:
            assert (cell[0] == cell[1]).all() and (cell[0] % 8 == (0 if g["kind"] == "cell0" else 7)).all()
        combos.add((g["kind"], g["diag"], g["bits"]))
    assert len(combos) == 36
    odd = cc.build("close_pairs_odd")
    assert len(odd[1]) == 3 * 18 and cc.bound("close_pairs_odd").max() > 10 * cc.FLAT_BAR
    assert cc.bound("close_pairs_odd").min() >= cc.FLAT_BAR


def partner_worth(name, pairs):
    """|brute(i) - brute(i) with partner j deleted|, in bars, for the ordered pairs (i, j)."""
    cloud = cc.build(name)
    i, j = np.asarray(pairs).T
    with_all = cc.brute_rows(cloud, i)
    without = cc.brute_rows(cloud, i, skip=j)
    return np.abs(with_all - without).max(axis=1) / (cc.FLAT_BAR * cloud[3]["h"])


@pytest.mark.parametrize("name", FACES + ("triads",))
def test_every_designed_partner_is_worth_a_hundred_bars(name):
    pairs = cc.build(name)[3]["pairs"]
    worth = partner_worth(name, np.concatenate([pairs, pairs[:, ::-1]]))
    print(f"{name}: {len(worth)} partners, the least is worth {worth.min():.0f} bars")
    assert len(worth) >= 2 * len(cc.build(name)[3]["groups"]) and worth.min() >= 100.0


@pytest.mark.parametrize("name", cc.DENSE)
def test_partners_in_the_dense_cases_are_worth_a_hundred_bars(name):
    """A sample of 200 particles, each with the FARTHEST of its partners within 0.55 cells - the one worth least."""
    size, parts, solid, meta = cc.build(name)
    rng = np.random.default_rng(1)
    rows = rng.choice(len(parts), 200, replace=False)
    cells = meta["q"] / cc.Q
    d = np.sqrt(((cells[rows][:, None, :] - cells[None, :, :]) ** 2).sum(axis=2))
    d[np.arange(200), rows] = np.inf
    d[d > cc.D_MAX] = -1.0
    far = d.argmax(axis=1)
    has = d[np.arange(200), far] > 0.0
    assert has.sum() >= 190
    worth = partner_worth(name, np.stack([rows[has], far[has]], axis=1))
    print(f"{name}: the least of {has.sum()} sampled partners is worth {worth.min():.0f} bars")
    assert worth.min() >= 100.0
