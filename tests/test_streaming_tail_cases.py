"""The designed clouds of tests/streaming_tail_cases.py hold what they are named for (no device, no oracle: numpy alone, with the
restatements of tests/move_cases.py) - what tests/test_gpu_streaming_tails.py then runs on the device against the oracle."""
import numpy as np

from tests import move_cases as mc
from tests import streaming_tail_cases as sc


def min_distance(x):
    """Smallest Euclidean distance between two of the points."""
    e = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    np.fill_diagonal(e, np.inf)
    return float(e.min())


def test_every_cloud_has_the_property_it_is_named_for():
    # ---- lattice_n*: the counts around a wave, a chunk and a workgroup of the counting advection; nobody within reach of the
    # position correction before or after the move; both paths of the move in one wave
    assert sc.AC_CHUNKS >= 1 and sc.WAVE == 64 * sc.AC_CHUNKS
    assert {1, 63, 64, 65, 511, 512, 513} <= set(sc.COUNTS)
    assert {sc.WAVE * k + d for k in (1, 2) for d in (-1, 1)} <= set(sc.COUNTS)
    for n in sc.COUNTS:
        cloud = sc.build(f"lattice_n{n}")
        size, parts, solid, meta = cloud
        assert size == (24, 17, 17) and len(parts) == n and solid is None
        a, b, clamped = mc.free_flight(cloud)
        assert np.array_equal(b, clamped)  # no wall in the way
        if n > 1:
            assert min_distance(a) > 1.4 and min_distance(b) > 0.85 > sc.RE
        open_water = mc.open_water(cloud)
        for w in range(0, n - 63, sc.WAVE):  # every wave with at least 64 particles
            lanes = open_water[w:w + sc.WAVE]
            if len(lanes) >= 64:
                assert lanes.any() and not lanes.all(), (n, w)
        # the keys change: some particle ends in another cell, some in another tile (n large enough)
        if n >= 511:
            assert (np.floor(a) != np.floor(b)).any() and (sc.tile_of(size, a) != sc.tile_of(size, b)).any()

    # ---- the largest lattice on two slab ranks split at z = 8: to each rank the other's particles are holes, and every chunk of 64
    # consecutive uploads (every chunk position of every wave) holds holes and particles of its own; some particles change ranks
    size, parts, solid, meta = cloud = sc.build(f"lattice_n{sc.SLAB_N}")
    a, b, _ = mc.free_flight(cloud)
    split = 8 * sc.SLAB_BOUNDS[1]
    mine = a[:, 2] < split
    for c in range(0, sc.SLAB_N - 63, 64):
        assert mine[c:c + 64].any() and not mine[c:c + 64].all(), c
    assert ((a[:, 2] < split) != (b[:, 2] < split)).any()

    # ---- mixed: in every wave open-water lanes beside lanes in the plate's skin, lanes that hit it, exact 7-cell moves out of a
    # clear tile and particles on the max face
    cloud = sc.build("mixed")
    size, parts, solid, meta = cloud
    kind = np.array(meta["kind"])
    a, b, clamped = mc.free_flight(cloud)
    open_water = mc.open_water(cloud)
    n = len(parts)
    assert n > sc.WAVE and n % 64 != 0
    for w in range(0, n, sc.WAVE):
        k = kind[w:w + sc.WAVE]
        assert {"plain", "skin", "hit", "seven", "max_face"} <= set(k), (w, set(k))
        lanes = open_water[w:w + sc.WAVE]
        assert lanes.any() and not lanes.all()
        for c in range(0, len(k), 64):  # and every chunk of 64 holds lanes of both paths
            assert open_water[w + c:w + c + 64].any() and not open_water[w + c:w + c + 64].all(), (w, c)
    seven = kind == "seven"
    assert (np.abs(b - a)[seven] == (7.0, 0.0, 0.0)).all()
    # "clear" start tile, and a hair less than 7 would take the short cut: it is the 7 that sends them the long way
    shorter = parts["vel"].copy()
    shorter[seven, 0] -= 1.0 / mc.M
    assert mc.open_water(cloud, shorter)[seven].all()
    face = kind == "max_face"
    assert (a[face, 1] == size[1]).all() and (clamped[face, 1] == size[1] - meta["skin"]).all() and open_water[face].any()
    skin = kind == "skin"
    assert ((a[skin, 0] > sc.PLATE_X - meta["skin"]) & (a[skin, 0] < sc.PLATE_X)).all() and (b[skin, 0] == a[skin, 0]).all()
    hit = kind == "hit"
    assert (np.floor(b[hit, 0]) == sc.PLATE_X).all() and not open_water[skin | hit].any()
    # the model's ends (restated collision code): every particle stays farther than the correction's reach from every other
    mask = mc.solid_mask(size, solid)
    ends = np.array([mc.collide_model(size, mask, a[i], clamped[i], meta["skin"])[0] for i in range(n)])
    assert min_distance(a) > 1.0 and min_distance(ends) > 1.0
    assert (np.abs(ends[skin | hit, 0] - (sc.PLATE_X - meta["skin"])) < 1e-12).all()
    # the coercing source takes some particles of every kind but the 7-cell movers, and leaves some
    (cells, vel), _ = sc.mixed_source()
    covered = np.zeros(size, dtype=bool)
    covered[cells[:, 0], cells[:, 1], cells[:, 2]] = True
    c = np.minimum(np.floor(a).astype(np.int64), np.asarray(size) - 1)
    taken = covered[c[:, 0], c[:, 1], c[:, 2]]
    assert 50 <= taken.sum() <= n - 50 and not taken[seven].any()
    for kd in ("plain", "skin", "hit", "max_face"):
        assert taken[kind == kd].any() and not taken[kind == kd].all(), kd

    # ---- g2p_tiles: tiles of exactly 1, 255, 256, 257 and 4 097 particles - 1, one short of a round, a round, one more, and
    # sixteen rounds and one - beside tiles of none
    size, parts, solid, meta = sc.build("g2p_tiles")
    assert sc.G2P_THREADS == 256
    t = sc.tile_of(size, parts["pos"])
    per_tile = np.bincount(t[:, 0] + 5 * (t[:, 1] + 2 * t[:, 2]), minlength=20)
    assert tuple(per_tile[:5]) == (1, 255, 256, 257, 16 * sc.G2P_THREADS + 1) and not per_tile[5:].any()

    # ---- stale_leavers: more than G2P_LV_CAP leave one tile, exactly G2P_LV_CAP another, none the third - by a margin fp32 keeps
    cloud = sc.build("stale_leavers")
    size, parts, solid, meta = cloud
    a = parts["pos"]
    b = a + parts["vel"] * meta["dt"]
    t0, t1 = sc.tile_of(size, a), sc.tile_of(size, b)
    left = (t0 != t1).any(axis=1)
    assert np.array_equal(left, meta["leaves"])
    to_face = lambda x: np.abs(x - 8.0 * np.rint(x / 8.0))  # distance to the nearest tile face
    assert (to_face(a) > 0.04).all() and (to_face(b) > 0.04).all()
    lost = {tuple(k): int(left[(t0 == k).all(axis=1)].sum()) for k in np.unique(t0, axis=0)}
    assert lost == {(0, 0, 0): sc.G2P_LV_CAP + 44, (2, 0, 0): sc.G2P_LV_CAP, (4, 1, 1): 0}
    assert sorted(lost.values()) == [0, sc.G2P_LV_CAP, sc.G2P_LV_CAP + 44] and sc.G2P_LV_CAP == 256
    gone = {tuple(k) for k in np.unique(t1[left], axis=0)}
    assert gone == {(1, 0, 0), (3, 0, 0)} and not gone & {tuple(k) for k in np.unique(t0, axis=0)}
