"""CPU tests of tests/transfer_cases.py: the clouds are what they claim to be, the oracle is the reference on exactly these
inputs (without that a device-against-oracle comparison on them proves nothing), and no face of any case lies so close to the
reference's `sum w > 1e-6` that fp32 weights could put the device on the other side."""
import numpy as np
import pytest

from oracle import loader as orc
from tests import transfer_cases as tc
from tests import util

CASE_METHODS = tc.case_methods()
IDS = [f"{n}-{tc.method_id(m)}" for n, m in CASE_METHODS]


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("name,method", CASE_METHODS, ids=IDS)
def test_oracle_is_the_reference_on_the_adversarial_clouds(name, method):
    want = tc.staged(name, method, "ref")
    got = tc.oracle_stages(name, method)
    assert set(got) == set(want)
    for k in sorted(want):
        if np.asarray(want[k]).dtype.kind in "iu":
            assert np.array_equal(got[k], want[k]), k
        else:
            util.assert_close(got[k], want[k], 1e-13, f"{name}:{k}", atol=1e-300)


@pytest.mark.parametrize("name,method", CASE_METHODS, ids=IDS)
def test_no_face_weight_within_the_band_around_the_threshold(name, method):
    """A condition on the inputs, not a measurement: fp32 weights carry a relative error of a few 2^-24, so with no fp64 weight sum
    inside 1e-6 (1 +- 1e-3) the device and the reference decide `sum w > 1e-6` alike for EVERY face - none is excluded from any
    comparison. And the oracle's zero faces are exactly the faces below the threshold."""
    size, parts, solid, meta = tc.build(name)
    sw = tc.face_weight_sums(size, parts, meta["h"], meta["off"], method)
    lo, hi = tc.W_MIN * (1.0 - tc.BAND), tc.W_MIN * (1.0 + tc.BAND)
    assert not ((sw >= lo) & (sw <= hi)).any(), f"{int(((sw >= lo) & (sw <= hi)).sum())} faces in the band: pick another seed"
    vel = tc.oracle_stages(name, method)["p2g_vel"]
    if method == tc.APIC:  # (APIC zeroes the faces on the max walls whatever their weight, src/simulation.cpp:428-445)
        nx, ny, nz = size
        raw = np.arange(nx * ny * nz)
        wall = np.stack([raw % nx == nx - 1, (raw // nx) % ny == ny - 1, raw // (nx * ny) == nz - 1], axis=1)
        sw = np.where(wall, 0.0, sw)
    assert not vel[sw < lo].any()
    # (a face above the threshold is non-zero unless its velocities cancel: with random velocities, never exactly)
    assert (vel[sw > hi] != 0.0).all()


def test_tile_counts_hold_the_counts_they_promise():
    for deferred in (False, True):
        size, parts, solid, meta = tc.tile_counts(tc.TILE_COUNTS, deferred)
        tile = np.floor(parts["pos"] / 8).astype(int)
        for (t, n) in meta["per_tile"]:
            assert int((tile == np.array(t)).all(axis=1).sum()) == n
        assert sorted(n for _, n in meta["per_tile"]) == sorted(tc.TILE_COUNTS) and len(parts) == sum(tc.TILE_COUNTS)
        assert (np.array(size) // 8).prod() > len(tc.TILE_COUNTS)  # some tiles beside them hold nothing


def test_contrast_puts_sparse_and_crowded_cells_side_by_side():
    for name in ("contrast_21_13_18", "contrast_9_8_7"):
        size, parts, solid, meta = tc.build(name)
        counts = tc.oracle_stages(name, tc.PIC)["counts"]
        assert set(np.unique(counts)) == {0, 1, 2, 8, 33, 64}
        assert any(s % 8 for s in size)


def test_lattice_covers_faces_centres_and_tile_corners():
    size, parts, solid, meta = tc.build("lattice")
    two = parts["pos"] * 2.0
    assert np.array_equal(two, np.round(two))
    for a in range(3):
        assert parts["pos"][:, a].min() == 0.0 and parts["pos"][:, a].max() == size[a]
    cell = np.minimum(parts["pos"].astype(int), np.array(size) - 1)
    have = {tuple(c) for c in cell}
    tiles = {tuple(t) for t in cell // 8}
    last = [min(8, size[a] - 8 * meta["ragged_tile"][a]) - 1 for a in range(3)]
    for key, hi in (("interior_tile", (7, 7, 7)), ("ragged_tile", last), ("lonely_tile", (7, 7, 7))):
        t = np.array(meta[key])
        for corner in np.ndindex(2, 2, 2):
            assert tuple(t * 8 + np.array(corner) * np.array(hi)) in have, (key, corner)
    around = lambda t: {tuple(np.array(t) + np.array(o)) for o in np.ndindex(3, 3, 3)} - {tuple(np.array(t) + 1)}
    ntile = -(-np.array(size) // 8)
    inside = lambda ts: {t for t in ts if all(0 <= t[a] < ntile[a] for a in range(3))}
    assert around(np.array(meta["interior_tile"]) - 1) <= tiles
    assert not (inside(around(np.array(meta["lonely_tile"]) - 1)) & tiles)
    assert any(size[a] % 8 for a in range(3))


@pytest.mark.parametrize("name", ["lone_hats", "lone_hats_h17", "lone_hats_h17_unscaled"])
def test_lone_hats_put_the_prescribed_weight_on_their_face(name):
    size, parts, solid, meta = tc.build(name)
    nx, ny, nz = size
    cells = np.floor((parts["pos"] - np.array(meta["off"])) / meta["h"])
    d = np.abs(cells[:, None, :] - cells[None, :, :]).max(axis=2)
    assert d[~np.eye(len(parts), dtype=bool)].min() >= 3
    assert {(h["target"], h["kept"]) for h in meta["hats"]} == set(tc.LONE_TARGETS)
    for method in meta["methods"]:
        sw = tc.face_weight_sums(size, parts, meta["h"], meta["off"], method)
        vel = tc.oracle_stages(name, method)["p2g_vel"]
        for hat in meta["hats"]:
            x, y, z = hat["cell"]
            raw = x + nx * (y + ny * z)
            assert abs(sw[raw, hat["comp"]] - hat["target"]) <= 0.01 * hat["target"], hat
            assert (vel[raw, hat["comp"]] != 0.0) == hat["kept"], hat


def test_fast_scales_with_vmax_and_thin_grids_are_thin():
    a, b = tc.fast(1.0)[1], tc.fast(1000.0)[1]
    assert np.array_equal(a["pos"], b["pos"]) and np.abs(b["vel"]).max() <= 1000.0 and np.abs(b["vel"]).max() > 990.0
    assert np.allclose(b["vel"], a["vel"] * 1000.0, rtol=1e-15) and np.allclose(b["cx"], a["cx"] * 1000.0, rtol=1e-15)
    size = (9, 8, 7)
    m_pic, m_apic = tc.max_single_wv(size, b, method=tc.PIC), tc.max_single_wv(size, b, method=tc.APIC)
    assert 500.0 < m_pic <= 1000.0 and m_pic < m_apic <= 2000.0
    for name in ("thin_2_9_17", "thin_17_2_9", "thin_5_5_5"):
        size, parts, solid, meta = tc.build(name)
        assert min(size) in (2, 5) and max(size) <= 17
        assert (parts["pos"] >= 0).all() and (parts["pos"] <= np.array(size)).all()
        on_half = (parts["pos"] * 2 == np.round(parts["pos"] * 2)).all(axis=1)
        assert on_half.sum() > 10
