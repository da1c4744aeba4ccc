"""CPU tests of tests/mesher_edge_cases.py: the oracle is the reference on exactly these inputs (digests and counts of what the
real reference produced, tests/golden/mesher_edges.npz, and a live oracle/_ref where it is present) - without that a
device-against-oracle comparison on them proves nothing -, every case holds what it is there for, counted with the numpy
restatement beside the cases, and no designed particle is idle: deleting it changes a sampled value.
Bit for bit throughout (NaN equals NaN); there is no tolerance in this file."""
import os

import numpy as np
import pytest

from oracle import loader as orc
from tests import mesher_edge_cases as ec
from tests.test_mesher import same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
CASES = [("cloud", c) for c in ec.CLOUD_IDS] + [("field", f) for f in ec.FIELD_IDS]
CASE_IDS = [f"{k}:{c}" for k, c in CASES]

_oracle = {}


def oracle(kind, cid):
    """(values, positions, indices) of the oracle, computed once per case."""
    if (kind, cid) not in _oracle:
        _oracle[kind, cid] = ec.results(cid, "oracle", kind == "field")
    return _oracle[kind, cid]


@pytest.fixture(scope="module")
def golden():
    """case -> (counts int64[4], digests uint8[3, 32]) of the compiled reference."""
    with np.load(os.path.join(GOLDEN, "mesher_edges.npz")) as z:
        return {str(k): (c, s) for k, c, s in zip(z["ids"], z["counts"], z["sha"])}


@pytest.fixture(scope="module")
def indices_per_case():
    """Indices the reference emits for each of the 256 cases (the single-cell fixtures of tests/golden/mesher.npz)."""
    with np.load(os.path.join(GOLDEN, "mesher.npz")) as z:
        return z["cases_counts"][:256, 1].astype(np.int64)


# ------------------------------------------------------------------------------------------- oracle == reference
@needs_ref
@pytest.mark.parametrize("kind,cid", CASES, ids=CASE_IDS)
def test_oracle_matches_live_reference(kind, cid):
    want = ec.results(cid, "ref", kind == "field")
    for a, b in zip(oracle(kind, cid), want):
        assert same(a, b)


@pytest.mark.parametrize("kind,cid", CASES, ids=CASE_IDS)
def test_oracle_matches_reference_golden(golden, kind, cid):
    counts, sha = ec.summary(*oracle(kind, cid))
    assert np.array_equal(counts, golden[f"{kind}:{cid}"][0])
    assert np.array_equal(sha, golden[f"{kind}:{cid}"][1])


def test_golden_holds_digests_and_counts_only(golden):
    assert sorted(golden) == sorted(CASE_IDS)
    with np.load(os.path.join(GOLDEN, "mesher_edges.npz")) as z:
        assert sorted(z.files) == ["counts", "ids", "sha"]
        assert z["counts"].shape == (len(CASES), 4) and z["sha"].shape == (len(CASES), 3, 32)
    assert os.path.getsize(os.path.join(GOLDEN, "mesher_edges.npz")) < 8 * 1024


@pytest.mark.parametrize("kind", ["oracle", pytest.param("ref", marks=needs_ref)])
def test_unrepresentable_coordinates_change_nothing(kind):
    """NaN, +-inf, +-1e300, +-2^31 and 2^31 - 1 in one coordinate: (int) of them is undefined in C++, x86 yields INT_MIN, the device
    saturates and turns NaN into 0 - all of which particle_cell drops. The reference itself says so."""
    a = ec.results("unrepresentable", kind)
    b = ec.results("cell_faces", kind)
    assert all(same(x, y) for x, y in zip(a, b))
    assert len(a[2]) > 0 and np.isfinite(a[0]).sum() > 100


# ------------------------------------------------------------------------------------------- what the cases hold
def sees_any(p, kw):
    return ec.weights(p, kw)[0].any(axis=1)


@pytest.mark.parametrize("cid", ["cell_faces", "cell_faces_h05"])
def test_cell_faces_holds_every_decision_on_every_axis(cid):
    p, kw = ec.cloud(cid)
    c = ec.cell_faces_coordinates(kw["size"])
    world = np.asarray(kw["grid_offset"]) + kw["cell_size"] * c
    assert len(c) == 51 and sorted(map(tuple, world)) == sorted(map(tuple, p))
    assert np.array_equal((world - np.asarray(kw["grid_offset"])) / kw["cell_size"], c)  # the quotient is exact
    assert np.array_equal(c, np.round(c / ec.Q) * ec.Q)
    t, cls = ec.particle_indices(world, kw)
    for a in range(3):
        mine, n = slice(17 * a, 17 * a + 17), kw["size"][a]
        # kept, dropped for an index 0, dropped as outside - decided by this axis alone: the other two are interior
        assert np.bincount(cls[mine], minlength=3).tolist() == [9, 5, 3]
        others = np.delete(t[mine], a, axis=1)
        assert ((others >= 2) & (others <= 4)).all()
        assert sorted(t[mine][cls[mine] == ec.KEPT][:, a]) == [1, 1, 1, 2, 2, n - 2, n - 1, n - 1, n - 1]
        assert sorted(c[mine][cls[mine] == ec.INDEX0][:, a]) == [-0.5, -ec.Q, 0.0, ec.Q, 1.0 - ec.Q]
        assert sorted(c[mine][cls[mine] == ec.OUTSIDE][:, a]) == [-1.5, n, n + ec.Q]
    # the oracle agrees about who is kept: exactly the points that see a kept particle are not 1
    assert np.array_equal(oracle("cloud", cid)[0].ravel() != 1.0, sees_any(p, kw))


def test_unrepresentable_holds_cell_faces_and_24_particles_spread_through_it():
    p, kw = ec.cloud("unrepresentable")
    q, _ = ec.cloud("cell_faces")
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(p) < 2.0 ** 31 - 1.0).all(axis=1)
    assert bad.sum() == 24 and np.array_equal(p[~bad], q)
    at = np.nonzero(bad)[0]
    assert at[0] == 0 and at[-1] == len(p) - 1 and np.diff(at).max() <= 4
    _, cls = ec.particle_indices(p, kw)
    assert (cls[bad] == ec.OUTSIDE).all() and np.bincount(cls).tolist() == [27, 15, 33]
    for a in range(3):
        col = p[bad][:, a]
        mine = col[~((np.abs(col) < 8.0))]
        assert sorted(map(repr, mine)) == sorted(map(repr, np.array(ec.UNREPRESENTABLE)))
    others = np.sort(np.where(np.abs(p[bad]) < 8.0, p[bad], 3.0), axis=1)
    assert ((others >= 2.0) & (others < 5.0)).all()


def test_kernel_edge_counts():
    p, kw = ec.cloud("kernel_edge")
    v = oracle("cloud", "kernel_edge")[0].ravel()
    n_nan, n_exact, n_finite = ec.point_census(p, kw)
    # 64 points see each site; a weight reaches: nobody at at_extent, beyond_pair and weightless; 1 point at beyond (the next one
    # along x), inside, grid_point, coincident; 2 at inside_pair
    assert (n_nan, n_exact, n_finite) == (9 * 64 - 64 - 6, 1, 6)
    assert int(np.isnan(v).sum()) == n_nan and int((v == -kw["r"]).sum()) == n_exact
    assert int((np.isfinite(v) & (v != 1.0)).sum()) == n_finite
    sees, w, sq = ec.weights(p, kw)
    assert (sees.sum(axis=1) <= 2).all() and (sees.sum(axis=0) == 64).all()  # lone: only the coincident pair shares points
    e2 = kw["particle_extent"] ** 2
    site = {s: k for k, s in enumerate(ec.KERNEL_EDGE_SITES)}
    assert sorted(sq[:, site["at_extent"]])[:3] == [e2, e2, 0.640625]  # exactly at the extent from two points, then farther
    assert (w[:, site["at_extent"]] == 0).all() and (w[:, site["beyond_pair"]] == 0).all() and (w[:, site["weightless"]] == 0).all()
    for s in ("inside", "inside_pair"):
        least = np.sort(w[:, site[s]][w[:, site[s]] > 0])[0]
        assert 1e-27 < least < 1e-26
    assert sorted(sq[:, site["beyond"]])[1] > e2 and sorted(sq[:, site["beyond_pair"]])[0] > e2
    assert sorted(sq[:, site["beyond_pair"]])[0] == sorted(sq[:, site["beyond_pair"]])[1] < e2 * (1 + 2.0 ** -28)
    first = ec.KERNEL_EDGE_SITES.index("coincident")
    assert ec.KERNEL_EDGE_SITES[first + 1] == "coincident" and np.array_equal(p[first], p[first + 1])


@pytest.mark.parametrize("radius", ec.RADII)
def test_radii_reach_one_two_three_blocks_and_the_whole_grid(radius):
    p, kw = ec.cloud(f"radii-{radius}")
    assert len(p) == 600 and kw["particle_extent"] == 0.9 * radius
    _, cls = ec.particle_indices(p, kw)
    assert (np.bincount(cls, minlength=3) > 100).all()
    blocks, whole = [], True
    for a in range(3):
        n, g = kw["size"][a], np.arange(kw["size"][a] + 1)
        lo, hi = np.maximum(g - radius, 0), np.minimum(g + radius, n)
        blocks.append(int((((hi - 1) >> 3) - (lo >> 3) + 1).max()))
        whole = whole and bool(((lo == 0) & (hi == n)).all())
    assert tuple(blocks) == {1: (2, 2, 2), 2: (2, 2, 2), 5: (3, 2, 2), 9: (3, 2, 2), 20: (3, 2, 2), 64: (3, 2, 2)}[radius]
    assert whole == (radius >= 20)


@pytest.mark.parametrize("radius", ec.GAP_RADII)
@pytest.mark.parametrize("variant", list(ec.GAP_BLOCKS))
def test_block_gaps_points_see_the_flagged_block_last_or_in_the_middle(radius, variant):
    """Counts, per kind, the grid points that have a particle in their neighbourhood (value other than 1) and find the one flagged
    block only as the LAST block along one axis (the lowest along the other two), or only in the MIDDLE."""
    cid = f"block_gaps-{radius}-{variant}"
    p, kw = ec.cloud(cid)
    block = ec.GAP_BLOCKS[variant]
    t, cls = ec.particle_indices(p, kw)
    assert len(p) == 40 and (cls == ec.KEPT).all() and ((t.astype(int) >> 3) == np.array(block)).all()
    kinds = ec.block_kinds(kw, block)
    touched = oracle("cloud", cid)[0].ravel() != 1.0
    assert not touched[(kinds == "-").any(axis=1)].any() and touched.sum() > 500
    count = lambda *k: int((touched & (kinds == np.array(k)).all(axis=1)).sum())  # noqa: E731
    last = [count("H", "L", "L"), count("L", "H", "L"), count("L", "L", "H")]
    middle = [count("M", "L", "L"), count("L", "M", "L"), count("L", "L", "M")]
    if variant == "corner":  # the control: block 0 is the lowest block of every neighbourhood that reaches it
        assert last == middle == [0, 0, 0] and count("L", "L", "L") == touched.sum()
    else:
        assert min(last) > 0
        # radius 3 looks at 6 cells per axis, two blocks at the most; radius 9 at 18 cells, three or four
        assert min(middle) > 0 if radius == 9 else max(middle) == 0
    print(cid, "touched", int(touched.sum()), "last x/y/z", last, "middle x/y/z", middle)


def test_heavy_cells_counts():
    p, kw = ec.cloud("heavy_cells")
    cells = np.bincount(ec.kept_cells(p, kw), minlength=12 ** 3)
    want = np.zeros(12 ** 3, dtype=np.int64)
    for (x, y, z), n in ec.HEAVY.values():
        want[x + 12 * (y + 12 * z)] = n
    assert np.array_equal(cells, want) and len(p) == 3258
    u, inv, n = np.unique(p, axis=0, return_inverse=True, return_counts=True)
    assert (n == 2).sum() == 32 and (n <= 2).all()  # 64 particles coincident in pairs
    twice = np.nonzero(n[inv.ravel()] == 2)[0]
    assert (ec.kept_cells(p, kw)[twice] == 5 + 12 * (5 + 12 * 5)).all()
    assert np.array_equal(p * 2.0 ** 16, np.round(p * 2.0 ** 16))
    heavy = np.nonzero(ec.kept_cells(p, kw) == 5 + 12 * (5 + 12 * 5))[0]
    assert (np.diff(heavy) > 1).sum() > 200  # shuffled: the cell's particles are interleaved with the others'


@pytest.mark.parametrize("ncell", list(ec.SCAN_COUNTS))
def test_scan_edges_cloud_counts(ncell):
    p, kw = ec.cloud(f"scan_edges-{ncell}")
    nx, ny, nz = kw["size"]
    assert nx * ny * nz == ncell
    c = np.arange(ncell)
    inner = (c % nx > 0) & ((c // nx) % ny > 0) & (c // (nx * ny) > 0)
    want = np.where(inner, c % 3, 0)
    if min(kw["size"]) >= 2:
        want[-1] = max(want[-1], 1)
        assert want[-1] > 0 and inner.sum() > 0
    else:
        assert ncell in (257, 2047, 2049) and not inner.any()  # no factorisation with every extent >= 2: nothing is kept
    assert np.array_equal(np.bincount(ec.kept_cells(p, kw), minlength=ncell), want) and len(p) == want.sum()


def test_wide_sheet_counts():
    p, kw = ec.cloud("wide_sheet")
    nx, ny, nz = kw["size"]
    assert nx * ny * nz == 2101250 and -(-nx * ny * nz // ec.SCAN_BLOCK) == 1027 and len(p) == 200000
    cells = ec.kept_cells(p, kw)
    assert len(cells) == len(p) and (cells >= nx * ny).all()  # all kept, all in layer iz = 1
    beyond = int((cells >= ec.PER2).sum())
    occ = ec.cell_cases(oracle("cloud", "wide_sheet")[0]).ravel()
    crossing = int(((occ[ec.PER2:] != 0) & (occ[ec.PER2:] != 255)).sum())
    print("wide_sheet: particles, cells with a sign change at cell index >= 2 097 152:", beyond, crossing)
    assert beyond > 0 and crossing > 0


@pytest.mark.parametrize("radius", ec.OFFGRID_RADII)
def test_offgrid_is_off_the_lattice_and_has_every_class(radius):
    p, kw = ec.cloud(f"offgrid-{radius}")
    assert len(p) == 900 and kw["cell_size"] == 0.7 and kw["cell_radius"] == radius
    assert not np.array_equal(p * 2.0 ** 20, np.round(p * 2.0 ** 20))
    assert (np.bincount(ec.particle_indices(p, kw)[1], minlength=3) > 100).all()


@pytest.mark.parametrize("cid", ec.CLOUD_IDS)
def test_dyadic_clouds_are_on_the_lattice(cid):
    p, kw = ec.cloud(cid)
    if cid.startswith("offgrid"):
        return
    assert kw["cell_size"] in (1.0, 0.5) and all(o * 4 == round(o * 4) for o in kw["grid_offset"])
    c = (p - np.asarray(kw["grid_offset"])) / kw["cell_size"]
    ok = np.isfinite(c) & (np.abs(c) < 2.0 ** 20)
    lattice = 2.0 ** 33 if cid == "kernel_edge" else 2.0 ** 20
    assert np.array_equal((c * lattice)[ok], np.round(c * lattice)[ok])
    assert np.array_equal((np.asarray(kw["grid_offset"]) + kw["cell_size"] * c)[ok], p[ok])


def test_extremes_counts():
    v, kw = ec.field("extremes")
    assert v.shape == (5, 6, 7) and set(map(repr, v.ravel())) == set(map(repr, ec.EXTREME_VALUES))
    v1, v2, _ = ec.vertex_edges(v)
    _, pos, idx = oracle("field", "extremes")
    assert len(v1) == len(pos)
    neg_zero = lambda a: (a == 0) & np.signbit(a)  # noqa: E731
    with np.errstate(all="ignore"):
        d = v1 - v2
        counts = dict(v2_plus_zero=int(((v2 == 0) & ~np.signbit(v2)).sum()), v1_plus_zero=int(((v1 == 0) & ~np.signbit(v1)).sum()),
                      minus_zero_corner=int((neg_zero(v1) | neg_zero(v2)).sum()),
                      overflow=int((np.isfinite(v1) & np.isfinite(v2) & np.isinf(d)).sum()),
                      infinite_corner=int((np.isinf(v1) | np.isinf(v2)).sum()), nan_corner=int((np.isnan(v1) | np.isnan(v2)).sum()),
                      denormal_pair=int(((np.abs(v1) == 4.9e-324) & (np.abs(v2) == 4.9e-324)).sum()))
        t = v1 / d
    print("extremes:", len(pos), "vertices,", counts, "NaN vertices", int(np.isnan(t).sum()))
    assert min(counts.values()) > 0
    # - 0.0 is outside (`f < 0` is false): an edge from - 0.0 to + 0.0 or to a positive value carries no vertex
    assert not (neg_zero(v1) & (v2 >= 0)).any() and not (neg_zero(v2) & (v1 >= 0)).any()
    # the NaN share, by the oracle alone: a comparison with equal_nan cannot pass on NaN alone
    assert np.isnan(pos).mean() < 0.25 and int(np.isfinite(pos).all(axis=1).sum()) >= 200
    assert int(np.isnan(pos).any(axis=1).sum()) == int(np.isnan(t).sum()) and len(idx) > 600


def test_near_ties_counts():
    v, kw = ec.field("near_ties")
    v1, v2, _ = ec.grid_edges(v)[0]  # the designed pairs lie along x
    assert ((v1 < 0) != (v2 < 0)).all() and len(ec.vertex_edges(v)[0]) == 3 * 6 * 6 * 5 == len(oracle("field", "near_ties")[1])
    ratio = np.abs(v1) / np.abs(v2)
    for want in (2.0 ** -60, 2.0 ** 60, 2.0 ** -1000, 2.0 ** 1000, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52):
        assert (ratio == want).sum() >= 8, want
    assert (ratio == 1.0 / (1.0 + 2.0 ** -52)).sum() >= 8 and (ratio == 1.0).sum() == 0
    assert (np.sign(v1) == -1).sum() > 40 and (np.sign(v1) == 1).sum() > 40  # either sign leads


@pytest.mark.parametrize("ncell", list(ec.SCAN_COUNTS))
def test_scan_edges_field_counts(ncell, indices_per_case):
    v, kw = ec.field(f"scan_edges-{ncell}")
    nx, ny, nz = kw["size"]
    assert nx * ny * nz == ncell and v.shape == (nz + 1, ny + 1, nx + 1)
    _, _, own = ec.vertex_edges(v)
    per_cell = np.bincount(own, minlength=ncell)
    assert len(per_cell) == ncell and per_cell[-1] >= 3  # the last cell creates its edges 5, 6 and 10 (and more on a low face)
    for b in range(0, ncell, 256):
        assert per_cell[b:b + 256].any()
    _, pos, idx = oracle("field", f"scan_edges-{ncell}")
    assert per_cell.sum() == len(pos) and indices_per_case[ec.cell_cases(v).ravel()].sum() == len(idx)
    assert indices_per_case[ec.cell_cases(v).ravel()[-1]] > 0


def test_wide_sheet_field_counts(indices_per_case):
    v, kw = ec.field("wide_sheet_field")
    nx, ny, nz = kw["size"]
    assert nx * ny * nz == 2100225 >= ec.PER2 and -(-nx * ny * nz // ec.SCAN_BLOCK) == 1026
    occ = ec.cell_cases(v).ravel()
    surface = ((occ != 0) & (occ != 255)).mean()
    assert 1 / 14 < surface < 1 / 10
    _, _, own = ec.vertex_edges(v)
    _, pos, idx = oracle("field", "wide_sheet_field")
    ni = indices_per_case[occ]
    assert len(own) == len(pos) and ni.sum() == len(idx)
    beyond_v, beyond_i = int((own >= ec.PER2).sum()), int(ni[ec.PER2:].sum())
    print(f"wide_sheet_field: surface cells 1 in {1 / surface:.1f}; owned by cells >= 2 097 152: {beyond_v} vertices, {beyond_i} indices")
    assert beyond_v > 0 and beyond_i > 0


# ------------------------------------------------------------------------------------------- no designed particle is idle
def _values_without(p, kw, drop):
    return orc.mesher_surface(np.delete(p, drop, axis=0), kind="oracle", **kw)


@pytest.mark.parametrize("cid", ["cell_faces", "cell_faces_h05", "kernel_edge"] +
                         [f"block_gaps-3-{v}" for v in ec.GAP_BLOCKS] + ["block_gaps-9-middle"])
def test_deleting_a_designed_particle_changes_a_sampled_value(cid):
    """Every KEPT particle: the sampled values without it differ somewhere. Every dropped one (cell_faces holds 24): nothing
    changes. The two coincident particles of kernel_edge are one designed item: a lone pair at one position gives, bit for bit,
    what one of them gives (2 w q / 2 w), so they are deleted together. block_gaps at radius 9 (the particles of radius 3, 0.1 s
    per sampling) is checked for the middle block and every fourth particle."""
    p, kw = ec.cloud(cid)
    full = oracle("cloud", cid)[0]
    _, cls = ec.particle_indices(p, kw)
    items = [[i] for i in range(len(p))]
    if cid == "kernel_edge":
        k = ec.KERNEL_EDGE_SITES.index("coincident")
        items = [it for it in items if it[0] not in (k, k + 1)] + [[k, k + 1]]
        assert same(_values_without(p, kw, [k]), full)
    if cid == "block_gaps-9-middle":
        items = items[::4]
    for it in items:
        assert same(_values_without(p, kw, it), full) == (cls[it[0]] != ec.KEPT), (cid, it)
