"""Surface mesher on the adversarial clouds and fields of tests/mesher_edge_cases.py: libfluid_amd/csrc/mesher.hip through the C
ABI against the live oracle (which tests/test_mesher_edge_cases.py holds to the compiled reference on exactly these inputs).
Bit for bit, with `same()` of tests/test_mesher.py: sampled values (NaN where the reference has 0 / 0), vertex positions, vertex
order and index lists, every point and every vertex of every case. There is no tolerance in this file."""
import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import mesher_cases as mc
from tests import mesher_edge_cases as ec
from tests.test_mesher import same, stitched_z_windows

pytestmark = pytest.mark.gpu

_want = {}


def want(kind, cid):
    """(values, positions, indices) of the oracle, computed once per case and shared by the tests; never written to."""
    if (kind, cid) not in _want:
        _want[kind, cid] = ec.results(cid, "oracle", kind == "field")
        for a in _want[kind, cid]:
            a.flags.writeable = False
    return _want[kind, cid]


def device_cloud(cid):
    p, kw = ec.cloud(cid)
    r = kw.pop("r")
    m = lfa.Mesher(**kw)
    m.sample(p, r)
    values = m.values()
    pos, idx = m.marching_cubes()
    counts = m._counts
    m.close()
    return values, pos, idx, counts


def assert_same_result(got, wanted):
    for a, b in zip(got, wanted):
        assert same(a, b)


@pytest.mark.parametrize("cid", [c for c in ec.CLOUD_IDS if c != "wide_sheet"])
def test_sampling_and_mesh_on_adversarial_clouds(cid):
    assert_same_result(device_cloud(cid)[:3], want("cloud", cid))


@pytest.mark.parametrize("fid", [f for f in ec.FIELD_IDS if f != "wide_sheet_field"])
def test_marching_cubes_on_adversarial_fields(fid):
    v, kw = ec.field(fid)
    m = lfa.Mesher(**kw)
    m.set_values(v)
    pos, idx = m.marching_cubes()
    m.close()
    assert_same_result((pos, idx), want("field", fid)[1:])


def test_unrepresentable_coordinates_change_nothing_on_the_device():
    """The device's conversion saturates and turns NaN into 0 where x86 yields INT_MIN: both must drop the particle."""
    got, base = device_cloud("unrepresentable"), device_cloud("cell_faces")
    assert_same_result(got[:3], base[:3])
    assert_same_result(got[:3], want("cloud", "cell_faces"))


@pytest.mark.parametrize("partition", ["layers", "one_cut"])
@pytest.mark.parametrize("cid", [c for c in ec.CLOUD_IDS if c != "wide_sheet"])
def test_z_windows_on_adversarial_clouds(cid, partition):
    """One-layer windows throughout, and one interior cut; at radii 9 and beyond every window stores the whole grid."""
    p, kw = ec.cloud(cid)
    r = kw.pop("r")
    nz = kw["size"][2]
    bounds = list(range(nz + 1)) if partition == "layers" else sorted({0, max(1, nz // 2), nz})
    values, wpos, widx = want("cloud", cid)
    pos, idx = stitched_z_windows(p, kw, r, bounds, values, np.random.default_rng(7))
    assert same(pos, wpos) and same(idx, widx)


GRID26 = dict(size=(26, 26, 26), grid_offset=(0.0, 0.0, 0.0), cell_size=1.0, particle_extent=2.0, cell_radius=3)


def test_particle_arrays_grow_on_a_reused_handle():
    """9 particles, then 3 258 (the four particle arrays are released and requested again), none, then the 9 again."""
    small, big = ec.cloud("kernel_edge")[0], ec.cloud("heavy_cells")[0]
    m = lfa.Mesher(**GRID26)
    sizes = []
    for p in (small, big, np.zeros((0, 3)), small):
        m.sample(p, 0.5)
        v = orc.mesher_surface(p, kind="oracle", r=0.5, **GRID26)
        assert same(m.values(), v)
        wpos, widx = orc.mesher_mesh(None, GRID26["size"], values=v, kind="oracle")
        pos, idx = m.marching_cubes()
        assert same(pos, wpos) and same(idx, widx)
        sizes.append(len(pos))
    m.close()
    assert len(big) > 300 * len(small) and sizes[0] == sizes[3] > 0 and sizes[1] > 0 and sizes[2] == 0


def test_mesh_arrays_grow_on_a_reused_handle():
    """A field with under 100 vertices, a dense random one (vpos and vidx are released and requested again), the small one again."""
    small = np.ones((27, 27, 27))
    small[10:12, 10:12, 10:12] = -0.75
    dense = mc.random_field(11, GRID26["size"])
    m = lfa.Mesher(**GRID26)
    sizes = []
    for v in (small, dense, small):
        m.set_values(v)
        pos, idx = m.marching_cubes()
        wpos, widx = orc.mesher_mesh(None, GRID26["size"], values=v, kind="oracle")
        assert same(pos, wpos) and same(idx, widx)
        sizes.append(len(pos))
    m.close()
    assert sizes[0] == sizes[2] == 24 and sizes[1] > 20000


def test_wide_sheet():
    """2 101 250 cells: k_scan_block_sums holds two block sums per thread, in the cell starts and in both offset scans."""
    values, pos, idx, counts = device_cloud("wide_sheet")
    wv, wpos, widx = want("cloud", "wide_sheet")
    assert counts == (len(wpos), len(widx))
    assert same(values, wv) and same(pos, wpos) and same(idx, widx)


def test_wide_sheet_field():
    v, kw = ec.field("wide_sheet_field")
    m = lfa.Mesher(**kw)
    m.set_values(v)
    pos, idx = m.marching_cubes()
    counts = m._counts
    m.close()
    _, wpos, widx = want("field", "wide_sheet_field")
    assert counts == (len(wpos), len(widx))
    assert same(pos, wpos) and same(idx, widx)
