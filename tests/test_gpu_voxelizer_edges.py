"""libfluid_amd/csrc/voxelizer.hip on the adversarial inputs of tests/voxel_edge_cases.py, bit-exact against what the real
reference computed on them (tests/golden/voxelizer_edges.npz; tests/test_voxel_edge_cases.py holds the oracle to the same
vectors). What each case is aimed at is said in voxel_edge_cases.py.

The `stale_*` grids hold EXTERIOR cells on entry to mark_exterior. Before the fix that came with this file (k_flood_pass let
any EXTERIOR cell start a front, and the passes ran with a SURFACE corner too) the device left, of these grids' cells,
6 / 104 / 6 242 / 1 126 exterior where the reference leaves 2 / 1 / 5 509 / 1 027 (stale_line, stale_corner_surface,
stale_reopened, stale_cavity)."""
import os

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import voxel_edge_cases as vec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxelizer_edges.npz")
I, E, S = lfa.VOX_INTERIOR, lfa.VOX_EXTERIOR, lfa.VOX_SURFACE


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def inputs(g, name):
    return g[f"{name}_pos"], g[f"{name}_idx"], float(g[f"{name}_cs"]), g[f"{name}_off"], g[f"{name}_ref_size"]


def cells_from_types(types, kinds, grid_min=None, ref_size=None):
    """grid3::for_each order (z slowest, x fastest) list of the cells whose type is in `kinds`."""
    z, y, x = np.nonzero(np.isin(types, kinds))
    c = np.stack([x, y, z], axis=1).astype(np.int64)
    if ref_size is not None:
        c = c + np.asarray(grid_min, dtype=np.int64)[None, :]
        c = c[np.all((c >= 0) & (c < np.asarray(ref_size)[None, :]), axis=1)]
    return c.astype(np.int32)


def same_cells(got, want):
    """An empty selection comes back as an empty int32[0, 3] (lfa_voxels_cells writes nothing then)."""
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    return np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ mesh cases
@pytest.mark.parametrize("index_type", [np.uint64, np.uint32])
@pytest.mark.parametrize("name", vec.MESH_NAMES)
def test_device_voxelizer_is_bit_exact_on_the_edge_meshes(golden, name, index_type):
    pos, idx, cs, off, rs = inputs(golden, name)
    want = golden[f"{name}_types"]
    v = lfa.Voxels.from_mesh(pos, idx.astype(index_type), cs, off)
    assert np.array_equal(v.grid_min, golden[f"{name}_grid_min"])
    assert np.array_equal(v.grid_offset, golden[f"{name}_grid_off"])
    got = v.types()
    assert got.shape == want.shape
    assert np.array_equal(got == S, want == S), ("surface", int((got == S).sum()), int((want == S).sum()))
    assert np.array_equal(got, want), {k: (int((got == k).sum()), int((want == k).sum())) for k in (I, E, S)}
    assert same_cells(v.cells(True, False, rs), golden[f"{name}_cells_ref_interior"])
    assert same_cells(v.cells(True, True), golden[f"{name}_cells_all"])
    assert same_cells(v.cells(False, True), cells_from_types(want, [S]))
    v.close()


def test_seven_and_lattice_01_keep_selected_cells(golden):
    assert len(golden["seven_cells_ref_interior"]) > 0 and len(golden["lattice_01_cells_ref_interior"]) > 0


@pytest.mark.parametrize("name", ["tower", "degenerate_037"])
def test_staged_calls_on_the_edge_meshes(golden, name):
    pos, idx, cs, off, rs = inputs(golden, name)
    want = golden[f"{name}_types"]
    v = lfa.Voxels.create(want.shape[::-1], golden[f"{name}_grid_off"], cs)
    v.voxelize_triangles(pos, idx)
    surf = v.types()
    assert np.array_equal(surf == S, want == S) and not (surf == E).any()
    v.mark_exterior()
    assert np.array_equal(v.types(), want)
    v.close()


def test_an_empty_selection_is_an_empty_array(golden):
    """lfa_voxels_cells writes nothing for an empty selection; the wrapper hands it a zero-length buffer and returns it."""
    want = golden["lattice_01_types"]
    v = lfa.Voxels.create(want.shape[::-1], golden["lattice_01_grid_off"], 0.1)
    v.upload(np.full(want.shape, E, dtype=np.uint8))                    # nothing to select at all
    for args in ((True, True), (True, False), (False, True), (True, True, (35, 30, 50))):
        c = v.cells(*args)
        assert c.dtype == np.int32 and c.shape == (0, 3)
    v.upload(want)                                                      # a full list, then an empty one from the same handle
    assert len(v.cells(True, True)) == 26048
    v.upload(np.full(want.shape, E, dtype=np.uint8))
    assert v.cells(True, True).shape == (0, 3)
    v.close()


# ------------------------------------------------------------------------------------------------------------ grid cases
@pytest.mark.parametrize("name", vec.GRID_NAMES)
def test_mark_exterior_on_uploaded_grids_is_the_reference_s(golden, name):
    t, want = golden[f"{name}_in"], golden[f"{name}_out"]
    v = lfa.Voxels.create(t.shape[::-1], (0.0, 0.0, 0.0), 1.0)
    v.upload(t)
    v.mark_exterior()
    got = v.types()
    print(name, "exterior cells: input", int((t == E).sum()), "device", int((got == E).sum()), "reference", int((want == E).sum()))
    assert np.isin(got, (I, E, S)).all()
    assert np.array_equal(got, want), {k: (int((got == k).sum()), int((want == k).sum())) for k in (I, E, S)}
    v.mark_exterior()                                                   # a second call changes nothing
    assert np.array_equal(v.types(), want)
    v.close()


def test_reopening_a_voxelized_box_leaves_its_cavity_interior(golden):
    """The realistic form of stale_reopened: from_mesh, the host removes part of a wall, mark_exterior again."""
    pos, idx, cs, off, rs = inputs(golden, "lattice_05")
    v = lfa.Voxels.from_mesh(pos, idx, cs, off)
    t = v.types()
    assert np.array_equal(t, golden["lattice_05_types"])
    z, y, x = np.argwhere(t == I)[0]
    edited = t.copy()
    edited[z, y, :x] = np.where(edited[z, y, :x] == S, I, edited[z, y, :x])   # a tunnel from the first interior cell to x = 0
    assert (edited != t).sum() >= 1
    v.upload(edited)
    v.mark_exterior()
    got = v.types()
    assert np.array_equal(got, orc.voxel_mark_exterior(edited, kind="oracle"))
    assert np.array_equal(got, edited)                                  # the exterior of the first call walls the tunnel in
    assert same_cells(v.cells(True, False), cells_from_types(edited, [I]))
    v.close()


# --------------------------------------------------------------------------------------------- compaction against numpy
@pytest.mark.parametrize("size", [(128, 128, 128), (129, 128, 128), (131, 127, 127), (3, 2, 1)])
def test_cell_lists_are_numpy_s_on_random_grids(size):
    """1024 blocks of 2048 cells (one entry per thread of k_scan_blocks), 1032 and 1032 (two), and a grid below one block."""
    nx, ny, nz = size
    t = np.random.default_rng(20240607).integers(0, 3, size=(nz, ny, nx), dtype=np.uint8)
    v = lfa.Voxels.create(size, (0.0, 0.0, 0.0), 1.0)
    v.upload(t)
    assert same_cells(v.cells(True, False), cells_from_types(t, [I]))
    assert same_cells(v.cells(False, True), cells_from_types(t, [S]))
    v.close()


def test_clipped_cell_list_is_numpy_s_on_a_random_grid(golden):
    pos, idx, cs, off, rs = inputs(golden, "seven")
    v = lfa.Voxels.from_mesh(pos, idx, cs, off)
    gmin = v.grid_min.copy()
    assert (gmin != 0).all() and np.array_equal(gmin, golden["seven_grid_min"])
    nx, ny, nz = v.size
    t = np.random.default_rng(7).integers(0, 3, size=(nz, ny, nx), dtype=np.uint8)
    v.upload(t)
    want = cells_from_types(t, [I, S], gmin, rs)
    assert 0 < len(want) < (t != E).sum()                               # the clip cuts some cells and keeps some
    assert same_cells(v.cells(True, True, rs), want)
    v.close()


# ------------------------------------------------------------------------------------------------------------ clamping
def test_triangles_that_stick_out_are_clamped_to_the_grid():
    """The project's own behaviour (the reference requires the triangle inside the grid): the cells of the small grid get
    what an enclosing grid on the same lattice gets. Cell size 0.5 and offsets that are multiples of 0.5: the centre sums
    are exact, so the first cell of the clamped range starts the same sum the enclosing grid reaches there."""
    cs, pad = 0.5, 12
    small_n, small_off = (9, 7, 6), np.array([1.0, 0.5, -0.5])
    big_n, big_off = tuple(n + 2 * pad for n in small_n), small_off - pad * cs
    hi = small_off + np.array(small_n) * cs                                                # (5.5, 4.0, 2.5)
    pos = np.array([[-1.3, 1.1, 0.2], [7.9, 2.3, 1.1], [2.2, 3.1, -0.1],      # out on x low and x high
                    [2.1, -2.2, 0.3], [3.3, 6.6, 1.4], [4.4, 1.2, 2.1],       # out on y low and y high
                    [1.7, 1.3, -3.1], [4.6, 2.9, 5.2], [2.4, 3.6, 0.4],       # out on z low and z high
                    [-2.0, -1.5, -3.0], [8.0, 6.0, 5.0], [0.3, 5.5, -2.2],    # out on every side
                    [6.1, 4.6, 3.2], [7.3, 5.5, 4.1], [6.6, 6.2, 3.3],        # wholly beyond the high corner
                    [-1.2, -1.1, -2.9], [0.4, -0.3, -1.2], [-0.7, 0.2, -2.2],  # wholly below the low corner
                    [1.0, 0.5, -0.5], [5.5, 0.5, -0.5], [1.0, 4.0, 2.5]],     # on the grid's own corners: touches, fits
                   dtype=np.float64)
    idx = np.arange(len(pos), dtype=np.uint64)
    assert (pos.min(axis=0) < small_off).all() and (pos.max(axis=0) > hi).all()
    assert (pos.min(axis=0) > big_off + cs).all() and (pos.max(axis=0) < big_off + (np.array(big_n) - 1) * cs).all()
    want = orc.voxel_triangles(np.zeros(big_n[::-1], dtype=np.uint8), big_off, cs, pos, idx, kind="oracle")
    crop = want[pad:pad + small_n[2], pad:pad + small_n[1], pad:pad + small_n[0]]
    assert 0 < (crop == S).sum() < crop.size and (want == S).sum() > (crop == S).sum()
    for index_type in (np.uint64, np.uint32):
        v = lfa.Voxels.create(small_n, small_off, cs)
        v.voxelize_triangles(pos, idx.astype(index_type))
        got = v.types()
        assert np.array_equal(got, crop), (int((got == S).sum()), int((crop == S).sum()))
        v.close()
