"""CPU tests of tests/voxel_edge_cases.py: the oracle is the reference on exactly these inputs (the golden vectors the real
reference produced, tests/golden/voxelizer_edges.npz, and a live oracle/_ref where it is present) - without that a
device-against-golden comparison on them proves nothing about the oracle the other tests use -, and every case holds what it
is there for, counted with numpy."""
import os

import numpy as np
import pytest

from oracle import loader as orc
from tests import voxel_edge_cases as vec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxelizer_edges.npz")
I, E, S = vec.INTERIOR, vec.EXTERIOR, vec.SURFACE
needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def cells_from_types(types, kinds, grid_min=None, ref_size=None):
    """grid3::for_each order (z slowest, x fastest) list of the cells whose type is in `kinds`."""
    z, y, x = np.nonzero(np.isin(types, kinds))
    c = np.stack([x, y, z], axis=1).astype(np.int64)
    if ref_size is not None:
        c = c + np.asarray(grid_min, dtype=np.int64)[None, :]
        c = c[np.all((c >= 0) & (c < np.asarray(ref_size)[None, :]), axis=1)]
    return c.astype(np.int32)


def counts(t):
    return tuple(int((t == k).sum()) for k in (I, E, S))


# ------------------------------------------------------------------------------------------- oracle == reference
@pytest.mark.parametrize("name", vec.MESH_NAMES)
def test_golden_inputs_are_the_generated_meshes(golden, name):
    pos, idx, cs, off, rs = vec.make(name)
    assert np.array_equal(pos, golden[f"{name}_pos"]) and np.array_equal(idx, golden[f"{name}_idx"])
    assert cs == float(golden[f"{name}_cs"]) and np.array_equal(np.asarray(off), golden[f"{name}_off"])
    assert np.array_equal(np.asarray(rs), golden[f"{name}_ref_size"])


@pytest.mark.parametrize("name", vec.GRID_NAMES)
def test_golden_inputs_are_the_generated_grids(golden, name):
    t = vec.grid(name)
    assert t.dtype == np.uint8 and np.array_equal(t, golden[f"{name}_in"]) and np.isin(t, (I, E, S)).all()


@pytest.mark.parametrize("name", vec.MESH_NAMES)
def test_oracle_matches_reference_golden_on_the_meshes(golden, name):
    pos, idx, cs, off, rs = vec.make(name)
    gmin, goff, types = orc.voxelize(pos, idx, cs, off, kind="oracle")
    assert np.array_equal(gmin, golden[f"{name}_grid_min"]) and np.array_equal(goff, golden[f"{name}_grid_off"])
    assert np.array_equal(types, golden[f"{name}_types"])
    assert np.array_equal(cells_from_types(types, [I], gmin, rs), golden[f"{name}_cells_ref_interior"])
    assert np.array_equal(cells_from_types(types, [I, S]), golden[f"{name}_cells_all"])
    # the staged entry points on the fitted grid are the fused call
    surf = orc.voxel_triangles(np.zeros_like(types), goff, cs, pos, idx, kind="oracle")
    assert np.array_equal(surf == S, types == S) and not (surf == E).any()
    assert np.array_equal(orc.voxel_mark_exterior(surf, kind="oracle"), types)


@pytest.mark.parametrize("name", vec.GRID_NAMES)
def test_oracle_matches_reference_golden_on_the_grids(golden, name):
    t = vec.grid(name)
    keep = t.copy()
    out = orc.voxel_mark_exterior(t, kind="oracle")
    assert np.array_equal(t, keep) and out is not t                     # a new array
    assert np.array_equal(out, golden[f"{name}_out"])
    assert np.array_equal(orc.voxel_mark_exterior(out, kind="oracle"), out)  # a second call changes nothing


@needs_ref
@pytest.mark.parametrize("name", vec.MESH_NAMES)
def test_oracle_matches_live_reference_on_the_meshes(golden, name):
    pos, idx, cs, off, rs = vec.make(name)
    for a, b in zip(orc.voxelize(pos, idx, cs, off, kind="oracle"), orc.voxelize(pos, idx, cs, off, kind="ref")):
        assert np.array_equal(a, b)
    goff, types = golden[f"{name}_grid_off"], golden[f"{name}_types"]
    surf = orc.voxel_triangles(np.zeros_like(types), goff, cs, pos, idx, kind="ref")
    assert np.array_equal(surf, orc.voxel_triangles(np.zeros_like(types), goff, cs, pos, idx, kind="oracle"))
    assert np.array_equal(orc.voxel_mark_exterior(surf, kind="ref"), types)


@needs_ref
@pytest.mark.parametrize("name", vec.GRID_NAMES)
def test_oracle_matches_live_reference_on_the_grids(golden, name):
    t = vec.grid(name)
    assert np.array_equal(orc.voxel_mark_exterior(t, kind="ref"), orc.voxel_mark_exterior(t, kind="oracle"))


@needs_ref
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_staged_oracle_matches_live_reference_on_random_edited_grids(seed):
    """Random grids of all three types (a host's edits), then triangles on top of them, then the flood."""
    rng = np.random.default_rng(seed)
    t = rng.choice(np.array([I, I, I, E, S], dtype=np.uint8), size=(9, 11, 13))
    pos = rng.uniform(0.5, 4.0, size=(12, 3))
    idx = rng.integers(0, 12, size=3 * 7).astype(np.uint64)
    off, cs = (-0.25, 0.1, 0.0), 0.5
    a, b = orc.voxel_triangles(t, off, cs, pos, idx, kind="oracle"), orc.voxel_triangles(t, off, cs, pos, idx, kind="ref")
    assert np.array_equal(a, b) and (a != t).any()
    assert np.array_equal(orc.voxel_mark_exterior(a, kind="oracle"), orc.voxel_mark_exterior(b, kind="ref"))


# ----------------------------------------------------------------------------------- what every case is there for
def test_tower_is_longer_than_a_chunk_on_every_axis_and_more_than_1024_blocks(golden):
    pos, idx, cs, off, rs = vec.make("tower")
    goff, types = golden["tower_grid_off"], golden["tower_types"]
    lo, hi = ((pos.min(axis=0) - goff) / cs).astype(np.int64), ((pos.max(axis=0) - goff) / cs).astype(np.int64)
    assert len(idx) == 3 and (hi - lo + 1 > 128).all(), hi - lo + 1
    assert types.shape == (134, 132, 132) and types.size == 2334816 > 1024 * 2048      # per = 2 in k_scan_blocks
    assert counts(types) == (0, 2317278, 17538)
    # surface cells in the second chunk of every axis, and in the second chunk of all three at once
    z, y, x = np.nonzero(types == S)
    for a, l in ((x, lo[0]), (y, lo[1]), (z, lo[2])):
        assert (a - l >= 128).any()
    assert cs * 3 != 0.3 and not float(cs).is_integer()                                   # 0.1: the sums round
    c, run = goff[2] + lo[2] * cs + 0.5 * cs, []
    for k in range(hi[2] - lo[2] + 1):
        run.append(c)
        c += cs
    exact = goff[2] + (lo[2] + np.arange(len(run))) * cs + 0.5 * cs
    assert (np.array(run)[128:] != exact[128:]).any()                                     # the carry is not recomputable


def test_lattice_faces_lie_on_cell_boundaries(golden):
    pos, idx, cs, off, rs = vec.make("lattice_05")
    q = (pos - golden["lattice_05_grid_off"]) / cs
    assert np.array_equal(q, np.rint(q)) and len(idx) == 36
    assert counts(golden["lattice_05_types"]) == (90, 152, 190)
    # a touching cell counts: cell `hi` of every axis lies outside the box and shares only the face with it, and is surface.
    # (On the low side the touching layer lo - 1 is not in the triangle's index range, src/voxelizer.cpp:64, and stays out.)
    t = golden["lattice_05_types"]
    z, y, x = np.nonzero(t == S)
    lo, hi = q.min(axis=0).astype(int), q.max(axis=0).astype(int)
    assert (x.min(), y.min(), z.min()) == tuple(lo) and (x.max(), y.max(), z.max()) == tuple(hi)
    assert (t[:, :, hi[0]] == S).sum() > 0 and (t[:, hi[1], :] == S).sum() > 0 and (t[hi[2], :, :] == S).sum() > 0


def test_lattice_01_has_a_surface_corner_and_no_exterior_cell(golden):
    t = golden["lattice_01_types"]
    assert t[0, 0, 0] == S and counts(t) == (21236, 0, 4812)
    assert len(golden["lattice_01_cells_ref_interior"]) > 0


def test_degenerate_holds_the_five_kinds(golden):
    pos, idx, cs, off, rs = vec.make("degenerate")
    tri = pos[idx.astype(np.int64).reshape(-1, 3)]
    assert len(tri) == 5 and len(tri) % 4 == 1
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert [a == 0.0 for a in area] == [True, True, False, True, True]
    i = idx.reshape(-1, 3)
    assert i[0, 0] == i[0, 1] == i[0, 2] and i[1, 0] != i[1, 1] and np.array_equal(tri[1, 0], tri[1, 1])
    assert len(set(i[3])) == 3 and len({tuple(p) for p in tri[3]}) == 3 and len(set(i[4])) == 2
    for name in ("degenerate", "degenerate_037"):
        t = golden[f"{name}_types"]
        # every degenerate triangle still marks the cells it passes through: the point's cell among them
        p, goff, c = pos[0], golden[f"{name}_grid_off"], float(golden[f"{name}_cs"])
        x, y, z = ((p - goff) / c).astype(int)
        assert t[z, y, x] == S and (t == I).sum() == 0
    assert float(golden["degenerate_037_cs"]) == 0.37 and np.array_equal(golden["degenerate_037_off"], (-0.4, 0.11, 0.2))


def test_seven_keeps_interior_cells_and_has_a_triangle_inside_one_cell(golden):
    pos, idx, cs, off, rs = vec.make("seven")
    tri = idx.astype(np.int64).reshape(-1, 3)
    assert len(tri) == 7 and len(tri) % 4 == 3 and np.array_equal(tri[5], tri[6])
    goff, t = golden["seven_grid_off"], golden["seven_types"]
    for k in (4, 5):
        c = ((pos[tri[k]] - goff) / cs).astype(int)
        assert (c == c[0]).all()                                                           # inside a single cell
    assert (t == I).sum() > 0 and len(golden["seven_cells_ref_interior"]) > 0
    # the small triangle inside the tetrahedron alone turns its cell from interior to surface
    x, y, z = ((pos[tri[4, 0]] - goff) / cs).astype(int)
    _, _, without = orc.voxelize(pos, np.delete(idx, [12, 13, 14]), cs, off, kind="oracle")
    assert t[z, y, x] == S and without[z, y, x] == I and (t != without).sum() == 1


def test_maze_is_one_long_corridor_and_its_pockets_stay_interior(golden):
    t, out = vec.grid("maze"), golden["maze_out"]
    assert t.shape == (5, 27, 41) and all(n % 8 for n in t.shape)
    pockets = np.zeros(t.shape, dtype=bool)
    for (x, y, z) in vec.MAZE_POCKETS:
        pockets[z, y, x] = True
    corridor = (t == I) & ~pockets
    assert corridor.sum() == 1679 and np.array_equal(out == E, corridor) and np.array_equal(out == I, pockets)
    # on a grid without exterior cells the spread rule is the reference's; its sweeps are the longest shortest path
    model, sweeps = vec.spread_rule(t)
    assert np.array_equal(model, out) and sweeps == 1678 >= 1500
    # how each pocket meets the corridor: not at all, across an edge only, across a corner only
    c = np.pad(corridor, 1)
    for (x, y, z), kind in vec.MAZE_POCKETS.items():
        near = {1: 0, 2: 0, 3: 0}
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dx or dy or dz) and c[z + 1 + dz, y + 1 + dy, x + 1 + dx]:
                        near[abs(dx) + abs(dy) + abs(dz)] += 1
        assert near[1] == 0, (x, y, z)
        if kind == "sealed":
            assert near[2] == 0 and near[3] == 0
        elif kind == "edge":
            assert near[2] > 0
        else:
            assert near[2] == 0 and near[3] > 0
    assert {"sealed", "edge", "corner"} == set(vec.MAZE_POCKETS.values())


@pytest.mark.parametrize("name", ["column_x", "column_y", "column_z", "sheet"])
def test_thin_grids_stop_at_their_wall(golden, name):
    t, out = vec.grid(name), golden[f"{name}_out"]
    assert sorted(t.shape)[0] == 1 and not (t == E).any()
    if name == "sheet":
        assert t.shape == (1, 17, 9) and counts(out) == (44, 100, 9)
        assert out[0, 11, 8] == E and out[0, 12, 7] == I and out[0, 12, 8] == S          # the diagonal neighbour stays interior
    else:
        assert sorted(t.shape) == [1, 1, 50] and counts(out) == (19, 30, 1)
        assert np.array_equal(out.reshape(-1), np.r_[np.full(30, E), S, np.full(19, I)].astype(np.uint8))


@pytest.mark.parametrize("name", vec.STALE_NAMES)
def test_stale_cases_tell_the_reference_s_rule_from_the_spread_rule(golden, name):
    t, out = golden[f"{name}_in"], golden[f"{name}_out"]
    assert (t == E).any()
    model, _ = vec.spread_rule(t)
    assert not np.array_equal(model, out), name
    print(name, "exterior cells: input", int((t == E).sum()), "reference", int((out == E).sum()), "spread rule", int((model == E).sum()))
    if name == "stale_line":
        assert out.reshape(-1).tolist() == [1, 1, 0, 0, 0, 0] and (model == E).all()
    if name == "stale_corner_surface":
        assert t[0, 0, 0] == S and np.array_equal(out, t) and (model == E).sum() == t.size - 1
    if name == "stale_reopened":
        assert t.shape == (18, 19, 20) and all(n > 16 for n in t.shape)                   # several 8^3 blocks
        closed = t.copy()
        closed[7:9, 9:11, 5] = S
        unflooded = np.where(closed == E, I, closed).astype(np.uint8)
        assert np.array_equal(orc.voxel_mark_exterior(unflooded), closed)                  # the input IS a flooded closed box
        assert (t != closed).sum() == 4 and np.array_equal(out, t)                         # patch and cavity stay interior
        assert (model == I).sum() == 0
    if name == "stale_cavity":
        assert (t == E).sum() == 1 and counts(out) == (99, 1027, 194) and (model == I).sum() == 0
        z, y, x = np.argwhere(t == E)[0]
        assert out[z, y, x] == E and (out[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] == E).sum() == 1
