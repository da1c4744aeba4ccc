"""Vertex normals of the device mesher (lfa_mesher_normals): mesh::generate_normals() of the reference, bit for bit.

CPU (`-m "not gpu"`): the fixture tests/golden/mesher_normals.npz (the real reference's normals,
tests/golden/make_golden_normals.py) equals a plain in-order fp64 restatement of the loop and, where oracle/_ref exists, the
live reference; the branch counts the inputs must keep exercising; the boundary (header, exports, binding).
GPU (`-m gpu`): libfluid_amd/csrc/mesher.hip through the C ABI against the fixture at tolerance 0. The bar is derived, not
measured: same operands, same order of additions, correctly rounded fp64 + - * / sqrt on both sides.

A finding about the inputs: in the `nan` field no vertex takes the (1, 0, 0) fallback (no sum is shorter than 1e-6); the 7
vertices whose normal is exactly (1, 0, 0) there have sums (a, 0, 0) with a > 0.02 and get it from the division. Both facts
are asserted below; the fallback branch is covered by `zeros15` (6 vertices) and `zeros30` (14)."""
import os
import re

import numpy as np
import pytest

import libfluid_amd as lfa
from libfluid_amd import scenes
from oracle import loader as orc
from tests import mesher_cases as mc
from tests import mesher_normals_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesher.npz")
GOLDEN_NORMALS = os.path.join(ROOT, "tests", "golden", "mesher_normals.npz")
E_INVALID, E_UNSUPPORTED = -1, -6


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def golden():
    g = load(GOLDEN)
    g.update(load(GOLDEN_NORMALS))
    return g


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def all_cases(g):
    """Yields (values[2,2,2], positions, indices, normals) for the 512 single-cell fixtures."""
    vo = io = k = 0
    for variant in (None, g["cases_mags"]):
        for case in range(256):
            nv, ni = g["cases_counts"][k]
            yield (mc.single_cell_values(case, None if variant is None else variant[case]),
                   g["cases_pos"][vo:vo + nv], g["cases_idx"][io:io + ni], g["cases_normals"][vo:vo + nv])
            vo, io, k = vo + nv, io + ni, k + 1


def field_mesher(name):
    """(Mesher arguments, values) of a fixture that is defined by grid-point values."""
    if name in nc.EXTRA_FIELDS:
        v, size = nc.extra_field(name)
    else:
        size = nc.FIELD_SIZES[name]
        v = mc.random_field(int(name[-1]), size)
    return dict(size=size, **nc.FIELD_GRID), v


def want_normals(pos, idx):
    """The live reference where it is built, else the in-order restatement (equal bit for bit: the CPU tests)."""
    return orc.ref_mesh_obj(pos, idx, normals=True)[1] if orc.have_ref() and len(pos) else nc.in_order_normals(pos, idx)


# ---------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", nc.GOLDEN_MESHES + list(nc.EXTRA_FIELDS))
def test_fixture_is_the_in_order_loop(golden, name):
    pos, idx, nrm = golden[f"{name}_pos"], golden[f"{name}_idx"], golden[f"{name}_normals"]
    assert len(pos) > 0 and nrm.dtype == np.float64
    assert same(nrm, nc.in_order_normals(pos, idx))
    if orc.have_ref():
        assert same(nrm, orc.ref_mesh_obj(pos, idx, normals=True)[1])


def test_fixture_of_the_single_cell_cases_is_the_in_order_loop(golden):
    assert len(golden["cases_normals"]) == len(golden["cases_pos"])
    n = 0
    for _, pos, idx, nrm in all_cases(golden):
        assert same(nrm, nc.in_order_normals(pos, idx))
        n += 1
    assert n == 512


@pytest.mark.parametrize("name", list(nc.EXTRA_FIELDS))
def test_extra_fields_exercise_the_branches(golden, name):
    """The inputs are pinned (values, and the reference's mesh of them), and so are the branches they are there for."""
    v, size = nc.extra_field(name)
    assert same(v, golden[f"{name}_values"])
    pos, idx, nrm = golden[f"{name}_pos"], golden[f"{name}_idx"], golden[f"{name}_normals"]
    p, i = orc.mesher_mesh(None, size, values=v, kind="oracle", **nc.FIELD_GRID)
    assert same(p, pos) and same(i, idx)
    nv, nt, fallbacks, nans, exact_x = nc.EXTRA_FIELDS[name]
    assert (len(pos), len(idx) // 3) == (nv, nt)
    assert nc.fallbacks_and_nans(pos, idx) == (fallbacks, nans)
    assert int(np.isnan(nrm).any(axis=1).sum()) == nans
    assert int((nrm == (1.0, 0.0, 0.0)).all(axis=1).sum()) == exact_x
    if name == "nan":
        assert int(np.isnan(pos).any(axis=1).sum()) == 41
    else:  # valence: the longest ordered sums
        assert np.bincount(idx.astype(np.int64)).max() == {"zeros15": 18, "zeros30": 15}[name]


def test_golden_mesh_sizes(golden):
    sizes = {n: (len(golden[f"{n}_pos"]), len(golden[f"{n}_idx"]) // 3) for n in nc.GOLDEN_MESHES}
    assert sizes == {"block": (390, 776), "edges": (440, 852), "fine": (744, 1484), "field1": (466, 697), "field2": (40, 30),
                     "field3": (115, 119)}
    assert len(golden["sparse_idx"]) == 0


def test_normals_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libfluid_amd.h")).read(), flags=re.S)
    lib = lfa.load_library()
    for name in ("lfa_mesher_normals", "lfa_mesher_download_normals"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/libfluid_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in lfa.SIGNATURES
    assert "mesh.h:38-53" in open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["field1", "field2", "field3"] + list(nc.EXTRA_FIELDS))
def test_normals_of_value_fields(golden, name):
    kw, v = field_mesher(name)
    m = lfa.Mesher(**kw)
    m.set_values(v)
    pos, idx = m.marching_cubes()
    assert same(pos, golden[f"{name}_pos"]) and same(idx, golden[f"{name}_idx"])
    got = m.normals()
    assert got.dtype == np.float64 and same(got, golden[f"{name}_normals"])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["block", "edges", "fine"])
def test_normals_of_uploaded_values_of_particle_cases(golden, name):
    _, kw = mc.particle_case(name)
    kw.pop("r")
    m = lfa.Mesher(**kw)
    m.set_values(golden[f"{name}_values"])
    m.marching_cubes()
    assert same(m.normals(), golden[f"{name}_normals"])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["block", "edges", "fine"])
def test_normals_from_sampled_particles(golden, name):
    p, kw = mc.particle_case(name)
    r = kw.pop("r")
    m = lfa.Mesher(**kw)
    m.sample(p, r)
    pos, idx = m.marching_cubes()
    assert same(pos, golden[f"{name}_pos"]) and same(idx, golden[f"{name}_idx"])
    assert same(m.normals(), golden[f"{name}_normals"])
    m.close()


@pytest.mark.gpu
def test_normals_of_all_256_cases(golden):
    m = lfa.Mesher((1, 1, 1))
    for v, pos, idx, nrm in all_cases(golden):
        m.set_values(v)
        p, i = m.marching_cubes()
        assert same(p, pos) and same(i, idx)
        got = m.normals()
        assert same(got, nrm), (v, got, nrm)
    m.close()


@pytest.mark.gpu
def test_empty_mesh(golden):
    p, kw = mc.particle_case("sparse")
    r = kw.pop("r")
    m = lfa.Mesher(**kw)
    pos, idx, nrm = m.generate_mesh(p, r, normals=True)
    assert len(pos) == 0 and len(idx) == 0 and nrm.shape == (0, 3)
    guard = np.full(6, 7.0)
    m._chk(m.lib.lfa_mesher_download_normals(m.h, guard.ctypes.data_as(lfa.C.c_void_p)))  # LFA_OK, nothing written
    assert (guard == 7.0).all()
    m.close()


@pytest.mark.gpu
def test_dam_break_surface_at_scale():
    """The 100^3 surface of tests/test_mesher.py::test_dam_break_surface_at_scale (same seed and settings)."""
    p = scenes.seed_block((1, 1, 1), (49, 49, 49))["pos"]
    p = p[np.random.default_rng(9).permutation(len(p))]
    kw = dict(size=(100, 100, 100), grid_offset=(0.0, 0.0, 0.0), cell_size=0.5, particle_extent=1.0, cell_radius=3)
    m = lfa.Mesher(**kw)
    pos, idx, nrm = m.generate_mesh(p, 0.5, normals=True)
    assert len(idx) > 100000 and nrm.shape == pos.shape
    want, fell_back = nc.in_order_normals(pos, idx, with_fallback_mask=True)
    if orc.have_ref():
        want = orc.ref_mesh_obj(pos, idx, normals=True)[1]
    assert same(nrm, want)
    regular = ~fell_back & ~np.isnan(nrm).any(axis=1)  # by-product, not the bar
    assert regular.sum() > 0.9 * len(nrm) and np.abs(np.linalg.norm(nrm[regular], axis=1) - 1.0).max() < 1e-15 * 4
    m.close()


@pytest.mark.gpu
def test_normals_from_a_simulation():
    sim = lfa.Sim((24, 24, 24), method=lfa.APIC)
    parts = scenes.seed_block((2, 1, 3), (12, 10, 11))
    parts = parts[np.random.default_rng(4).permutation(len(parts))]
    sim.upload_particles(parts)
    for _ in range(2):
        sim.time_step(0.01)
    m = lfa.Mesher(size=(48, 48, 48), grid_offset=(0.0, 0.0, 0.0), cell_size=0.5, particle_extent=1.0, cell_radius=3)
    m.sample_sim(sim, 0.5)
    pos, idx = m.marching_cubes()
    assert len(idx) > 1000
    assert same(m.normals(), want_normals(pos, idx))
    m.close()
    sim.close()


@pytest.mark.gpu
def test_state_rules(golden):
    kw, v = field_mesher("field1")
    m = lfa.Mesher(**kw)

    def refused(call):
        with pytest.raises(lfa.LibfluidError) as e:
            call()
        assert e.value.code == E_INVALID and "lfa_mesher_" in str(e.value)

    refused(m.compute_normals)   # before any extraction
    refused(m.download_normals)
    m.set_values(v)
    refused(m.compute_normals)   # values, but no mesh
    m.marching_cubes()
    refused(m.download_normals)  # a mesh, but no normals of it
    a = m.normals()
    assert same(a, golden["field1_normals"]) and same(m.normals(), a) and same(m.download_normals(), a)
    m.set_values(v)              # re-uploaded: the mesh is gone, and so are its normals
    refused(m.compute_normals)
    refused(m.download_normals)
    m.marching_cubes()
    refused(m.download_normals)  # a new extraction: the old normals are not handed out for it
    assert same(m.normals(), a)
    m.close()
    p, pkw = mc.particle_case("edges")
    r = pkw.pop("r")
    m = lfa.Mesher(**pkw)
    m.sample(p, r)
    m.marching_cubes()
    assert same(m.normals(), golden["edges_normals"])
    m.sample(p, r)               # re-sampled without a new extraction
    refused(m.compute_normals)
    refused(m.download_normals)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", [("zeros30", "zeros15"), ("zeros15", "zeros30")])
def test_a_second_field_on_the_same_handle(golden, order):
    """zeros15 has more vertices and triangles than zeros30: a larger mesh after a smaller one and the other way round."""
    assert len(golden["zeros15_pos"]) > len(golden["zeros30_pos"]) and len(golden["zeros15_idx"]) > len(golden["zeros30_idx"])
    kw, _ = field_mesher(order[0])
    m = lfa.Mesher(**kw)
    for name in order + order[:1]:
        m.set_values(golden[f"{name}_values"])
        m.marching_cubes()
        assert same(m.normals(), golden[f"{name}_normals"])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["block", "fine"])
def test_windows(golden, name):
    p, kw = mc.particle_case(name)
    r = kw.pop("r")
    nz = kw["size"][2]
    m = lfa.Mesher(window=(0, nz), **kw)  # the whole grid, spelled as a window
    m.sample(p, r)
    m.marching_cubes()
    assert same(m.normals(), golden[f"{name}_normals"])
    m.close()
    for lo, hi in ((0, nz // 2), (nz // 2, nz)):
        m = lfa.Mesher(window=(lo, hi), **kw)
        m.sample(p, r, ids=np.arange(len(p), dtype=np.uint32))
        before = m.marching_cubes()
        for call in (m.compute_normals, m.normals):
            with pytest.raises(lfa.LibfluidError) as e:
                call()
            assert e.value.code == E_UNSUPPORTED and "window" in str(e.value)
        after = m.download_mesh()
        assert same(before[0], after[0]) and same(before[1], after[1]) and len(before[1]) > 0
        again = m.marching_cubes()
        assert same(before[0], again[0]) and same(before[1], again[1])
        m.close()


@pytest.mark.gpu
def test_generate_mesh_returns_a_pair_unless_asked(golden):
    p, kw = mc.particle_case("fine")
    r = kw.pop("r")
    m = lfa.Mesher(**kw)
    out = m.generate_mesh(p, r)
    assert isinstance(out, tuple) and len(out) == 2
    out = m.generate_mesh(p, r, normals=True)
    assert len(out) == 3 and same(out[0], golden["fine_pos"]) and same(out[1], golden["fine_idx"]) and same(out[2], golden["fine_normals"])
    m.close()


@pytest.mark.gpu
def test_a_handle_that_never_asks_allocates_nothing_more(golden):
    """lfa_pool_stats: the normals' buffers (24 B per vertex and per triangle) are requested by the first lfa_mesher_normals and
    reused afterwards; sampling, extraction and download request nothing for them."""
    p, kw = mc.particle_case("block")
    r = kw.pop("r")

    def requests():
        s = lfa.pool_stats()
        return s["hits"] + s["misses"]

    def mesh_only(m):
        m.sample(p, r)
        return m.marching_cubes()

    lfa.Mesher(**kw).close()  # (first use of the device, one-time set-up)
    n0 = requests()
    m = lfa.Mesher(**kw)
    mesh_only(m)
    plain = requests() - n0
    m.close()
    n0 = requests()
    m = lfa.Mesher(**kw)
    pos, idx = mesh_only(m)
    assert requests() - n0 == plain  # the same requests as a handle of the same history: the feature costs nothing unasked
    n1 = requests()
    assert same(m.normals(), golden["block_normals"])
    assert requests() - n1 == 2      # normals + face vectors
    n2 = requests()
    m.normals()
    again = mesh_only(m)
    m.normals()
    assert requests() == n2          # reused
    assert same(again[0], pos) and same(again[1], idx)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("below", [1, 390, 12345678901])
def test_normals_of_a_rebased_mesh(golden, below):
    """lfa_mesher_rebase shifts the index list in place (a caller that concatenates the meshes of several meshers); the normals
    are those of the unshifted mesh, whenever they are asked for: the shift is remembered, never applied to the positions."""
    p, kw = mc.particle_case("block")
    r = kw.pop("r")
    m = lfa.Mesher(**kw)
    m.sample(p, r)
    m.marching_cubes()
    m.rebase(below)
    pos, idx = m.download_mesh()
    assert same(pos, golden["block_pos"]) and np.array_equal(idx, golden["block_idx"] + np.uint64(below))
    assert same(m.normals(), golden["block_normals"])
    m.rebase(7)  # a second shift adds up
    assert np.array_equal(m.download_mesh()[1], golden["block_idx"] + np.uint64(below + 7))
    assert same(m.normals(), golden["block_normals"])
    m.marching_cubes()  # a new extraction starts from unshifted indices again
    assert np.array_equal(m.download_mesh()[1], golden["block_idx"]) and same(m.normals(), golden["block_normals"])
    m.close()


@pytest.mark.gpu
def test_normals_time_follows_the_state_rules(golden):
    kw, v = field_mesher("field1")
    m = lfa.Mesher(**kw)
    m.set_values(v)
    m.marching_cubes()
    with pytest.raises(lfa.LibfluidError) as e:
        m.normals_ms()
    assert e.value.code == E_INVALID and "lfa_mesher_normals_time" in str(e.value)
    m.normals()
    assert m.normals_ms() > 0.0
    m.close()
