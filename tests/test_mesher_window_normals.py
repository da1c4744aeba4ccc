"""Vertex normals on z-windows (lfa_mesher_window_normals, lfa_mesher_download_boundary): the windows of a slab run, stitched,
give mesh::generate_normals() of the single grid bit for bit.

CPU (`-m "not gpu"`): the boundary (header, exports, binding); the seams the GPU cases rely on are really in the fixtures.
GPU (`-m gpu`): libfluid_amd/csrc/mesher.hip through the C ABI against tests/golden/mesher_normals.npz (the real reference's
normals) at tolerance 0, NaNs equal. The bar is derived, not measured: a window adds the same face vectors (same operands: the
vertices of the plane below it are recomputed with the arithmetic that created them) in the same order (the triangles of the
layer above come last in a vertex's sum, in the order of the upper window's list), then the same dot, sqrt and division."""
import os
import re
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import mesher_cases as mc
from tests import mesher_normals_cases as nc
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6
CUTS = [(0.5,), (0.25, 0.6), (0.1, 0.2, 0.3, 0.7, 0.9)]
NEW_ENTRY_POINTS = ("lfa_mesher_boundary_size", "lfa_mesher_download_boundary", "lfa_mesher_window_normals",
                    "lfa_mesher_window_normals_from")


@pytest.fixture(scope="module")
def golden():
    g = {}
    for f in ("mesher.npz", "mesher_normals.npz"):
        with np.load(os.path.join(ROOT, "tests", "golden", f)) as z:
            g.update({k: z[k] for k in z.files})
    return g


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def bounds_of(nz, cuts):
    """The window bounds tests/test_mesher.py::test_z_windows_reproduce_the_single_grid_mesh uses; cuts = None: one window per
    cell layer."""
    if cuts is None:
        return list(range(nz + 1))
    return sorted({0, nz} | {max(1, min(nz - 1, int(round(c * nz)))) for c in cuts})


def seam_vertices(pos, idx, grid_offset, cell_size, planes):
    """Mask of the vertices that lie on one of the interior window planes and have a triangle that reaches below the plane and
    one that reaches above it: the vertices whose sum a lower window continues with the boundary of the upper one."""
    zc = (pos[:, 2] - grid_offset[2]) / cell_size
    tri = idx.reshape(-1, 3).astype(np.int64)
    with np.errstate(invalid="ignore"):
        tz_lo, tz_hi = np.fmin.reduce(zc[tri], axis=1), np.fmax.reduce(zc[tri], axis=1)
        out = np.zeros(len(pos), dtype=bool)
        for b in planes:
            on = np.abs(zc - b) < 1e-9
            below, above = np.zeros(len(pos), dtype=bool), np.zeros(len(pos), dtype=bool)
            for k in range(3):
                below[tri[tz_lo < b - 1e-9, k]] = True
                above[tri[tz_hi > b + 1e-9, k]] = True
            out |= on & below & above
    return out


def field_case(name, golden):
    size = nc.extra_field(name)[1] if name in nc.EXTRA_FIELDS else nc.FIELD_SIZES[name]
    return dict(size=size, **nc.FIELD_GRID), golden[f"{name}_values"]


def particle_windows(name, bounds, seed=3):
    """Windows fed as the existing window test feeds them: the particles a window can see, shuffled, with their input indices."""
    p, kw = mc.particle_case(name)
    kw = dict(kw)
    r = kw.pop("r")
    rng = np.random.default_rng(seed)
    ms = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        m = lfa.Mesher(window=(lo, hi), **kw)
        zc = (p[:, 2] - kw["grid_offset"][2]) / kw["cell_size"]
        see = np.nonzero((zc >= m.z0 - 1.0) & (zc <= m.z0 + m.n_planes + 1.0))[0]
        see = see[rng.permutation(len(see))]
        m.sample(p[see], r, ids=see.astype(np.uint32))
        m.marching_cubes()
        ms.append(m)
    return ms, kw


def field_windows(name, bounds, golden):
    kw, v = field_case(name, golden)
    ms = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        m = lfa.Mesher(window=(lo, hi), **kw)
        m.set_window_values(v)
        m.marching_cubes()
        ms.append(m)
    return ms, kw


def close_all(ms):
    for m in ms:
        m.close()


def refused(call, code=E_INVALID, word="lfa_mesher_"):
    with pytest.raises(lfa.LibfluidError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)
    return str(e.value)


# ---------------------------------------------------------------------------------------------------------- CPU
def test_window_normals_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libfluid_amd.h")).read(), flags=re.S)
    lib = lfa.load_library()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/libfluid_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in lfa.SIGNATURES
    for name in ("boundary", "window_normals", "set_window_values"):
        assert callable(getattr(lfa.Mesher, name))
    assert callable(lfa.stitch_windows)


SEAM_CASES = [(n, c) for n in ("block", "edges", "fine") for c in CUTS] + \
             [(n, c) for n in ("field1", "field3") for c in CUTS[:2] + [None]] + [(n, None) for n in nc.EXTRA_FIELDS]


@pytest.mark.parametrize("name,cuts", SEAM_CASES)
def test_the_cuts_go_through_the_surface(golden, name, cuts):
    """Every stitched case below has vertices on an interior window plane with triangles on both sides, counted from the
    fixture; on one-layer windows the extra fields keep their special vertices there: (1, 0, 0) fallbacks and the longest sums
    (zeros15, zeros30), NaN vertices and NaN normals (nan)."""
    if name in ("block", "edges", "fine"):
        kw = mc.particle_case(name)[1]
    else:
        kw = field_case(name, golden)[0]
    pos, idx, nrm = golden[f"{name}_pos"], golden[f"{name}_idx"], golden[f"{name}_normals"]
    seam = seam_vertices(pos, idx, kw["grid_offset"], kw["cell_size"], bounds_of(kw["size"][2], cuts)[1:-1])
    assert seam.sum() > 0
    if name in ("zeros15", "zeros30"):
        fell_back = nc.in_order_normals(pos, idx, with_fallback_mask=True)[1]
        valence = np.bincount(idx.astype(np.int64), minlength=len(pos))
        assert (seam & fell_back).sum() > 0 and valence[seam].max() == valence.max()
    if name == "nan":
        # (a NaN vertex has no z to place it on a plane: the seam vertices with a NaN normal have a NaN vertex as a neighbour)
        assert np.isnan(nrm[seam]).any() and np.isnan(pos).any()


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cuts", CUTS)
@pytest.mark.parametrize("name", ["block", "edges", "fine"])
def test_stitched_particle_windows(golden, name, cuts):
    ms, kw = particle_windows(name, bounds_of(mc.particle_case(name)[1]["size"][2], cuts))
    pos, idx, nrm = lfa.stitch_windows(ms, normals=True)
    close_all(ms)
    assert same(pos, golden[f"{name}_pos"]) and np.array_equal(idx, golden[f"{name}_idx"])
    assert nrm.dtype == np.float64 and same(nrm, golden[f"{name}_normals"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,cuts", [c for c in SEAM_CASES if c[0] not in ("block", "edges", "fine")])
def test_stitched_field_windows(golden, name, cuts):
    """cuts = None: one window per cell layer, the smallest shape where the first own layer is also the top layer: the vertices
    recomputed below it and the boundary imported above it meet in one layer."""
    kw = field_case(name, golden)[0]
    ms, _ = field_windows(name, bounds_of(kw["size"][2], cuts), golden)
    pos, idx, nrm = lfa.stitch_windows(ms, normals=True)
    close_all(ms)
    assert same(pos, golden[f"{name}_pos"]) and np.array_equal(idx, golden[f"{name}_idx"])
    assert same(nrm, golden[f"{name}_normals"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fine", "field1", "zeros30", "nan"])
def test_the_whole_grid_spelled_as_a_window(golden, name):
    if name == "fine":
        ms, kw = particle_windows(name, [0, mc.particle_case(name)[1]["size"][2]])
    else:
        ms, kw = field_windows(name, [0, field_case(name, golden)[0]["size"][2]], golden)
    m = ms[0]
    assert same(m.window_normals(), golden[f"{name}_normals"])
    assert same(m.normals(), golden[f"{name}_normals"]) and same(m.window_normals(None), golden[f"{name}_normals"])
    m.close()


@pytest.mark.gpu
def test_window_normals_of_all_256_cases(golden):
    m = lfa.Mesher((1, 1, 1))
    vo = k = 0
    for variant in (None, golden["cases_mags"]):
        for case in range(256):
            nv = golden["cases_counts"][k][0]
            m.set_values(mc.single_cell_values(case, None if variant is None else variant[case]))
            m.marching_cubes()
            assert same(m.window_normals(), golden["cases_normals"][vo:vo + nv]), case
            vo, k = vo + nv, k + 1
    assert k == 512
    m.close()


@pytest.mark.gpu
def test_the_boundary_is_self_contained_and_the_handle_form_gives_the_same_bits(golden):
    name = "block"
    ms, kw = particle_windows(name, bounds_of(mc.particle_case(name)[1]["size"][2], CUTS[1]))
    assert len(ms) == 3
    by_handle = [ms[0].window_normals(ms[1]), ms[1].window_normals(ms[2]), ms[2].window_normals()]
    cases, face = ms[2].boundary()
    assert cases.dtype == np.uint8 and cases.shape == (kw["size"][1], kw["size"][0]) and face.dtype == np.float64
    assert face.shape[1] == 3 and len(face) > 0 and face.shape[0] * 3 <= ms[2]._counts[1]
    cases, face = cases.copy(), face.copy()
    top = ms[2].window_normals()
    ms[2].close()  # the upper handle is gone: the copies are all the lower one gets
    mid = ms[1].window_normals((cases, face))
    b1 = tuple(a.copy() for a in ms[1].boundary())
    ms[1].close()
    low = ms[0].window_normals(b1)
    ms[0].close()
    for a, b in zip(by_handle, (low, mid, top)):
        assert same(a, b)
    assert same(np.concatenate([low, mid, top]), golden[f"{name}_normals"])


@pytest.mark.gpu
def test_empty_windows_and_an_empty_boundary(golden):
    """`sparse` has no surface at all; `block` cut so that the top window and the boundary it exports are empty."""
    ms, kw = particle_windows("sparse", [0, 4, 9])
    cases, face = ms[1].boundary()
    assert not cases.any() and face.shape == (0, 3)
    pos, idx, nrm = lfa.stitch_windows(ms, normals=True)
    assert len(pos) == 0 and len(idx) == 0 and nrm.shape == (0, 3)
    guard = np.full(6, 7.0)
    ms[0]._chk(ms[0].lib.lfa_mesher_download_normals(ms[0].h, guard.ctypes.data_as(lfa.C.c_void_p)))  # LFA_OK, nothing written
    assert (guard == 7.0).all()
    close_all(ms)
    nz = mc.particle_case("block")[1]["size"][2]
    ms, kw = particle_windows("block", [0, nz - 1, nz])
    assert ms[1]._counts == (0, 0) and ms[1].boundary()[1].shape == (0, 3)
    pos, idx, nrm = lfa.stitch_windows(ms, normals=True)
    close_all(ms)
    assert same(nrm, golden["block_normals"])


@pytest.mark.gpu
def test_state_and_refusal_rules(golden):
    name = "field1"
    kw, v = field_case(name, golden)
    nz = kw["size"][2]
    ms, _ = field_windows(name, [0, 2, 3, nz], golden)
    lo, mid, top = ms
    want = lfa.stitch_windows(ms, normals=True)[2]
    assert same(want, golden[f"{name}_normals"])
    # lfa_mesher_normals stays whole-grid only
    for m in ms:
        refused(m.compute_normals, E_UNSUPPORTED, "window")
    refused(lo.boundary)                                        # own_lo == 0: nothing lies below it
    refused(lambda: lo.window_normals())                        # a missing boundary below the top
    refused(lo.download_normals)                                # ... leaves no normals
    refused(lambda: top.window_normals(top.boundary()))         # a surplus one on the top
    refused(lambda: top.window_normals(mid))
    cases, face = mid.boundary()
    refused(lambda: lo.window_normals((cases, face[:-1])))      # a wrong n_triangles
    refused(lambda: lo.window_normals((cases, np.concatenate([face, face[:1]]))))
    refused(lambda: lo.window_normals(top))                     # not the window directly above
    refused(lambda: lo.window_normals(lo))
    msg = refused(lambda: lo.window_normals(top.boundary()))    # its boundary does not fit either: count or corner signs
    assert "triangles" in msg or "cell (" in msg
    other = lfa.Mesher(window=(2, 3), **dict(kw, cell_size=kw["cell_size"] * 2))
    other.set_window_values(v)
    other.marching_cubes()
    refused(lambda: lo.window_normals(other))                   # another grid
    other.close()
    assert same(lo.window_normals(mid), want[:lo._counts[0]])   # (and a refusal spoils nothing)
    assert lo.normals_ms() > 0.0 and same(lo.download_normals(), want[:lo._counts[0]])
    # stale after upload_values and marching_cubes
    mid.set_window_values(v)
    refused(mid.boundary)
    refused(lambda: lo.window_normals(mid))
    refused(lambda: mid.window_normals(top))
    mid.marching_cubes()
    refused(mid.download_normals)
    refused(mid.normals_ms)
    assert same(mid.window_normals(top), want[lo._counts[0]:lo._counts[0] + mid._counts[0]])
    lo.marching_cubes()
    refused(lo.download_normals)
    assert same(lo.window_normals(mid.boundary()), want[:lo._counts[0]])
    close_all(ms)


@pytest.mark.gpu
def test_a_stale_boundary_is_refused_by_the_consistency_check(golden):
    """The upper window is re-sampled with other particles after its boundary was taken: the old boundary no longer is what lies
    above the lower window... and, the other way round, the lower window moves on: the corner signs on the shared plane differ."""
    p, kw = mc.particle_case("block")
    kw = dict(kw)
    r = kw.pop("r")
    nz = kw["size"][2]
    ids = np.arange(len(p), dtype=np.uint32)
    lo, up = lfa.Mesher(window=(0, nz // 2), **kw), lfa.Mesher(window=(nz // 2, nz), **kw)
    for m in (lo, up):
        m.sample(p, r, ids=ids)
        m.marching_cubes()
    old = tuple(a.copy() for a in up.boundary())
    want = lo.window_normals(old)
    assert same(want, golden["block_normals"][:len(want)])
    fewer = p[p[:, 0] < 6.0]                                     # another surface through the shared plane
    up.sample(fewer, r)
    refused(up.boundary)                                         # sampled, not yet extracted: no boundary
    up.marching_cubes()
    new = up.boundary()
    assert not np.array_equal(new[0] & 0xF, old[0] & 0xF)
    msg = refused(lambda: lo.window_normals(new))
    assert "cell (" in msg and f"layer {nz // 2}" in msg
    refused(lambda: lo.window_normals(up))
    refused(lo.download_normals)
    lo.sample(fewer, r)                                          # the lower window follows: now the old one is stale
    lo.marching_cubes()
    msg = refused(lambda: lo.window_normals(old))
    assert "cell (" in msg or "triangles" in msg
    got = lo.window_normals(new)
    whole = lfa.Mesher(**kw)
    pos, idx, nrm = whole.generate_mesh(fewer, r, normals=True)
    assert len(got) > 0 and same(got, nrm[:len(got)]) and same(up.window_normals(), nrm[len(got):])
    for m in (lo, up, whole):
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(5, 0), (0, 12345678901), (390, 7)])
def test_rebasing_either_handle_before_or_after_changes_nothing(golden, shift):
    name = "edges"
    ms, kw = particle_windows(name, bounds_of(8, CUTS[0]))
    lo, up = ms
    n_lo = lo._counts[0]
    want = golden[f"{name}_normals"]
    lo.rebase(shift[0]); up.rebase(shift[1])                     # before anything was computed
    assert same(lo.window_normals(up), want[:n_lo]) and same(up.window_normals(), want[n_lo:])
    b = up.boundary()
    up.rebase(3); lo.rebase(11)                                  # after: cached face vectors, shifted index lists
    assert same(lo.window_normals(up), want[:n_lo]) and same(lo.window_normals(b), want[:n_lo])
    assert same(up.window_normals(), want[n_lo:]) and same(up.boundary()[1], b[1])
    up.marching_cubes()                                          # a new extraction starts from unshifted indices
    up.rebase(n_lo)
    assert same(up.boundary()[1], b[1]) and same(up.window_normals(), want[n_lo:])
    assert np.array_equal(np.concatenate([lo.download_mesh()[1] - np.uint64(shift[0] + 11), up.download_mesh()[1]]),
                          golden[f"{name}_idx"])
    close_all(ms)


@pytest.mark.gpu
def test_a_window_that_never_asks_allocates_nothing_more(golden):
    """lfa_pool_stats, as tests/test_mesher_normals.py does for the whole grid: a window that only meshes requests what it
    requested before this feature existed (the same as a handle of the same history); the buffers of the window normals are
    requested by the first call that needs them and reused afterwards."""
    p, kw = mc.particle_case("block")
    kw = dict(kw)
    r = kw.pop("r")
    nz = kw["size"][2]
    ids = np.arange(len(p), dtype=np.uint32)

    def requests():
        s = lfa.pool_stats()
        return s["hits"] + s["misses"]

    def mesh_only(m):
        m.sample(p, r, ids=ids)
        return m.marching_cubes()

    lfa.Mesher(window=(0, nz // 2), **kw).close()
    n0 = requests()
    m = lfa.Mesher(window=(nz // 2, nz), **kw)
    mesh_only(m)
    m.rebase(5)
    plain = requests() - n0
    m.close()
    n0 = requests()
    up = lfa.Mesher(window=(nz // 2, nz), **kw)
    mesh_only(up)
    up.rebase(5)
    assert requests() - n0 == plain
    lo = lfa.Mesher(window=(0, nz // 2), **kw)
    mesh_only(lo)
    n1 = requests()
    up.boundary()
    assert requests() - n1 == 2          # face vectors + the recomputed vertices of the layer below
    up.window_normals()
    assert requests() - n1 == 3          # + normals; the top window imports nothing
    n2 = requests()
    a = lo.window_normals(up)
    assert requests() - n2 == 6          # normals, face vectors; imported cases, offsets, flag word, face vectors
    n3 = requests()
    mesh_only(up); mesh_only(lo)
    b = lo.window_normals(up.boundary())
    up.window_normals()
    assert requests() == n3 and same(a, b)
    assert same(np.concatenate([b, up.download_normals()]), golden["block_normals"])
    lo.close(); up.close()


@pytest.mark.gpu
def test_the_two_entry_points_share_one_path_and_one_state(golden):
    """lfa_mesher_normals is the window path without a boundary: on a whole-grid handle either entry point gives the reference's
    rows from the same two buffers, whatever lfa_mesher_rebase did in between (the cached face vectors are those of the unshifted
    mesh); on a window the refusal comes before the state is touched; every refusal names the entry point that was called."""
    name = "field1"
    kw, v = field_case(name, golden)
    want = golden[f"{name}_normals"]

    def requests():
        s = lfa.pool_stats()
        return s["hits"] + s["misses"]

    m = lfa.Mesher(**kw)
    msg = refused(m.compute_normals, E_INVALID, "lfa_mesher_normals")  # before any extraction
    assert "lfa_mesher_window_normals" not in msg
    m.set_values(v)
    m.marching_cubes()
    assert same(m.normals(), want) and m.normals_ms() > 0.0
    n1 = requests()
    m.rebase(5)
    assert same(m.window_normals(), want) and m.normals_ms() > 0.0
    assert same(m.normals(), want) and m.normals_ms() > 0.0
    assert requests() == n1              # both entry points use the same two buffers
    m.close()

    ms, _ = field_windows(name, [0, 2, 3, kw["size"][2]], golden)
    lo, mid, top = ms
    rows = lo.window_normals(mid)
    assert same(rows, want[:lo._counts[0]])
    refused(lo.compute_normals, E_UNSUPPORTED, "window")
    assert same(lo.download_normals(), rows)  # the refusal spoils nothing
    close_all(ms)


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", [[0, 2, 4], [0, 1, 2, 3, 4]])
def test_slab_ranks_stitch_their_normals(bounds):
    """The run of tests/test_gpu_slabs.py::test_slab_ranks_mesh_their_windows_into_the_single_domain_mesh with normals. The
    particles of a slab run differ from the single domain's by the solver's fp32 summation orders (~1e-6), so the single-domain
    handle the stitched normals are compared with bit for bit is a whole-grid Mesher holding the ranks' own samples (the planes
    two windows both sample agree bit for bit: ghost particles are copies); the single-domain run itself is the bar for the
    topology."""
    size, block = (16, 16, 32), ((2, 0, 3), (14, 10, 29))
    mkw = dict(size=size, grid_offset=(0.0, 0.0, 0.0), cell_size=1.0, particle_extent=1.0, cell_radius=2)
    s = lfa.Sim(size, method=lfa.APIC)
    s.seed_block(*block)
    for _ in range(2):
        s.time_step(util.DT)
    m = lfa.Mesher(**mkw)
    m.sample_sim(s, 0.5)
    want_pos, want_idx = m.marching_cubes()
    want_nrm = m.normals()
    m.close(); s.close()
    assert len(want_idx) > 1000

    n = len(bounds) - 1
    hub = lfa.LocalHub(n)
    sims = []
    for r in range(n):
        t = lfa.Sim(size, method=lfa.APIC)
        t.init_local_slab(hub.h, r, bounds)
        t.seed_block(*block)
        sims.append(t)
    meshes, errors = [None] * n, []

    def worker(r):
        try:
            for _ in range(2):
                sims[r].time_step(util.DT)
            sims[r].hash()
            lo, hi = sims[r].slab()
            mm = lfa.Mesher(window=(lo * 8, min(hi * 8, size[2])), **mkw)
            mm.sample_sim(sims[r], 0.5)
            mm.marching_cubes()
            meshes[r] = mm
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=90)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), "slab threads hung"
    pos, idx, nrm = lfa.stitch_windows(meshes, normals=True)
    field = np.empty((size[2] + 1, size[1] + 1, size[0] + 1))
    for mm in meshes:
        lo, hi = mm.own
        s_lo = max(lo - 1, 0)
        got = mm.values()[s_lo - mm.z0: hi - mm.z0 + 1]
        if lo > 0:
            assert same(got[:2], field[s_lo: lo + 1])  # the planes the window below has sampled too
        field[s_lo: hi + 1] = got
        mm.close()
    for t in sims:
        t.close()
    hub.close()
    m = lfa.Mesher(**mkw)
    m.set_values(field)
    p1, i1 = m.marching_cubes()
    assert same(p1, pos) and np.array_equal(i1, idx)
    assert same(m.normals(), nrm)
    m.close()
    assert same(nc.in_order_normals(pos, idx), nrm)
    assert np.array_equal(idx, want_idx) and np.array_equal(np.isnan(nrm), np.isnan(want_nrm))
