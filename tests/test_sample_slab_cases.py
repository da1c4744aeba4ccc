"""CPU tests of tests/sample_slab_cases.py: the conditions on the inputs that tests/test_gpu_sample_slabs.py relies on, asserted and
not measured - every rank of every decomposition owns points whose block reads each ghost layer it has, the division decides
owners on the face z = 8, the particles leave fluid on both sides of both faces and some tiles implicit - and the declaration,
export and binding of the two collective entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import sample_cases as sc
from tests import sample_slab_cases as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = sc.points()


def test_grid_and_points_are_those_of_the_single_domain_cases():
    assert sc.SIZE == (40, 24, 17) and sc.H == 0.3 and sc.OFFSET == (0.69, -0.35, 15.3)
    assert len(POINTS) == 13326 and ss.N_TILE_LAYERS == 3
    assert [list(b) for b in ss.BOUNDS] == [[0, 1, 3], [0, 2, 3], [0, 1, 2, 3]]
    for b in ss.BOUNDS:
        assert b[0] == 0 and b[-1] == ss.N_TILE_LAYERS
    assert ss.window([0, 1, 2, 3], 2) == (16, 17)  # the smallest slab there is: one cell layer


@pytest.mark.parametrize("bounds", ss.BOUNDS, ids=str)
def test_every_rank_owns_points_that_read_each_of_its_ghost_layers(bounds):
    own = ss.owner(POINTS, bounds)
    inside = sc.classify(POINTS)[1]
    assert int((own < 0).sum()) == int((~inside).sum()) == 10
    below, above = ss.reads_ghost(POINTS, bounds)
    counts = []
    for r in range(len(bounds) - 1):
        assert int((own == r).sum()) >= 1000
        if r > 0:
            counts.append(int((below & (own == r)).sum()))
        if r + 2 < len(bounds):
            counts.append(int((above & (own == r)).sum()))
    print(bounds, "owned points whose block reads a ghost layer, per face and side:", counts)
    assert min(counts) >= 1000, counts
    # the ranks partition the inside points
    assert sorted(set(own[inside].tolist())) == list(range(len(bounds) - 1))


def test_only_the_division_decides_the_owner_on_the_face_z_8():
    lattice, built, _ = sc.lattice()
    fi, inside = sc.classify(lattice)
    got = sc.cells_of(fi)
    slipped = (built[:, 2] == 8) & (got[:, 2] == 7)
    print("lattice points built for cell z = 8 that land in cell 7:", int(slipped.sum()))
    assert inside.all() and int(slipped.sum()) >= 100
    own = ss.owner(lattice, [0, 1, 3])
    assert (own[slipped] == 0).all() and (own[(built[:, 2] == 8) & ~slipped] == 1).all()


def test_owner_and_stitch():
    pts = np.array(sc.OFFSET) + np.array([[3.5, 3.5, 7.5], [3.5, 3.5, 8.5], [3.5, 3.5, 16.5], [3.5, 3.5, 17.5], [np.nan, 0.0, 0.0]]) * sc.H
    assert ss.owner(pts, [0, 1, 3]).tolist() == [0, 1, 1, -1, -1]
    assert ss.owner(pts, [0, 2, 3]).tolist() == [0, 0, 1, -1, -1]
    assert ss.owner(pts, [0, 1, 2, 3]).tolist() == [0, 1, 2, -1, -1]
    nx, ny, nz = sc.SIZE
    ranks = []
    for r in range(3):
        c = np.zeros(nx * ny * nz, dtype=lfa.CELL_DTYPE)
        c["type"] = r + 1
        ranks.append(c)
    got = ss.stitch(ranks, [0, 1, 2, 3])["type"].reshape(nz, ny, nx)
    assert (got[:8] == 1).all() and (got[8:16] == 2).all() and (got[16:] == 3).all()
    assert ss.reach([0, 1, 2, 3], 1, nz) == (1, 17) and ss.reach([0, 2, 3], 0, nz) == (0, 17) and ss.reach([0, 2, 4], 1, 32) == (9, 32)
    assert ss.reach([0, 2, 4], 0, 32) == (0, 23)


def test_the_particles_leave_fluid_on_both_sides_of_both_faces_and_implicit_tiles():
    parts = ss.slab_particles()
    assert len(parts) == len(sc.sparse_particles()) + 1200
    sim = orc.CpuSim(sc.SIZE, cell_size=sc.H, offset=sc.OFFSET, gravity=sc.GRAVITY, method=orc.PIC)
    sim.set_particles(parts)
    sim.hash()
    sim.p2g()
    types = sim.cells()["type"].reshape(sc.SIZE[2], sc.SIZE[1], sc.SIZE[0])
    sim.close()
    for face in ss.FACES:
        below, above = int((types[face - 1] == orc.FLUID).sum()), int((types[face] == orc.FLUID).sum())
        print("fluid cells in the layers", face - 1, "and", face, ":", below, above)
        assert below >= 10 and above >= 10
    # particle tiles, dilated by one tile: the set the device grid is explicit on
    fi, inside = sc.classify(parts["pos"])
    assert inside.all()
    tiles = np.zeros((3, 3, 5), dtype=bool)
    t = sc.cells_of(fi) >> 3
    tiles[t[:, 2], t[:, 1], t[:, 0]] = True
    dil = np.zeros_like(tiles)
    for z, y, x in np.argwhere(tiles):
        dil[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    assert 0 < int((~dil).sum()) and not dil[ss.SEED_TILE[2], ss.SEED_TILE[1], ss.SEED_TILE[0]]
    # implicit and explicit tiles meet on both slab faces
    for layer in (1, 2):
        assert (dil[layer - 1] != dil[layer]).any() or ((~dil[layer]).any() and dil[layer].any())
    # the seed box of state (d) lies inside its tile, away from every particle tile's own cells
    lo = (ss.SEED_BOX[0] - np.array(sc.OFFSET)) / sc.H
    hi = lo + ss.SEED_BOX[1] / sc.H
    assert (np.floor(lo).astype(int) >> 3).tolist() == list(ss.SEED_TILE) and (np.floor(hi).astype(int) >> 3).tolist() == list(ss.SEED_TILE)


def test_collective_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\bint\s+(lfa_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert decl["lfa_sample_velocity_collective"] == ("lfa_sim *s, const double *xyz, uint64_t n, uint32_t *index, double *velocity, "
                                                      "uint8_t *types, uint64_t capacity, uint64_t counts[3]")
    assert decl["lfa_mesher_vertex_velocities_collective"] == "lfa_mesher *m, lfa_sim *s, uint64_t counts[2]"
    # the existing calls keep their signatures
    assert decl["lfa_sample_velocity"] == "lfa_sim *s, const double *xyz, uint64_t n, double *velocity, uint8_t *types, uint64_t *n_outside"
    assert decl["lfa_mesher_vertex_velocities"] == "lfa_mesher *m, lfa_sim *s, uint64_t *n_outside"
    lib = lfa.load_library()
    vp, u64 = C.c_void_p, C.c_uint64
    for name in ("lfa_sample_velocity_collective", "lfa_mesher_vertex_velocities_collective"):
        assert hasattr(lib, name), f"{name} is not exported"
    assert lfa.SIGNATURES["lfa_sample_velocity_collective"] == (C.c_int, [vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64 * 3)])
    assert lfa.SIGNATURES["lfa_mesher_vertex_velocities_collective"] == (C.c_int, [vp, vp, C.POINTER(u64 * 2)])
    assert callable(lfa.Sim.sample_velocity_collective) and callable(lfa.Mesher.vertex_velocities_collective)
    # the header says what a host has to know: the call is collective, and a lone failure is the rank's own
    for phrase in ("COLLECTIVE", "lfa_hash_particles", "NEW collective call"):
        assert phrase in header


def _have_hipcc():
    import shutil
    return any(c and (shutil.which(c) or os.path.exists(c)) for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"))


@pytest.mark.skipif(not _have_hipcc(), reason="no hipcc on this machine")
def test_the_sampling_kernels_use_no_scratch():
    """The compiler's own metadata (tools/kernel_resources.py compiles sample.hip for gfx950; nothing runs on a device): the dense
    kernel stays within a few VGPRs of the 84 it had before the shared device functions and the cell-z range, and the write pass -
    the same 24 fp64 samples per lane plus the compaction - spills nothing either."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sample.hip", "k_sample_"],
                         capture_output=True, text=True, check=True).stdout
    print(out)
    seen = {}
    for m in re.finditer(r"(k_sample_\w+)\(.*vgpr\s+(\d+) sgpr\s+(\d+) spill\s+(\d+) lds\s+(\d+) scratch\s+(\d+)", out):
        seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert {"k_sample_velocity", "k_sample_count", "k_sample_write"} <= set(seen), out
    for name, (vgpr, sgpr, spill, lds, scratch) in seen.items():
        assert spill == 0 and scratch == 0 and lds == 0, (name, spill, lds, scratch)
    assert abs(seen["k_sample_velocity"][0] - 84) <= 4, seen["k_sample_velocity"]
    assert seen["k_sample_write"][0] <= 96, seen["k_sample_write"]  # 5 waves per SIMD, like the dense kernel
