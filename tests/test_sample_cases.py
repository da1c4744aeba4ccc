"""CPU tests of tests/sample_cases.py: the oracle is the compiled reference on exactly these points (tolerance 0 - without that a
device-against-oracle comparison on them proves nothing), the point set holds what it promises (conditions on the inputs, asserted
and not measured), the inside test is false for everything that is no point of the box, and the C ABI of the velocity sampling is
declared, exported and bound. tests/test_gpu_sample.py compares the device with the model."""
import os
import re

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import sample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lfa_sample_velocity", "lfa_sample_velocity_time", "lfa_mesher_vertex_velocities", "lfa_mesher_download_velocities",
           "lfa_mesher_velocities_time")


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
def test_oracle_is_the_reference_on_the_case_set():
    pts, cells = sc.points(), sc.random_field()
    want = sc.model(cells, pts, "ref")
    got = sc.model(cells, pts, "oracle")
    inside = sc.classify(pts)[1]
    assert got[0][inside].tobytes() == want[0][inside].tobytes()
    assert got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    assert np.abs(got[0][inside]).max() > 1.0  # (the field is not trivial)


def test_the_point_set_holds_what_it_promises():
    pts = sc.points()
    fi, inside = sc.classify(pts)
    assert len(pts) == 576 * 16 + sc.N_RANDOM + 11 + 3
    assert int((~inside).sum()) == 10
    crosses, clamped = sc.neighbourhood_stats(pts)
    assert int((crosses == 3).sum()) >= 1000
    assert int((clamped == 3).sum()) >= 400
    # every one of the 8 fractions occurs on every axis
    lattice, built, which = sc.lattice()
    assert len(lattice) == 576 * 16
    for axis in range(3):
        assert set(which[:, axis]) == set(range(8))
    # the division hazard the offset was chosen for: off + c h, divided by h again, lands in the cell below
    lf, lin = sc.classify(lattice)
    assert lin.all()
    got = sc.cells_of(lf)
    assert (got <= built).all() and (got >= built - 1).all()
    assert int((got < built).any(axis=1).sum()) >= 1
    # the far face on z alone lands INSIDE (5.1 / 0.3 rounds below 17): only the division decides
    block = sc.outside_block()
    assert sc.classify(block)[1].tolist() == [False] * 5 + [True] + [False] * 5
    assert sc.classify(sc.corner_checks())[1].all()
    # the lattice reaches both ends of every axis and both sides of every tile face
    for axis, n in enumerate(sc.SIZE):
        assert set(sc.axis_cells(n)) <= set(got[:, axis].tolist())


def test_the_classification_is_false_for_what_is_no_point_of_the_box():
    inside_point = np.array(sc.OFFSET) + np.array([3.5, 3.5, 3.5]) * sc.H
    assert sc.classify(inside_point)[1].all()
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300, 1e19, -1e19, 2.0 ** 31 * sc.H, 2.0 ** 63 * sc.H, 2.0 ** 64 * sc.H):
        for axis in range(3):
            p = inside_point.copy()
            p[axis] = bad
            fi, inside = sc.classify(p)
            assert fi.dtype == np.float64  # decided on the doubles: no cast comes before the comparison
            assert not inside.any(), (bad, axis)
    # the model returns +0.0 (not -0.0), type 0, and counts
    pts = np.array([[np.nan, 0.0, 0.0], [-1e300, 1e300, 0.0]])
    vel, types, n_out = sc.model(sc.random_field(), pts)
    assert n_out == 2 and not types.any() and vel.tobytes() == np.zeros((2, 3)).tobytes()


def test_sampling_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = lfa.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/libfluid_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in lfa.SIGNATURES
    decl = {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\bint\s+(lfa_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert decl["lfa_sample_velocity"] == "lfa_sim *s, const double *xyz, uint64_t n, double *velocity, uint8_t *types, uint64_t *n_outside"
    assert decl["lfa_sample_velocity_time"] == "lfa_sim *s, double *ms"
    assert decl["lfa_mesher_vertex_velocities"] == "lfa_mesher *m, lfa_sim *s, uint64_t *n_outside"
    assert decl["lfa_mesher_download_velocities"] == "lfa_mesher *m, double *velocity"
    assert decl["lfa_mesher_velocities_time"] == "lfa_mesher *m, double *ms"
    # the binding's prototypes are the declared ones
    import ctypes as C
    vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
    assert lfa.SIGNATURES["lfa_sample_velocity"] == (C.c_int, [vp, vp, u64, vp, vp, C.POINTER(u64)])
    assert lfa.SIGNATURES["lfa_sample_velocity_time"] == (C.c_int, [vp, C.POINTER(dbl)])
    assert lfa.SIGNATURES["lfa_mesher_vertex_velocities"] == (C.c_int, [vp, vp, C.POINTER(u64)])
    assert lfa.SIGNATURES["lfa_mesher_download_velocities"] == (C.c_int, [vp, vp])
    assert lfa.SIGNATURES["lfa_mesher_velocities_time"] == (C.c_int, [vp, C.POINTER(dbl)])
    # every entry cites the reference lines of the definition
    for cite in ("src/simulation.cpp:447-461", "src/mac_grid.cpp:42-112", "include/fluid/misc.h:20-36", "src/simulation.cpp:17-23"):
        assert cite in header
    assert callable(lfa.Sim.sample_velocity) and callable(lfa.Sim.sample_velocity_ms)
    assert callable(lfa.Mesher.vertex_velocities) and callable(lfa.Mesher.velocities_ms)
    assert "sample.hip" in open(os.path.join(ROOT, "libfluid_amd", "build.py")).read()


def _have_hipcc():
    import shutil
    return any(c and (shutil.which(c) or os.path.exists(c)) for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"))


@pytest.mark.skipif(not _have_hipcc(), reason="no hipcc on this machine")
def test_k_sample_velocity_uses_no_scratch_and_spills_nothing():
    """The compiler's own metadata (tools/kernel_resources.py compiles sample.hip for gfx950; nothing runs on a device): 24 fp64
    samples per lane fit the registers - beyond the budget the compiler spills to scratch without a word. The VGPR bound is the
    one of 5 waves per SIMD (512 / 5 in granules of 8: 96), the occupancy the kernel was recorded with at 84 VGPRs."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sample.hip", "k_sample_velocity"],
                         capture_output=True, text=True, check=True).stdout
    print(out)
    m = re.search(r"k_sample_velocity\(.*vgpr\s+(\d+) sgpr\s+(\d+) spill\s+(\d+) lds\s+(\d+) scratch\s+(\d+)", out)
    assert m, out
    vgpr, sgpr, spill, lds, scratch = (int(x) for x in m.groups())
    assert vgpr <= 96 and spill == 0 and scratch == 0 and lds == 0, (vgpr, spill, lds, scratch)
