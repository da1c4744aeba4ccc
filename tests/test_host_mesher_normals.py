"""fluid_amd::mesher::generate_mesh_with_normals (libfluid_amd/host/mesher.h): generate_mesh + mesh::generate_normals() in one
call, the normals computed on the device.

CPU: tests/host_normals_driver.cpp compiles (g++ -Wall -Wextra) and links against the standalone value types and, where the
reference's headers exist, with the shim in front of them, where mesh_t is the reference's own fluid::mesh.
GPU: positions, indices and normals equal the fixtures bitwise, and the driver finds the device's normals byte-identical to
mesh_t::generate_normals() of the same mesh (exit code 5 otherwise): the host loop and the device path are the same function."""
import os
import subprocess

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import callers_util
from tests import mesher_cases as mc
from tests import mesher_normals_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_normals_driver.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesher.npz")
GOLDEN_NORMALS = os.path.join(ROOT, "tests", "golden", "mesher_normals.npz")


def build_driver(tmp_path, reference_types=False):
    exe = str(tmp_path / ("host_normals_driver" + ("_reftypes" if reference_types else "")))
    lfa.load_library()
    inc = ["-I" + callers_util.SHIM, "-I" + callers_util.REF_INCLUDE] if reference_types else []
    cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-Wextra", *os.environ.get("LFA_HOST_CXXFLAGS", "").split(), *inc,
           "-o", exe, SRC, "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def read_mesh(path):
    raw = open(path, "rb").read()
    nv, ni = (int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=2))
    pos = np.frombuffer(raw, dtype=np.float64, count=3 * nv, offset=16).reshape(-1, 3)
    idx = np.frombuffer(raw, dtype=np.uint64, count=ni, offset=16 + 24 * nv)
    nrm = np.frombuffer(raw, dtype=np.float64, count=3 * nv, offset=16 + 24 * nv + 8 * ni).reshape(-1, 3)
    assert len(raw) == 16 + 48 * nv + 8 * ni
    return pos, idx, nrm


def test_host_driver_compiles_and_links(tmp_path):
    build_driver(tmp_path)


@pytest.mark.skipif(not callers_util.have_reference(), reason="the reference's headers are not on this machine")
def test_host_driver_compiles_with_the_references_own_mesh_type(tmp_path):
    build_driver(tmp_path, reference_types=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["block", "fine"])
def test_generate_mesh_with_normals_matches_reference(tmp_path, name):
    with np.load(GOLDEN) as z:
        want_pos, want_idx = z[f"{name}_pos"], z[f"{name}_idx"]
    with np.load(GOLDEN_NORMALS) as z:
        want_nrm = z[f"{name}_normals"]
    p, kw = mc.particle_case(name)
    exe = build_driver(tmp_path)
    p.tofile(tmp_path / "p.bin")
    args = [exe, str(tmp_path / "p.bin"), *(str(x) for x in kw["size"]), *(repr(float(x)) for x in kw["grid_offset"]),
            repr(kw["cell_size"]), repr(kw["particle_extent"]), str(kw["cell_radius"]), repr(kw["r"]), str(tmp_path / "m.bin")]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    pos, idx, nrm = read_mesh(tmp_path / "m.bin")
    assert np.array_equal(pos, want_pos) and np.array_equal(idx, want_idx)
    assert not np.isnan(nrm).any() and np.array_equal(nrm, want_nrm)  # (no NaN: the driver's comparison was byte for byte)


@pytest.mark.gpu
def test_generate_mesh_with_normals_from_a_simulation(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, "sim", "24", "0.5", str(tmp_path / "m.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    pos, idx, nrm = read_mesh(tmp_path / "m.bin")
    assert len(idx) > 1000 and nrm.shape == pos.shape
    assert np.array_equal(nrm, nc.in_order_normals(pos, idx), equal_nan=True)
