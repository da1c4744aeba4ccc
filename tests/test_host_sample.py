"""sample_velocity() of the C++ host class (libfluid_amd/host/simulation.h) and vertex_velocities() of the mesher
(libfluid_amd/host/mesher.h) through tests/host_sample_driver.cpp: the grid of tests/sample_cases.py with a seeded box, three
time_step()s, the case set's points. The bar is that of tests/test_gpu_sample.py: the model (the oracle's PIC transfer) on the grid
that grid() shows, byte for byte - also after an edit through grid() that no step has carried to the device."""
import os
import subprocess

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import sample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "host_sample_driver.cpp")
EDITED_CELL = 8 + sc.SIZE[0] * (8 + sc.SIZE[1] * 8)  # (the driver's)


def build_driver(tmp_path):
    exe = str(tmp_path / "host_sample_driver")
    lfa.load_library()
    cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-Wextra", *os.environ.get("LFA_HOST_CXXFLAGS", "").split(), "-o", exe,
           DRIVER_SRC, "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return exe


def test_host_sample_driver_compiles_and_links(tmp_path):
    build_driver(tmp_path)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_sample")
    exe = build_driver(out)
    points = sc.points()
    points.tofile(out / "points.bin")
    r = subprocess.run([exe, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = {"points": points}
    for tag in ("step3", "edit"):
        rec[tag] = dict(vel=np.fromfile(out / (tag + "_velocity.bin"), dtype=np.float64).reshape(-1, 3),
                        types=np.fromfile(out / (tag + "_types.bin"), dtype=np.uint8),
                        outside=int(np.fromfile(out / (tag + "_outside.bin"), dtype=np.uint64)[0]),
                        grid=np.fromfile(out / (tag + "_grid.bin"), dtype=lfa.CELL_DTYPE))
    for name in ("positions", "vertex_velocities", "sampled"):
        rec["mesh_" + name] = np.fromfile(out / ("mesh_" + name + ".bin"), dtype=np.float64).reshape(-1, 3)
    rec["mesh_outside"] = np.fromfile(out / "mesh_outside.bin", dtype=np.uint64)
    return rec


def against_model(rec, tag):
    q = rec[tag]
    want_vel, want_types, want_out = sc.model(q["grid"], rec["points"])
    bad = np.flatnonzero((q["vel"].view(np.uint64) != want_vel.view(np.uint64)).any(axis=1))
    print(tag, "points", len(rec["points"]), "outside", q["outside"], "rows that differ", len(bad))
    assert q["vel"].tobytes() == want_vel.tobytes(), (tag, bad[:8])
    assert q["types"].tobytes() == want_types.tobytes() and q["outside"] == want_out == 10, tag


@pytest.mark.gpu
def test_sample_velocity_answers_for_the_grid_that_grid_shows(run):
    against_model(run, "step3")
    assert np.abs(run["step3"]["grid"]["vel"]).max() > 0.0 and np.abs(run["step3"]["vel"]).max() > 0.0


@pytest.mark.gpu
def test_an_edit_through_grid_is_seen_without_a_step(run):
    against_model(run, "edit")
    before, after = run["step3"]["grid"], run["edit"]["grid"]
    changed = np.flatnonzero((before["vel"] != after["vel"]).any(axis=1))
    # the edited cell holds the edit; the upload stores fp32, so a value that was no fp32 number (an implicit tile's background)
    # may have been rounded - grid() shows what the device holds, and the sample answers for that
    assert EDITED_CELL in changed and np.array_equal(after["vel"][EDITED_CELL], [1.25, -2.5, 3.75])
    others = changed[changed != EDITED_CELL]
    assert np.array_equal(after["vel"][others], before["vel"][others].astype(np.float32).astype(np.float64))
    assert np.array_equal(after["type"], before["type"])
    assert run["edit"]["vel"].tobytes() != run["step3"]["vel"].tobytes()


@pytest.mark.gpu
def test_vertex_velocities_equal_the_sample_at_the_meshs_positions(run):
    assert len(run["mesh_positions"]) > 100
    assert run["mesh_vertex_velocities"].tobytes() == run["mesh_sampled"].tobytes()
    assert run["mesh_outside"][0] == run["mesh_outside"][1]
    assert np.abs(run["mesh_vertex_velocities"]).max() > 0.0
