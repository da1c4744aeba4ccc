"""Tracers of the C++ host class (libfluid_amd/host/simulation.h) through tests/host_tracer_driver.cpp: the grid of
tests/sample_cases.py with a seeded box, tracers started inside it, three time_step(dt)s with a fixed dt. After the last step a
tracer's velocity is the PIC transfer of the grid that grid() shows at the tracer's position - the model of tests/sample_cases.py,
byte for byte - on the one-call path and on the staged path alike; with advance_tracers = false the tracers stay where they were."""
import os
import subprocess

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import sample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "host_tracer_driver.cpp")
N = 257


def start_state():
    """Tracers inside the seeded box (cells [2, 11) x [2, 9) x [2, 8)) with velocities of up to two cells per step."""
    rng = np.random.default_rng(sc.SEED + 7)
    pos = np.array(sc.OFFSET) + (np.array([2.0, 2.0, 2.0]) + rng.random((N, 3)) * np.array([9.0, 7.0, 6.0])) * sc.H
    vel = (rng.random((N, 3)) - 0.5) * 4.0 * sc.H / 0.005
    return pos, vel


def build_driver(tmp_path):
    exe = str(tmp_path / "host_tracer_driver")
    lfa.load_library()
    cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-Wextra", *os.environ.get("LFA_HOST_CXXFLAGS", "").split(), "-o", exe,
           DRIVER_SRC, "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return exe


def test_host_tracer_driver_compiles_without_warnings(tmp_path):
    build_driver(tmp_path)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_tracers")
    exe = build_driver(out)
    pos, vel = start_state()
    np.concatenate([pos, vel]).tofile(out / "tracers.bin")
    r = subprocess.run([exe, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = {"pos0": pos, "vel0": vel}
    for tag in ("fused", "staged", "off"):
        rec[tag] = dict(pos=np.fromfile(out / (tag + "_pos.bin"), dtype=np.float64).reshape(-1, 3),
                        vel=np.fromfile(out / (tag + "_vel.bin"), dtype=np.float64).reshape(-1, 3),
                        types=np.fromfile(out / (tag + "_types.bin"), dtype=np.uint8),
                        grid=np.fromfile(out / (tag + "_grid.bin"), dtype=lfa.CELL_DTYPE),
                        calls=int(np.fromfile(out / (tag + "_calls.bin"), dtype=np.uint64)[0]))
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["fused", "staged"])
def test_time_step_carries_the_tracers(run, tag):
    q = run[tag]
    assert q["calls"] == (3 if tag == "staged" else 0)
    want_vel, want_types, n_out = sc.model(q["grid"], q["pos"])
    bad = np.flatnonzero((q["vel"] != want_vel).any(axis=1))
    print(tag, "tracers", len(q["pos"]), "rows that differ", len(bad))
    assert np.array_equal(q["vel"], want_vel) and q["vel"].tobytes() == want_vel.tobytes(), (tag, bad[:8])
    assert np.array_equal(q["types"], want_types) and n_out == 0
    assert (q["pos"] != run["pos0"]).any(axis=1).all()  # every tracer has moved
    assert np.abs(q["vel"]).max() > 0.0


@pytest.mark.gpu
def test_advance_tracers_off_leaves_them_where_they_were_added(run):
    q = run["off"]
    assert np.array_equal(q["pos"], run["pos0"]) and np.array_equal(q["vel"], run["vel0"])
    assert not q["types"].any()  # no transfer has run: the type of a new tracer
    assert np.abs(q["grid"]["vel"]).max() > 0.0  # the simulation itself has stepped
