"""sources_draw_from_random of the C++ host class (libfluid_amd/host/simulation.h): time_step hands `random` to the device for the
seeding of the fluid sources (lfa_set_source_rng) and takes it back, so seed_box, steps with a source and seed_box again leave the
generator - and the particles - where the reference leaves them.

tests/host_source_rng_driver.cpp runs that sequence on a 24^3 grid, with the step in one device call and with a callback
installed (the staged step); the expected values come from tests/seed_model.py and tests/source_model.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import seed_model as sm
from tests import source_model as srcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "host_source_rng_driver.cpp")
# (the driver's scene)
SIZE, H, OFF = (24, 24, 24), 0.5, np.array([0.25, -0.5, 1.0])
BOX1 = (OFF + np.array([1.1, 0.3, 2.2]), np.array([4.7, 2.2, 3.9]), 2)
BOX2 = (OFF + np.array([7.0, 4.0, 7.0]), np.array([2.0, 1.5, 2.0]), 3)
SOURCES = [([(x, 20, z) for z in range(8, 14) for x in range(8, 14)], (0.0, -2.0, 0.0), 2, True)]
RESOLUTION = H * 2.0 ** -23  # the device keeps an fp32 in-cell fraction


def build_driver(tmp_path):
    exe = str(tmp_path / "host_source_rng_driver")
    lfa.load_library()
    cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-Wextra", *os.environ.get("LFA_HOST_CXXFLAGS", "").split(), "-o", exe,
           DRIVER_SRC, "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # warning-free
    return exe


def test_driver_builds_and_reports_a_missing_device(tmp_path, gpu_available):
    exe = build_driver(tmp_path)
    if not gpu_available:  # no CPU fallback: the driver says so and stops
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout.startswith("single no device"), r.stdout + r.stderr
        assert not list(tmp_path.glob("*.bin"))


@pytest.mark.gpu
def test_steps_with_sources_leave_random_where_the_reference_does(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    load = lambda name: np.fromfile(tmp_path / (name + ".bin"), dtype=lfa.PARTICLE_DTYPE)  # noqa: E731
    lines = re.findall(r"^(single|staged) state (\w+) (\d+) (\d+)$", r.stdout, flags=re.M)
    got = {(w, a): (int(s), int(n)) for w, a, s, n in lines}
    assert len(got) == 8, r.stdout
    # the model: box 1 from a fresh generator; the source's cells, far above the box, are empty in the first step
    pos1, s1 = sm.seed_box(SIZE, H, OFF, *BOX1[:2], density=BOX1[2])
    counts = srcm.cell_counts(SIZE, H, OFF, pos1)
    seeded, _, vel, s2 = srcm.update_sources(SIZE, H, OFF, counts, SOURCES, s1)
    assert len(seeded) == 8 * 36
    for which in ("single", "staged"):
        assert got[which, "box1"] == (s1, len(pos1)), which
        assert got[which, "step1"] == (s2, len(pos1) + len(seeded)), which
        state3, n3 = got[which, "step2"]
        assert n3 >= len(pos1) + len(seeded)
        assert state3 == sm.advance(s2, 6 * (n3 - len(pos1) - len(seeded))), which  # six draws per particle of the second step
        pos2, s4 = sm.seed_box(SIZE, H, OFF, *BOX2[:2], density=BOX2[2], state=state3)
        assert got[which, "box2"] == (s4, n3 + len(pos2)) and len(pos2) > 0, which
        box1, final = load(which + "_box1"), load(which + "_final")
        assert np.abs(box1["pos"] - pos1).max() <= RESOLUTION, which
        assert len(final) == n3 + len(pos2)
        assert np.abs(final["pos"][n3:] - pos2).max() <= RESOLUTION, which  # by id: the last seed_box's particles come last
        assert np.array_equal(final["vel"][n3:], np.broadcast_to([0.0, 1.0, 0.0], (len(pos2), 3)))
    # the staged step's callback sees the source's particles where they were seeded (they have not moved yet), by id
    at_seeding = load("staged_seeded")
    assert len(at_seeding) == len(pos1) + len(seeded)
    new = at_seeding[len(pos1):]
    assert np.abs(new["pos"] - seeded).max() <= RESOLUTION
    assert np.array_equal(new["vel"], vel) and not new["cx"].any() and not new["cy"].any() and not new["cz"].any()
    # the flag off: sources leave `random` alone
    before, after = re.search(r"^off state (\d+) (\d+)$", r.stdout, flags=re.M).groups()
    assert int(before) == int(after) == s1
