"""frame_stats() / positions() of the C++ host class (libfluid_amd/host/simulation.h) against the testbed's own loops over
particles() (tests/host_frame_driver.cpp: scene 3 at 24^3, three time_step()s, then an edit through particles()).

The bars are those of tests/test_gpu_frame.py: the occupation grid, the counts, the maximum, the box and the positions exactly;
the energy within frame_model.energy_bound of the model's - and of the testbed loop's, which adds the same terms in another order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import frame_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "host_frame_driver.cpp")
SIZE, OFFSET, H, GRAVITY = (24, 24, 24), (0.0, 0.0, 0.0), 1.0, (0.0, -981.0, 0.0)  # (the driver's)


def build_driver(tmp_path):
    exe = str(tmp_path / "host_frame_driver")
    lfa.load_library()
    cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-Wextra", *os.environ.get("LFA_HOST_CXXFLAGS", "").split(), "-o", exe,
           DRIVER_SRC, "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    return exe


def test_host_frame_driver_compiles_and_links(tmp_path):
    build_driver(tmp_path)


def load(tmp_path, tag):
    st = lfa.FrameStats.from_buffer_copy((tmp_path / (tag + "_stats.bin")).read_bytes())
    assert (tmp_path / (tag + "_stats.bin")).stat().st_size == C.sizeof(lfa.FrameStats)
    host = np.fromfile(tmp_path / (tag + "_host.bin"), dtype=np.uint64)
    return dict(st=st, occ=np.fromfile(tmp_path / (tag + "_occupation.bin"), dtype=np.uint64),
                pos=np.fromfile(tmp_path / (tag + "_positions.bin"), dtype=np.float64).reshape(-1, 3),
                parts=np.fromfile(tmp_path / (tag + "_particles.bin"), dtype=lfa.PARTICLE_DTYPE),
                host_energy=float(host[:1].view(np.float64)[0]), host_max=float(host[1:2].view(np.float64)[0]), host_occ=host[2:])


@pytest.mark.gpu
def test_summary_equals_the_testbed_loops(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = {tag: load(tmp_path, tag) for tag in ("step1", "step2", "step3", "edit")}
    for tag, q in rec.items():
        st, parts = q["st"], q["parts"]
        m = fm.summary(parts, SIZE, OFFSET, H, GRAVITY)
        bound = fm.energy_bound(len(parts), m["energy_abs"])
        print(tag, "n", st.n, "energy", st.energy, "model", m["energy"], "testbed loop", q["host_energy"], "bound", bound)
        assert st.n == len(parts) > 0 and st.n_in_grid == m["n_in_grid"] == int(q["host_occ"].sum())
        assert np.array_equal(q["occ"], q["host_occ"]) and np.array_equal(q["occ"], m["occupation"].reshape(-1)), tag
        assert st.max_speed2 == q["host_max"] == m["max_speed2"], tag
        assert np.array_equal(np.array(st.lo), m["lo"]) and np.array_equal(np.array(st.hi), m["hi"]), tag
        assert q["pos"].tobytes() == np.ascontiguousarray(parts["pos"]).tobytes(), tag
        assert abs(st.energy - m["energy"]) <= bound and abs(st.energy_abs - m["energy_abs"]) <= bound, tag
        assert abs(st.energy - q["host_energy"]) <= bound, tag
    assert rec["step3"]["st"].max_speed2 > 0.0
    # the edit: particle 0 left its cell for (20, 21, 22); nothing else moved
    old = fm.cells(rec["step3"]["parts"]["pos"][:1], OFFSET, H)[0]
    delta = rec["edit"]["occ"].astype(np.int64) - rec["step3"]["occ"].astype(np.int64)
    want = np.zeros(SIZE[::-1], dtype=np.int64)
    want[old[2], old[1], old[0]] -= 1
    want[22, 21, 20] += 1
    assert np.array_equal(delta.reshape(SIZE[::-1]), want)
    assert np.array_equal(rec["edit"]["pos"][0], [20.5, 21.5, 22.5]) and np.array_equal(rec["edit"]["pos"][1:], rec["step3"]["pos"][1:])
