"""seed_on_device of the C++ host class (libfluid_amd/host/simulation.h): seed_box / seed_sphere through lfa_seed_box /
lfa_seed_sphere against the host loop of the same class (which tests/test_ref_callers.py holds to the reference's particles).

tests/host_seed_driver.cpp seeds one scene twice - a sphere, then a box, on a 24^3 grid - once per path."""
import os
import re
import subprocess

import numpy as np
import pytest

import libfluid_amd as lfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "host_seed_driver.cpp")
CELL_SIZE = 0.5  # (the driver's)


def build_driver(tmp_path, *defs):
    exe = str(tmp_path / "host_seed_driver")
    lfa.load_library()
    cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-Wall", "-Wextra", *defs, *os.environ.get("LFA_HOST_CXXFLAGS", "").split(), "-o", exe,
           DRIVER_SRC, "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_host_seed_driver_compiles_and_links(tmp_path):
    build_driver(tmp_path)
    build_driver(tmp_path, "-DLFA_SEED_DRAW_ORDER_LTR")


def test_host_generator_jump_ahead(tmp_path):
    """fluid_amd::pcg32::advance(k) against k draws; state() / set_state() round-trip (host code only)."""
    src = tmp_path / "jump.cpp"
    src.write_text("""
#include <cstdio>
#include "%s"
int main() {
    const unsigned long long ks[] = {0, 1, 5, 6, 1000003ull};
    for (unsigned long long k : ks) {
        fluid_amd::pcg32 a, b;
        for (unsigned long long i = 0; i < k; ++i) a();
        b.advance(k);
        if (a.state() != b.state() || a() != b()) { std::printf("advance(%%llu) differs\\n", k); return 1; }
    }
    fluid_amd::pcg32 a, b, c;
    a.advance((1ull << 32) + 7);
    b.advance(1ull << 32); b.advance(4); b(); b(); b();
    c.set_state(b.state());
    if (a.state() != b.state() || a() != c()) { std::printf("composed jump differs\\n"); return 1; }
    std::printf("%%llu\\n", (unsigned long long)fluid_amd::pcg32().state());
    return 0;
}
""" % os.path.join(ROOT, "libfluid_amd", "host", "simulation.h"))
    exe = str(tmp_path / "jump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    from tests import seed_model as sm
    assert int(r.stdout.split()[-1]) == sm.initial_state()  # the model starts where a fresh simulation's generator does


@pytest.mark.gpu
def test_device_seeding_matches_the_host_loop(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    load = lambda name: np.fromfile(tmp_path / (name + ".bin"), dtype=lfa.PARTICLE_DTYPE)  # noqa: E731
    for which in ("first", "second"):
        host, dev = load(which + "_host"), load(which + "_device")
        assert len(host) == len(dev) > 0, which
        # the device keeps an fp32 in-cell fraction: cell_size 2^-23 is its documented resolution
        assert np.abs(dev["pos"] - host["pos"]).max() <= CELL_SIZE * 2.0 ** -23, which
        assert np.abs(dev["old_pos"] - host["pos"]).max() <= CELL_SIZE * 2.0 ** -23, which
        assert np.array_equal(dev["vel"], host["vel"]), which
        for c in ("cx", "cy", "cz"):
            assert not dev[c].any() and not host[c].any()
    # the second set holds the second seed_box alone: a sphere and a floor-wide box before, one small box of 27 per cell now
    assert len(load("second_host")) < len(load("first_host"))
    assert np.array_equal(np.unique(load("second_device")["vel"], axis=0), [[0.0, 1.0, 0.0]])
    draws = dict(re.findall(r"^(host|device) draws (.*)$", r.stdout, flags=re.M))
    assert set(draws) == {"host", "device"} and draws["host"] == draws["device"], r.stdout
    upd = {w: (int(s), int(a), int(b)) for w, s, a, b in re.findall(r"^(host|device) update (-?\d+) (\d+) (\d+)$", r.stdout, flags=re.M)}
    assert set(upd) == {"host", "device"}, r.stdout
    for w, (status, before, after) in upd.items():
        assert status == 0 and before == after == len(load("second_host")), (w, r.stdout)
