"""Device seeding (lfa_seed_box / lfa_seed_sphere), the parts that need no GPU.

tests/seed_model.py restates the reference's seeding without its sequential loop; here it is pinned to what the g++-built
reference actually seeded (tests/golden/ref_callers.npz), its jump-ahead is checked against single steps, and the C ABI is checked
to be declared, exported and bound. tests/test_gpu_seed.py compares the device with the model."""
import os
import re

import numpy as np

import libfluid_amd as lfa
from tests import seed_model as sm
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sorted_rows(a):
    a = a.reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def test_model_seeds_what_the_reference_seeded():
    """The two testbed box scenes (tests/callers/reference_callers.cpp: a 20^3 grid, cell size 1, the testbed's coordinates scaled
    by 20 / 50): frame0.pos is the particle list right after seed_box, from a freshly constructed generator."""
    g = util.load_golden("ref_callers")
    s = 20.0 / 50.0
    scenes = {"testbed_scene0": (np.array([15.0, 15.0, 15.0]) * s, np.array([20.0, 20.0, 20.0]) * s),
              "testbed_scene3": (np.zeros(3), np.array([10.0, 50.0, 50.0]) * s)}
    for name, (start, size) in scenes.items():
        pos, _ = sm.seed_box((20, 20, 20), 1.0, (0.0, 0.0, 0.0), start, size)
        want = g[name + "/frame0.pos"]
        assert len(pos) * 3 == len(want), name
        assert np.array_equal(sorted_rows(pos), sorted_rows(want)), name


def test_jump_ahead_equals_single_steps():
    s0 = sm.initial_state()
    for k in (0, 1, 5, 6):
        s = s0
        for _ in range(k):
            s = sm.step(s)
        assert sm.advance(s0, k) == s, k
    # 2^32 + 7 steps, composed of two jumps (single steps from there on)
    big = (1 << 32) + 7
    s = sm.advance(sm.advance(s0, 1 << 32), 4)
    for _ in range(3):
        s = sm.step(s)
    assert sm.advance(s0, big) == s
    assert sm.advance(sm.advance(s0, 12345), big - 12345) == sm.advance(s0, big)
    # the vectorised form the model seeds with
    ks = np.array([0, 1, 5, 6, big, 6 * 307199], dtype=np.uint64)
    assert [int(v) for v in sm._advance_each(s0, ks)] == [sm.advance(s0, int(k)) for k in ks]


def test_model_draws_every_candidate():
    """The state after a call is the state before advanced by 6 x candidates, whatever the predicate accepted; an empty range
    draws nothing."""
    s0 = sm.initial_state()
    # cells 2..6 per axis (e - s + 1 = 5), density 3
    pos, s1 = sm.seed_box((8, 8, 8), 0.5, (0.0, 0.0, 0.0), (1.2, 1.2, 1.2), (2.0, 2.0, 2.0), density=3, state=s0)
    assert s1 == sm.advance(s0, 6 * 5 ** 3 * 27) and 0 < len(pos) < 5 ** 3 * 27
    pos, s2 = sm.seed_box((8, 8, 8), 0.5, (0.0, 0.0, 0.0), (9.0, 0.0, 0.0), (1.0, 1.0, 1.0), state=s0)
    assert len(pos) == 0 and s2 == s0


def test_seed_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = lfa.load_library()
    for name in ("lfa_seed_box", "lfa_seed_sphere"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/libfluid_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in lfa.SIGNATURES
    assert re.search(r"LFA_SEED_DRAW_LTR\s*=\s*1", text) and lfa.SEED_DRAW_LTR == 1
    assert "simulation.cpp:153-181" in header
    assert callable(lfa.Sim.seed_box) and callable(lfa.Sim.seed_sphere)
