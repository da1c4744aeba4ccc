"""Frame summary (lfa_frame_stats / lfa_download_positions), the parts that need no GPU.

tests/frame_model.py restates the loops the reference's hosts run over simulation::particles(); here it is pinned to what the
compiled reference published for frame 0 of the two testbed box scenes (tests/golden/ref_callers.npz: particles that
tests/seed_model.py reproduces bit for bit, at rest), and the C ABI is checked to be declared, exported and bound.
tests/test_gpu_frame.py compares the device with the model."""
import os
import re

import numpy as np

import libfluid_amd as lfa
from tests import frame_model as fm
from tests import seed_model as sm
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAVITY = (0.0, -981.0, 0.0)  # tests/callers/reference_callers.cpp: testbed


def test_model_computes_what_the_reference_published():
    g = util.load_golden("ref_callers")
    s = 20.0 / 50.0
    scenes = {"testbed_scene0": (np.array([15.0, 15.0, 15.0]) * s, np.array([20.0, 20.0, 20.0]) * s),
              "testbed_scene3": (np.zeros(3), np.array([10.0, 50.0, 50.0]) * s)}
    for name, (start, size) in scenes.items():
        pos, _ = sm.seed_box((20, 20, 20), 1.0, (0.0, 0.0, 0.0), start, size)
        got = fm.summary(sm.records(pos), (20, 20, 20), (0.0, 0.0, 0.0), 1.0, GRAVITY)
        want_occ = g[name + "/frame0.occupation"]
        assert np.array_equal(got["occupation"].reshape(-1).astype(np.float64), want_occ), name
        assert got["n"] == got["n_in_grid"] == len(pos) == int(want_occ.sum()), name
        want = float(g[name + "/frame0.energy"][0])
        # the reference adds 0.5 |v|^2 and subtracts g . x one after the other, in list order: another order of the same terms
        bound = fm.energy_bound(len(pos), got["energy_abs"])
        print(name, "energy", got["energy"], "reference", want, "difference", abs(got["energy"] - want), "bound", bound)
        assert abs(got["energy"] - want) <= bound, name
        assert got["max_speed2"] == 0.0


def test_the_round_trip_through_the_key_changes_cells():
    """off + c h, divided by h again: for off = 0.7, h = 0.3 the cells 2, 7, 8, 9 and 13 of the first 24 come back one lower. The
    occupation grid is the hosts' loop over reconstructed positions, so it sees that; a count by key would not."""
    off, h = np.float64(0.7), np.float64(0.3)
    c = np.arange(24)
    x = off + (c.astype(np.float64) + 0.0) * h
    pos = np.stack([x, x, x], axis=1)
    back = fm.cells(pos, (off, off, off), h)[:, 0]
    assert np.flatnonzero(back != c).tolist() == [2, 7, 8, 9, 13]
    assert (back[back != c] == c[back != c] - 1).all()
    occ, n_in = fm.occupation(pos, (24, 24, 24), (off, off, off), h)
    assert n_in == 24 and occ[1, 1, 1] == 2 and occ[2, 2, 2] == 0


def test_model_edge_cases():
    parts = np.zeros(3, dtype=lfa.PARTICLE_DTYPE)
    parts["pos"] = [[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [4.0, 0.5, 0.5]]  # -0.5 truncates to cell 0; 4.0 is outside a 4-cell grid
    parts["vel"] = [[1.0, 2.0, 2.0], [np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]]
    got = fm.summary(parts, (4, 4, 4), (0.0, 0.0, 0.0), 1.0, (0.0, 0.0, 0.0))
    assert got["n"] == 3 and got["n_in_grid"] == 2 and got["occupation"][0, 0, 0] == 2
    assert got["max_speed2"] == 9.0  # the NaN is skipped, as std::max(fastest, nan) skips it
    empty = fm.summary(parts[:0], (4, 4, 4), (0.0, 0.0, 0.0), 1.0, GRAVITY)
    assert empty["n"] == 0 and empty["energy"] == 0.0 and empty["max_speed2"] == 0.0 and not empty["occupation"].any()
    assert np.isposinf(empty["lo"]).all() and np.isneginf(empty["hi"]).all()


def test_frame_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = lfa.load_library()
    for name in ("lfa_frame_stats", "lfa_download_positions", "lfa_frame_stats_time"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/libfluid_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in lfa.SIGNATURES
    assert re.search(r"struct\s+lfa_frame_stats\s*\{", text)
    assert "testbed/main.cpp:50-88" in header and "grid_node.cpp:356-364" in header
    fields = [f for f, _ in lfa.FrameStats._fields_]
    assert fields == ["n", "n_in_grid", "energy", "energy_abs", "max_speed2", "lo", "hi"]
    at = [re.search(r"\b" + f + r"\b", text[text.index("struct lfa_frame_stats"):]).start() for f in fields]
    assert at == sorted(at)  # the binding's field order is the header's
    import ctypes as C
    assert C.sizeof(lfa.FrameStats) == 2 * 8 + 3 * 8 + 6 * 8
    assert callable(lfa.Sim.frame_stats) and callable(lfa.Sim.positions)
    assert "frame.hip" in open(os.path.join(ROOT, "libfluid_amd", "build.py")).read()
