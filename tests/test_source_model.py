"""Fluid sources that draw from the simulation's pcg32 (lfa_update_sources_rng / lfa_set_source_rng), the parts that need no GPU.

tests/source_model.py restates simulation::_update_sources / seed_cell; here it is pinned to the compiled reference (where
oracle/_ref is built) and to the particles it recorded (tests/golden/source_seeding.npz, written by
tests/golden/make_golden_sources.py) in every scene of tests/source_cases.py, its generator bookkeeping is checked, and the C ABI
is checked to be declared, exported and bound. tests/test_gpu_source_rng.py compares the device with the model."""
import os
import re

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import seed_model as sm
from tests import source_cases as sc
from tests import source_model as srcm
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_rows(name):
    grid, _, _, _ = sc.case(name)
    pos, cells, vel, _ = sc.expected(name)
    return sc.sorted_rows(pos, sc.raw_index(grid, cells), vel)


def assert_same_seeds(got, want, what):
    for g, w, field in zip(got, want, ("position", "raw_cell_index", "velocity")):
        assert g.shape == w.shape, (what, field, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, field)  # bit for bit


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this box)")
@pytest.mark.parametrize("name", sc.RTL)
def test_model_equals_the_compiled_reference(name):
    """A fresh reference simulation (generator in its default state), the case's resident particles, hash, the sources,
    _update_sources: its new records are the model's. (The pin also settles the order of seed_cell's three draws: z first.)"""
    from tests.golden.make_golden_sources import reference_seeds
    assert_same_seeds(model_rows(name), reference_seeds(name), name)


@pytest.mark.parametrize("name", sc.RTL)
def test_model_equals_the_recorded_reference(name):
    g = util.load_golden("source_seeding")
    want = tuple(g[f"{name}_{k}"] for k in ("pos", "raw", "vel"))
    assert len(want[0]) > 0
    assert_same_seeds(model_rows(name), want, name)


def test_cases_do_what_they_are_there_for():
    n = {name: len(sc.expected(name)[0]) for name in sc.ALL}
    assert n["A"] == 512 and n["E_root16"] == 4096 and n["E_root1"] == 300
    # B: every need from 0 to 8 occurs, and full cells sit in the middle of both sources
    grid, parts, sources, _ = sc.case("B")
    counts = srcm.cell_counts(grid["size"], 1.0, grid["offset"], parts["pos"])
    for cells, _, _, _ in sources:
        c = np.asarray(cells)
        assert len(c) == 400
        have = counts[c[:, 0] + 24 * (c[:, 1] + 16 * c[:, 2])]
        assert set(np.unique(have)) == set(range(9))
        full = np.flatnonzero(have == 8)
        assert np.diff(full).tolist().count(1) >= 60 and 0 < full.min() and full.max() < 399
    # C: 8 + 19 in (3,3,3); 27 + 19 in (5,5,5); 8 in (8,8,8); 19 in (2,2,2) on top of its 12; 5 in (9,9,9); nothing inactive
    pos, cells, vel, _ = sc.expected("C")
    per = {tuple(c): int((cells == c).all(axis=1).sum()) for c in np.unique(cells, axis=0)}
    assert per == {(3, 3, 3): 27, (5, 5, 5): 46, (8, 8, 8): 8, (2, 2, 2): 19, (9, 9, 9): 5}
    assert not (vel == 9.0).any()
    # F: the other draw order gives other particles, with the same state afterwards
    a, b = sc.expected("D_h05"), sc.expected("F_ltr_h05")
    assert a[0].tobytes() != b[0].tobytes() and a[3] == b[3]


def test_state_advances_by_six_draws_per_particle():
    s0 = 0x0123456789ABCDEF
    for name in sc.ALL:
        pos, _, _, s1 = sc.expected(name, s0)
        assert s1 == sm.advance(s0, 6 * len(pos)), name
    # a call that creates nothing leaves the state alone: full cells, an inactive source, no source at all
    full = np.full(16 ** 3, 8)
    src = [(((1, 2, 3), (4, 5, 6)), (0.0, 0.0, 0.0), 2, True), (((7, 7, 7),), (0.0, 0.0, 0.0), 3, False)]
    pos, _, _, s1 = srcm.update_sources((16, 16, 16), 1.0, (0.0, 0.0, 0.0), full, src, s0)
    assert len(pos) == 0 and s1 == s0
    assert srcm.update_sources((16, 16, 16), 1.0, (0.0, 0.0, 0.0), full, [], s0)[3] == s0
    # the particles of a call are one draw sequence: splitting the source list in two calls gives the same particles
    grid, parts, sources, _ = sc.case("C")
    counts = srcm.cell_counts(grid["size"], 1.0, grid["offset"], parts["pos"])
    whole = srcm.update_sources(grid["size"], 1.0, grid["offset"], counts, sources[:2], s0)
    first = srcm.update_sources(grid["size"], 1.0, grid["offset"], counts, sources[:1], s0)
    counts2 = counts.copy()
    counts2[3 + 16 * (3 + 16 * 3)] = counts2[9 + 16 * (9 + 16 * 9)] = 8
    second = srcm.update_sources(grid["size"], 1.0, grid["offset"], counts2, sources[1:2], first[3])
    assert np.concatenate([first[0], second[0]]).tobytes() == whole[0].tobytes() and second[3] == whole[3]


def test_source_rng_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = lfa.load_library()
    for name in ("lfa_update_sources_rng", "lfa_set_source_rng", "lfa_get_source_rng"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/libfluid_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in lfa.SIGNATURES
        # the comment in front of the declaration names the entry point and cites the reference lines it replaces
        comment = re.findall(r"/\*(.*?)\*/", header[:header.index("int " + name + "(")], flags=re.S)[-1]
        assert "simulation.cpp:756-765" in comment and ":136-151" in comment, name
    for name in ("update_sources_rng", "set_source_rng", "get_source_rng"):
        assert callable(getattr(lfa.Sim, name, None)), name
    host = open(os.path.join(ROOT, "libfluid_amd", "host", "simulation.h")).read()
    assert re.search(r"\bbool\s+sources_draw_from_random\s*=\s*false\s*;", host)
