"""CPU tests of tests/tracer_cases.py: on the transfer set and on the stepped scene's inputs the oracle is the compiled reference
(tolerance 0), the counting restatement march_model is the oracle bit for bit, and the stepped scene holds the counts it promises.
This pins what tests/test_gpu_tracers.py compares the device against; the move set is pinned by tests/test_move_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import move_cases as mc
from tests import sample_cases as sc
from tests import tracer_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")


def stepped_inputs():
    pos, vel = tc.stepped_tracers()
    return sc.SIZE, sc.H, sc.OFFSET, tc.block_cells(), pos, vel, sc.DT


@needs_ref
def test_oracle_is_the_reference_on_the_transfer_set():
    pts, cells = tc.transfer_points(), sc.random_field()
    want, got = sc.model(cells, pts, "ref"), sc.model(cells, pts, "oracle")
    assert np.array_equal(got[0], want[0]) and got[0].tobytes() == want[0].tobytes()
    assert np.array_equal(got[1], want[1]) and got[2] == want[2]


@needs_ref
def test_oracle_is_the_reference_on_the_stepped_scene():
    size, h, off, solid, pos, vel, dt = stepped_inputs()
    want = tc.advect_collide(size, h, off, solid, pos, vel, dt, kind="ref")
    got = tc.advect_collide(size, h, off, solid, pos, vel, dt)
    for k in ("advect", "collide"):
        assert np.array_equal(got[k], want[k]), k
    cells = sc.random_field()
    assert np.array_equal(sc.model(cells, got["collide"])[0], sc.model(cells, got["collide"], "ref")[0])


def test_transfer_set_keeps_the_finite_outside_points():
    pts = tc.transfer_points()
    assert len(pts) == len(sc.points()) - 3 and np.isfinite(pts).all()
    assert int((~sc.classify(pts)[1]).sum()) == 7  # of the 10 outside points, three are not finite


@pytest.mark.parametrize("name", ["stepped", "obstacles", "axis_aligned", "walls_24_21_18_n511", "lone_reach"])
def test_march_model_is_the_oracle(name):
    if name == "stepped":
        size, h, off, solid, pos, vel, dt = stepped_inputs()
        want = tc.advect_collide(size, h, off, solid, pos, vel, dt)["collide"]
    else:
        size, h, off, dt, solid, pos, vel = tc.move_case(name)
        want = mc.oracle(name)["collide"]
    ends, stopped = tc.march_model(size, mc.solid_mask(size, solid), h, off, pos, vel, dt)
    assert np.array_equal(ends, want)
    if name == "obstacles":  # the counting agrees with the grid-unit restatement of move_cases where that one is exact (dyadic cases)
        assert np.array_equal(stopped, mc.model(name)[1] > 0)


def test_stepped_scene_holds_its_counts():
    pos, vel = tc.stepped_tracers()
    assert pos.shape == vel.shape == (tc.N_TRACERS, 3)
    mask = tc.solid_mask()
    c = sc.cells_of(sc.classify(pos)[0])
    assert sc.classify(pos)[1].all() and not mask[c[:, 0], c[:, 1], c[:, 2]].any()
    # every velocity points at the block: towards +x, where its near face is
    assert (vel[:, 0] >= 0.0).all()
    ever, per_step, end = tc.stepped_cpu_model()
    print("stopped per step", per_step, "ever", int(ever.sum()), "never", int((~ever).sum()))
    assert int(ever.sum()) >= 20 and int((~ever).sum()) >= 20
    assert per_step[0] >= 20
    # nobody ends inside the block
    c = sc.cells_of(sc.classify(end)[0])
    assert sc.classify(end)[1].all() and not mask[c[:, 0], c[:, 1], c[:, 2]].any()


def test_tracer_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "libfluid_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\bint\s+(lfa_\w+)\s*\(([^)]*)\)\s*;", text)}
    want = {
        "lfa_tracers_add": "lfa_sim *s, const double *xyz, const double *velocity, uint64_t n",
        "lfa_tracers_clear": "lfa_sim *s",
        "lfa_tracers_count": "const lfa_sim *s, uint64_t *n",
        "lfa_tracers_advect_collide": "lfa_sim *s, double dt",
        "lfa_tracers_transfer": "lfa_sim *s",
        "lfa_tracers_step": "lfa_sim *s, double dt, uint64_t counts[2]",
        "lfa_tracers_download": "lfa_sim *s, double *xyz, double *velocity, uint8_t *types, uint64_t n",
        "lfa_tracers_time": "lfa_sim *s, double *ms",
    }
    lib = lfa.load_library()
    for name, args in want.items():
        assert decl.get(name) == args, name
        assert hasattr(lib, name) and name in lfa.SIGNATURES, name
    vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
    assert lfa.SIGNATURES["lfa_tracers_add"] == (C.c_int, [vp, vp, vp, u64])
    assert lfa.SIGNATURES["lfa_tracers_step"] == (C.c_int, [vp, dbl, C.POINTER(u64 * 2)])
    assert lfa.SIGNATURES["lfa_tracers_download"] == (C.c_int, [vp, vp, vp, vp, u64])
    for cite in ("src/simulation.cpp:240-248", ":612-683", "include/fluid/data_structures/grid.h:140-209", ":654-681"):
        assert cite in header
    for method in ("add_tracers", "clear_tracers", "num_tracers", "tracers_advect_collide", "tracers_transfer", "tracers_step",
                   "tracers", "tracers_ms"):
        assert callable(getattr(lfa.Sim, method))
    assert "tracers.hip" in open(os.path.join(ROOT, "libfluid_amd", "build.py")).read()


def _have_hipcc():
    import shutil
    return any(c and (shutil.which(c) or os.path.exists(c)) for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"))


@pytest.mark.skipif(not _have_hipcc(), reason="no hipcc on this machine")
def test_tracer_kernels_use_no_scratch_and_spill_nothing():
    """The compiler's own metadata (tools/kernel_resources.py compiles tracers.hip for gfx950; nothing runs on a device). The VGPR
    bound is the one of 5 waves per SIMD (512 / 5 in granules of 8: 96), as for k_sample_velocity."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "tracers.hip", "k_tracer_"],
                         capture_output=True, text=True, check=True).stdout
    print(out)
    seen = set()
    for m in re.finditer(r"(k_tracer_\w+)\(.*vgpr\s+(\d+) sgpr\s+(\d+) spill\s+(\d+) lds\s+(\d+) scratch\s+(\d+)", out):
        vgpr, sgpr, spill, lds, scratch = (int(x) for x in m.groups()[1:])
        assert vgpr <= 96 and spill == 0 and scratch == 0 and lds == 0, m.group(0)
        seen.add(m.group(1))
    assert {"k_tracer_step", "k_tracer_advect_collide", "k_tracer_transfer"} <= seen
