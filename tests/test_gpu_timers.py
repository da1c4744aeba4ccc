"""What lfa_get_step_timings and lfa_get_timings report, entry by entry (include/libfluid_amd.h; the names are STEP_TIMER_NAMES and
TIMER_NAMES of the binding). Every assertion follows from how the drivers fill the arrays: the entries are spans between HIP events
on the handle's streams, except an iteration count, a mean (the same double division the driver does, so compared with ==) and a
flag. Grid 16 x 16 x 16 = 2 x 2 x 2 tiles: the smallest with a tile neighbour in every direction and two tile layers."""
import math

import pytest

import libfluid_amd as lfa
from libfluid_amd import scenes

pytestmark = pytest.mark.gpu

SIZE, DT = (16, 16, 16), 0.01
# 12 x 8 x 12 cells, 9216 particles each. `air`: the block hangs in the air and falls freely - gravity alone leaves the velocity
# divergence-free, the right-hand side is zero and every solve ends with 0 iterations. `floor`: the same block on the grid's
# floor, where the wall stops the fall: the solve iterates, and the iteration mean is a quotient of two non-zero numbers.
BLOCKS = {"air": ((2, 2, 2), (14, 10, 14)), "floor": ((2, 0, 2), (14, 8, 14))}
_PARTS = {}


def block(name="air"):
    """Built once per name, never written."""
    if name not in _PARTS:
        _PARTS[name] = scenes.seed_block(*BLOCKS[name])
        _PARTS[name].setflags(write=False)
    return _PARTS[name]


# the entries of the step timers that are no times, and the stages that follow one another on one stream when nothing overlaps
NOT_A_TIME = ("pcg_iterations", "pcg_iteration_mean", "overlapped")
SERIAL_STAGES = ("advect_collide", "bin", "p2g", "build_system", "pcg_loop", "apply_pressure", "correct_collide", "extrapolate", "g2p")


def check_times(t, names):
    assert list(t) == names
    for k, v in t.items():
        assert math.isfinite(v) and v >= 0.0, (k, v)


@pytest.mark.parametrize("case", ["apic_overlap", "apic_serial", "slab_overlap", "no_particles", "floor_overlap", "floor_serial"])
def test_step_timings(case):
    sim = lfa.Sim(SIZE, method=lfa.APIC)
    hub = None
    if case == "slab_overlap":
        hub = lfa.LocalHub(1)
        sim.init_local_slab(hub.h, 0, [0, 2])
    seeded = case != "no_particles"
    if seeded:
        sim.upload_particles(block("floor" if case.startswith("floor") else "air"))
    overlap_on = not case.endswith("serial")
    sim.set_step_overlap(overlap_on)
    sim.enable_timing(True)
    for step in range(2):
        _, it, rc = sim.time_step(DT)
        assert rc >= 0
        t = sim.step_timings()
        print(case, step, it, t)
        check_times(t, lfa.STEP_TIMER_NAMES)
        assert t["pcg_iterations"] == it
        assert (it > 0) == case.startswith("floor")  # (what the two blocks are there for)
        assert t["pcg_iteration_mean"] == (t["pcg_loop"] / it if it else 0.0)
        # a handle without particles has nothing to run beside the solve: it reports 0 whatever was asked for
        assert t["overlapped"] == (1.0 if overlap_on and seeded else 0.0)
        spans = [k for k in lfa.STEP_TIMER_NAMES if k not in NOT_A_TIME and k != "time_step"]
        if seeded:
            # nested spans, at least one whole kernel shorter than the span around them
            assert t["p2g_scatter_kernel"] < t["p2g"]
            assert t["correct_cell_index"] + t["correct_tiled_kernel"] < t["correct_collide"]
            for k in spans:
                assert t[k] < t["time_step"], k
        else:
            assert t["correct_cell_index"] == 0.0 and t["correct_tiled_kernel"] == 0.0
            assert t["pcg_loop"] == 0.0 and t["pcg_iterations"] == 0.0
            # no kernel lies between the events here: the nesting holds without a margin (events of one stream are ordered)
            assert t["p2g_scatter_kernel"] <= t["p2g"]
            assert t["correct_cell_index"] + t["correct_tiled_kernel"] <= t["correct_collide"]
            for k in spans:
                assert t[k] <= t["time_step"], k
        if not overlap_on:
            # consecutive intervals on one stream; ten float32 roundings of hipEventElapsedTime stay below 1e-6 relative
            assert sum(t[k] for k in SERIAL_STAGES) <= t["time_step"] * (1 + 1e-5)
    sim.close()
    if hub is not None:
        hub.close()


@pytest.mark.parametrize("where", ["air", "floor"])
@pytest.mark.parametrize("precond", [lfa.PRECOND_MULTIGRID, lfa.PRECOND_MIC0_EXACT])
def test_hot_step_timings(precond, where):
    sim = lfa.Sim(SIZE, method=lfa.APIC, precond=precond)
    sim.upload_particles(block(where))
    sim.enable_timing(True)
    _, it, rc = sim.step_hot(DT)
    assert rc >= 0
    t = sim.timings()
    print(precond, where, it, t)
    check_times(t, lfa.TIMER_NAMES)
    assert (it > 0) == (where == "floor")
    assert t["pcg_iteration_mean"] == (t["pcg_loop"] / it if it else 0.0)
    assert t["p2g_scatter_kernel"] < t["p2g"]
    sim.close()
