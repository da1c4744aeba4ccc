"""GPU tests (-m gpu) of the multigrid V-cycle (libfluid_amd/csrc/mg.hip) against tests/vcycle_model.py, the cycle in numpy and
fp64, on the fields and right-hand sides of tests/vcycle_cases.py: z = M^-1 r from lfa_apply_preconditioner is held against the
model's z for every right-hand side, in every launch layout, after set-ups in sequence on one handle, and - through the solve's
iteration count - in the kernels fused with the PCG's AXPYs.

The level-0 inputs are the oracle's; every test first asserts that the device's are identical (unknowns, A bytes, counts, active
tiles per level). Bars, in max norm: fp64 1e-10 max |z_model|; fp32 8 d32 with d32 = max |V_float32(r) - V_float64(r)| from the
model alone, per field and right-hand side, and never below half an fp32 ulp of the largest entry of z - the rounding of the
result's storage (vcycle_cases.reference says why); closed tiles against the bar of their own solve
(vcycle_cases.closed_bars). No field, right-hand side or unknown is left out: the unknowns of closed tiles and the others are
checked separately, and both are checked. tests/test_vcycle_model.py shows that each of the model's ten one-rule mutants
misses these bars by a factor of 100 at least.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts, every solve `ITERS ...` (pytest -s shows them;
docs/experiments.md records them).
"""
import numpy as np
import pytest

import libfluid_amd as lfa
from tests import stencil_cases as sc
from tests import vcycle_cases as vc
from tests import vcycle_model as vm
from tests.test_gpu_parity import cells_from
from tests.test_gpu_stencil_edges import DTYPE_ID, DTYPES, margin, pointwise

pytestmark = pytest.mark.gpu

MG = lfa.PRECOND_MULTIGRID
KNOBS = ("LFA_MG_NO_PERSIST", "LFA_MG_NO_TAGGED", "LFA_MG_NO_TOP", "LFA_MG_NO_CLOSED", "LFA_MG_NO_PRUNE")
LAYOUTS = {"tagged": None, "tagged-no-top": "LFA_MG_NO_TOP", "flags": "LFA_MG_NO_TAGGED", "phase": "LFA_MG_NO_PERSIST"}


def new_sim(name, dtype, **extra):
    size, parts, solid, meta = vc.build(name)
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], density=meta["rho"], method=lfa.APIC, blending=1.0, precond=MG,
                pcg_dtype=dtype, **extra)
    if solid is not None:
        s.set_solid_cells(solid)
    return s


def set_up(s, name, solids=False):
    """The field's particles binned, the oracle's grid after gravity uploaded, the system built (`plate`: the device's own P2G - its
    particles are at rest). `solids`: the field's solid mask replaces the handle's first."""
    size, parts, solid, meta = vc.build(name)
    w = vc.system(name)
    if solids:
        s.clear_solid_cells()
        s.set_solid_cells(solid)
    s.upload_particles(parts)
    s.hash()
    if name == "plate":
        s.p2g()
    else:
        s.upload_cells(cells_from(w["vel"], w["type"]))
    s.build_system(vc.DT)
    return w


def strip(tiles):
    tiles = [int(t) for t in tiles]
    while tiles and tiles[-1] == 0:
        tiles.pop()
    return tiles


def inputs_identical(s, name, what, closed=True, prune=True):
    w, H = vc.system(name), vc.model(name, closed, prune)
    assert np.array_equal(s.fluid_cells(), w["fluid_cells"]), f"{what}: unknowns differ"
    assert np.array_equal(s.abits(), w["abits"]), f"{what}: A bytes differ"
    assert np.array_equal(s.cell_counts() > 0, w["counts"] > 0), f"{what}: cells that hold particles differ"
    if name not in vc.SEQUENCE_FIELDS:
        assert np.array_equal(s.cell_counts(), w["counts"]), f"{what}: counts differ"
    assert strip(s.mg_level_tiles()) == strip(H.tiles), f"{what}: active tiles per level {s.mg_level_tiles()}, model {H.tiles}"
    assert s.solver_stats()["device_waits_given_up"] == 0


def held(z, r, name, label, dtype, what, closed=True, prune=True):
    """z against the model's: the V-cycle's unknowns in max norm at the bar of the field and right-hand side, the closed tiles'
    unknown by unknown at the bar of their tile's solve."""
    f64 = dtype == lfa.PCG_F64
    H = vc.model(name, closed, prune)
    zm, _ = vc.reference(name, label, closed, prune)
    op = vm.open_mask(H)
    bar = vc.bar(name, label, f64, closed, prune)
    err = float(np.abs(z - zm)[op].max()) if op.any() else 0.0
    margin(what, err, bar)
    assert err <= bar, f"{what}: max |z - z_model| = {err:.3e}, bar {bar:.3e}, max |z_model| = {np.abs(zm).max():.3e}"
    if (~op).any():
        pointwise(z[~op], closed_solves(H, r, f64)[~op], vc.closed_bars(H, np.asarray(r), f64)[~op], f"{what} closed_tiles")


def closed_solves(H, r, f64):
    """The exact solves of the closed tiles' blocks for the right-hand side the device holds: r, rounded to fp32 where its vectors
    are fp32 (the rounding of an input is part of no error). 0 outside the closed tiles."""
    r = np.asarray(r, dtype=np.float64) if f64 else sc.f32(r)
    out = np.zeros(len(r))
    for idx, A in H.closed_blocks:
        out[idx] = np.linalg.solve(A, r[idx]) / H.a_scale
    return out


def all_held(s, name, dtype, what, labels=None, closed=True, prune=True):
    out = {}
    for label, r in vc.rhs(name).items():
        if labels is not None and label not in labels:
            continue
        out[label] = s.apply_precon(r)
        held(out[label], r, name, label, dtype, f"{what} {label}", closed, prune)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", vc.FIELDS)
def test_vcycle_is_the_model(name, dtype):
    s = new_sim(name, dtype)
    set_up(s, name)
    what = f"{name} {DTYPE_ID[dtype]}"
    inputs_identical(s, name, what)
    all_held(s, name, dtype, what)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", ["terraces", "droplets"])
def test_every_layout_is_the_model(name, dtype, monkeypatch):
    """tagged / tagged without the fused top level / flags / a launch per phase: each is the model, and all four are bit-identical
    on fields with pruned and closed tiles. LFA_MG_NO_PRUNE=1 is bit-identical to the default (a pruned tile only ever computed
    zeros); LFA_MG_NO_CLOSED=1 is the model that is told that no tile is closed."""
    what = f"{name} {DTYPE_ID[dtype]}"
    main = ("random", "b", "A_smooth", "A_coarse", "impulse_closed", "impulse_pruned_child", "impulse_pillar_aligned",
            "impulse_pillar_unaligned")
    got = {}
    for mode, knob in list(LAYOUTS.items()) + [("no-prune", "LFA_MG_NO_PRUNE"), ("no-closed", "LFA_MG_NO_CLOSED")]:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if knob:
            monkeypatch.setenv(knob, "1")
        s = new_sim(name, dtype)
        set_up(s, name)
        inputs_identical(s, name, f"{what} {mode}", closed=mode != "no-closed", prune=mode != "no-prune")
        if mode == "no-closed":
            got[mode] = all_held(s, name, dtype, f"{what} {mode}", labels=main, closed=False)
        else:
            got[mode] = all_held(s, name, dtype, f"{what} {mode}", labels=None if mode in LAYOUTS else main, prune=mode != "no-prune")
        s.close()
    for mode in ("tagged-no-top", "flags", "phase", "no-prune"):
        for label, z in got[mode].items():
            assert np.array_equal(z, got["tagged"][label]), f"{what} {mode} {label}: not bit-identical to the default layout"


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", ["droplets", "terraces"])
def test_closed_tiles_get_their_exact_inverse(name, dtype):
    """r supported on the closed tiles: z there is the solve of each tile's block, z elsewhere is the model's for r = 0 - exactly 0."""
    f64 = dtype == lfa.PCG_F64
    s = new_sim(name, dtype)
    set_up(s, name)
    what = f"{name} {DTYPE_ID[dtype]} closed_only"
    inputs_identical(s, name, what)
    H = vc.model(name)
    op = vm.open_mask(H)
    assert len(H.closed) >= 3
    r = np.where(op, 0.0, np.random.default_rng(5).normal(size=len(op)))
    z = s.apply_precon(r)
    s.close()
    want = closed_solves(H, r, f64)
    model = vm.vcycle(H, r)
    assert not model[op].any() and np.abs(model - closed_solves(H, r, True)).max() <= 1e-14 * np.abs(model).max()
    pointwise(z[~op], want[~op], vc.closed_bars(H, r, f64)[~op], what)
    assert not z[op].any(), f"{what}: {int(np.count_nonzero(z[op]))} unknowns outside the closed tiles are not exactly 0"


SEQUENCES = {
    # field, what happens before the step's set-up
    "come_and_go": [("A", None), ("B", None), ("A", "dtype"), ("S", "solids"), ("A", "dtype")],
    "terraces": [("terraces", None), ("terraces_shifted", None), ("terraces_half", "dtype"), ("terraces_half_solid", "solids"),
                 ("terraces", "solids+dtype")],
}


@pytest.mark.parametrize("solve", [False, True], ids=["no_solve", "solve_between"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_set_ups_in_sequence_leave_nothing_behind(seq, dtype, solve):
    """One handle through fields whose tiles leave and join on every level; between two steps the solid mask is set anew (a full
    pass over the level-1 types), between two others the vector type changes. After every set-up M^-1 on two right-hand sides is the
    stateless model of that step's field and bit-identical to a fresh handle that was given only that step. `solve`: a solve after
    every step, so that the V-cycles of a whole solve have written to every level before the next set-up."""
    other = lfa.PCG_F32 if dtype == lfa.PCG_F64 else lfa.PCG_F64
    cur = dtype
    steps = SEQUENCES[seq]
    s = new_sim(steps[0][0], cur)
    for k, (name, event) in enumerate(steps):
        if event and "dtype" in event:
            cur = other if cur == dtype else dtype
            s.set_params(pcg_dtype=cur)
        set_up(s, name, solids=bool(event and "solids" in event))
        what = f"{seq} {DTYPE_ID[dtype]} step {k} {name} {DTYPE_ID[cur]}"
        inputs_identical(s, name, what)
        got = all_held(s, name, cur, what, labels=("random", "b"))
        fresh = new_sim(name, cur)
        set_up(fresh, name)
        for label, z in got.items():
            assert np.array_equal(z, fresh.apply_precon(vc.rhs(name)[label])), f"{what} {label}: not bit-identical to a fresh handle"
        fresh.close()
        if solve:
            p, res, it, rc = s.solve(vc.DT)
            print(f"ITERS {what}: {it}")
            assert rc == 0 and res < 1e-6
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", vc.FIELDS)
def test_solve_takes_the_models_iterations(name, dtype):
    """The solve runs the finest level's pre-smoothing fused with the AXPYs (k_mg_axpy_presmooth), which lfa_apply_preconditioner does
    not: fp64 takes the model PCG's iterations, +- 1. fp32: printed."""
    w = vc.system(name)
    _, want = vc.model_pcg(name)
    s = new_sim(name, dtype)
    set_up(s, name)
    p, res, it, rc = s.solve(vc.DT)
    s.close()
    print(f"ITERS {name} multigrid {DTYPE_ID[dtype]} {it} (model {want}, oracle {w['iters']})")
    assert rc == 0 and res < 1e-6
    if dtype == lfa.PCG_F64:
        assert abs(int(it) - want) <= 1, (it, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
def test_plate_reaches_the_wave_per_tile_coarse_kernels(dtype, monkeypatch):
    """1 089 active tiles on level 1: more than the cell-parallel kernels and the fused top level take (1 024), so level 1 runs
    k_mg_presmooth, k_mg_residual_restrict and k_mg_prolong_postsmooth<real, false, 1>."""
    got = []
    for knob in (None, "LFA_MG_NO_PERSIST"):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if knob:
            monkeypatch.setenv(knob, "1")
        s = new_sim("plate", dtype)
        set_up(s, "plate")
        what = f"plate {DTYPE_ID[dtype]} {'phase' if knob else 'default'}"
        inputs_identical(s, "plate", what)
        assert s.mg_level_tiles()[:2] == [4225, 1089]
        got.append(all_held(s, "plate", dtype, what, labels=("random",))["random"])
        s.close()
    assert np.array_equal(got[0], got[1])
