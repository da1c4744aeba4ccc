"""GPU tests (-m gpu) of the tile-local and the multilevel MIC(0) preconditioner (libfluid_amd/csrc/pcg.hip) against
tests/multilevel_model.py, the operator in numpy and fp64, on the fields and right-hand sides of tests/multilevel_cases.py.

What runs which kernel against the model:

  k_mic_factor<real, false>                      test_tile_factor_is_the_model
  k_mic_apply<SWEEP_BOTH, false>, k_add_coarse,
  k_coarse_coeffs, k_coarse_factor, k_coarse_all test_operator_is_the_model (every field); the A2 assembly and its inverse with it
  k_coarse_apply, k_coarse_top                   test_operator_is_the_model[plate-multilevel] (81 level-1 blocks), and the solves on it
  k_mic_apply<SWEEP_BOTH, true> (embedded coarse
  workgroups), k_axpy_max's restriction,
  k_update_s's prolongation                      test_solve_iterates_are_the_models[...-unfused], k = 2, 3
  k_pcg_a's prolongation and P^T A s, k_pcg_b
  with fast_tile_sweeps, the restricted residual
  by linearity, its embedded coarse workgroups   test_solve_iterates_are_the_models[...-fused], k = 2, 3
  step_fused's non-embedded branch               test_solve_iterates_are_the_models[plate-multilevel-...-fused]

The level-0 inputs are the oracle's (the fp32-rounded grid after gravity is uploaded; `plate`: the device's own P2G and gravity on
particles at rest, held to vcycle_cases.plate_system_of); every test first asserts that the device's unknowns and A bytes are
identical. A solve's right-hand side is the device's own b, downloaded - held to the oracle's at 1e-6 where there is one -, so that
the rounding of an input is part of no error. Bars: multilevel_cases / vcycle_cases.fp32_deviation. No unknown is left out.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts, every solve `ITERS ...` (pytest -s shows them;
docs/experiments.md records them).
"""
import numpy as np
import pytest

import libfluid_amd as lfa
from tests import multilevel_cases as mc
from tests import multilevel_model as mm
from tests import solve_sequence_cases as ssc
from tests.test_gpu_parity import cells_from
from tests.test_gpu_stencil_edges import DTYPE_ID, DTYPES, margin, pointwise

pytestmark = pytest.mark.gpu

PRECOND = {mm.TILED: lfa.PRECOND_MIC0_TILED, mm.MULTILEVEL: lfa.PRECOND_MULTILEVEL}
FORMS = {"fused": 1, "unfused": 0}
ITERATE_FIELDS = ("maze", "droplets", "terraces", "plate_holed", "plate")
_iterates = {}


def new_sim(name, dtype, precond, **extra):
    size, parts, solid, meta = mc.build(name)
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], density=meta["rho"], method=lfa.APIC, blending=1.0,
                precond=PRECOND[precond], pcg_dtype=dtype, **extra)
    if solid is not None:
        s.set_solid_cells(solid)
    return s


def set_up(s, name, what):
    """The field's particles binned, the oracle's grid after gravity uploaded (`plate`: the device's own P2G and gravity), the system
    built; the device's unknowns and A bytes are the oracle's. Returns the device's b."""
    size, parts, solid, meta = mc.build(name)
    w = mc.system(name)
    s.upload_particles(parts)
    s.hash()
    if name == "plate":
        s.p2g()
        s.add_gravity(mc.DT)
    else:
        s.upload_cells(cells_from(w["vel"], w["type"]))
    s.build_system(mc.DT)
    assert np.array_equal(s.fluid_cells(), w["fluid_cells"]), f"{what}: unknowns differ"
    assert np.array_equal(s.abits(), w["abits"]), f"{what}: A bytes differ"
    b = s.b()
    if w["b"] is not None:
        assert np.abs(b - w["b"]).max() <= 1e-6 * np.abs(w["b"]).max(), f"{what}: b differs"
    return b


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", mc.FIELDS + mc.PLATES)
def test_tile_factor_is_the_model(name, dtype):
    """k_mic_factor<real, false>, unknown by unknown: 1e-13 (fp64) / 1e-6 (fp32) of the model's entry."""
    what = f"{name} {DTYPE_ID[dtype]} tile_factor"
    s = new_sim(name, dtype, mm.TILED)
    set_up(s, name, what)
    got = s.precon()
    s.close()
    want = mc.model(name).tile_factor()
    assert (want > 0).all()
    pointwise(got, want, (1e-13 if dtype == lfa.PCG_F64 else 1e-6) * want, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("precond", mc.PRECONDS)
@pytest.mark.parametrize("name", mc.FIELDS + mc.PLATES)
def test_operator_is_the_model(name, precond, dtype):
    """lfa_apply_preconditioner on every right-hand side of the field, in max norm over all unknowns."""
    f64 = dtype == lfa.PCG_F64
    s = new_sim(name, dtype, precond)
    set_up(s, name, f"{name} {precond} {DTYPE_ID[dtype]}")
    failed = []
    for label, r in mc.rhs(name).items():
        what = f"{name} {precond} {DTYPE_ID[dtype]} {label}"
        z = s.apply_precon(r)
        zm, _ = mc.reference(name, label, precond)
        bar = mc.bar(name, label, precond, f64)
        err = float(np.abs(z - zm).max())
        margin(what, err, bar)
        if not err <= bar:
            failed.append(f"{what}: max |z - z_model| = {err:.3e}, bar {bar:.3e}, max |z_model| = {np.abs(zm).max():.3e}")
    assert s.solver_stats()["device_waits_given_up"] == 0
    s.close()
    assert not failed, "\n".join(failed)


def model_iterate(name, precond, k, b, f64):
    key = (name, precond, k, f64)
    if key not in _iterates:
        _iterates[key] = (b.copy(),) + mc.iterate(name, precond, k, b, f64)
    b0, p, bar = _iterates[key]
    assert np.array_equal(b0, b), "the device's right-hand side is not the one the cached model iterate was computed for"
    return p, bar


def device_iterate(name, precond, dtype, form, k, what):
    """(p_k, b): a fresh handle, max_iterations = k, no warm start, the field's own b."""
    s = new_sim(name, dtype, precond, max_iterations=k, pcg_warm_start=0, pcg_fused=FORMS[form])
    b = set_up(s, name, what)
    p, res, it, rc = s.solve(mc.DT)
    gave_up = s.solver_stats()["device_waits_given_up"]
    s.close()
    print(f"ITERS {what}: {it} (capped at {k})")
    assert rc == lfa.W_PCG_NOT_CONVERGED and it == k, (rc, it, k)
    assert gave_up == 0
    return p, b


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("precond", mc.PRECONDS)
@pytest.mark.parametrize("name", ITERATE_FIELDS)
def test_solve_iterates_are_the_models(name, precond, dtype, form):
    """p_1 holds the first application; p_2 and p_3 the prolongation in k_pcg_a / k_update_s, the restriction in k_axpy_max, the
    restricted residual that k_pcg_b carries by linearity and the embedded coarse workgroups. On the plates k = 2 alone."""
    f64 = dtype == lfa.PCG_F64
    if name not in mc.PLATES:
        assert mc.model_pcg(name, precond)[1] > 3
    failed = []
    for k in ((2,) if name in mc.PLATES else (1, 2, 3)):
        what = f"{name} {precond} {DTYPE_ID[dtype]} {form} p_{k}"
        p, b = device_iterate(name, precond, dtype, form, k, what)
        pm, bar = model_iterate(name, precond, k, b, f64)
        err = float(np.abs(p - pm).max())
        margin(what, err, bar)
        if not err <= bar:
            failed.append(f"{what}: max |p - p_model| = {err:.3e}, bar {bar:.3e}, max |p_model| = {np.abs(pm).max():.3e}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("precond", mc.PRECONDS)
@pytest.mark.parametrize("name", ["plate_holed", "terraces"])
def test_fused_and_unfused_iterates_agree(name, precond, dtype):
    """Follows from test_solve_iterates_are_the_models; asserted so that a change of one form shows here first: twice the bar."""
    f64 = dtype == lfa.PCG_F64
    what = f"{name} {precond} {DTYPE_ID[dtype]} fused_vs_unfused p_3"
    (pf, b), (pu, bu) = (device_iterate(name, precond, dtype, form, 3, f"{what} {form}") for form in FORMS)
    assert np.array_equal(b, bu)
    _, bar = model_iterate(name, precond, 3, b, f64)
    err = float(np.abs(pf - pu).max())
    margin(what, err, 2.0 * bar)
    assert err <= 2.0 * bar, f"{what}: {err:.3e}, bar {2.0 * bar:.3e}"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("precond", mc.PRECONDS)
@pytest.mark.parametrize("name", mc.FIELDS + ("plate_holed",))
def test_whole_solve_takes_the_models_iterations(name, precond, dtype, form):
    """fp64: the model PCG's iteration count +- 1; fp32: printed. The pressure at P_REL of the oracle's. (`plate` has no oracle
    solve anywhere in the suite; its iterates are held above.)"""
    w = mc.system(name)
    _, want = mc.model_pcg(name, precond)
    what = f"{name} {precond} {DTYPE_ID[dtype]} {form}"
    s = new_sim(name, dtype, precond, pcg_fused=FORMS[form], max_iterations=1000)  # (the rate is asserted in fp64 alone)
    set_up(s, name, what)
    p, res, it, rc = s.solve(mc.DT)
    gave_up = s.solver_stats()["device_waits_given_up"]
    s.close()
    print(f"ITERS {what} {it} (model {want}, oracle {w['iters']})")
    assert rc == 0 and res < 1e-6 and gave_up == 0
    err, bar = float(np.abs(p - w["p"]).max()), ssc.P_REL * float(np.abs(w["p"]).max())
    margin(f"{what} p", err, bar)
    assert err <= bar
    if dtype == lfa.PCG_F64:
        assert abs(int(it) - want) <= 1, (it, want)
