"""GPU tests (-m gpu) of the grid stages around the pressure solve on the cell fields of tests/stencil_cases.py: k_abits, k_rhs,
lfa_apply_a, k_apply_pressure, k_extrapolate and the solve under every preconditioner, each stage from the oracle's state of the
stage before it. The oracle is handed the very fp32-rounded grids that are uploaded (stencil_cases.staged(rounded=True)), so the
rounding of a stage's input is part of no error. tests/test_stencil_cases.py pins the oracle to the reference on these inputs.

The max-norm bars are those of tests/test_gpu_parity.py. On top of them the two velocity stages are held face by face: what the
oracle leaves bit-identical stays bit-identical, what it sets to exactly 0 is exactly 0, and every other face lies within a counted
number of fp32 roundings of the oracle's value - a face handled by the wrong rule beside a small pressure, or a face the stage must
not touch, does not hide behind the largest entry of the field. No face is masked out.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts, every solve `ITERS <case> <preconditioner> <dtype> <n>`
(pytest -s shows them; docs/experiments.md records them).
"""
import numpy as np
import pytest

import libfluid_amd as lfa
from tests import stencil_cases as sc
from tests import util
from tests.test_gpu_parity import P_REL, VEL_REL, cells_from

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24  # half an ulp of fp32, relative
# k_apply_pressure, one face: u - coeff * ((p_n or 0) - p_c). Roundings, each at most EPS * s with s = |u| + coeff (|p_c| + |p_n|):
#   p_c and p_n to fp32 (together: EPS * coeff (|p_c| + |p_n|))   1
#   coeff = dt / (rho h) to fp32                                  1
#   the difference of the two pressures                           1
#   its product with coeff                                        1
#   the subtraction from u                                        1
#   storage (the fp32 face velocity that is downloaded)           1
# A face takes this path at most once where the types come from the P2G: the second rule of a face (from its +d cell) only computes
# when the -d cell is air, and an air cell holds no particles. On a grid with edited types (`retyped`) an unknown typed AIR below an
# unknown gets both: the second product (1) and a second subtraction whose result may reach 2 s (2) on top.
K_APPLY = 6
K_APPLY_TWICE = K_APPLY + 3
# k_extrapolate, one component: up to six fp32 additions (6), one division by the count (1), storage (1); each at most
# EPS * max |valid neighbour component| once divided by the count. From the second sweep on the averaged values carry the
# error of the sweep before: stencil_cases.extrapolate_sweeps adds the largest unit among them.
K_EXTRAP = 8
DTYPES = [lfa.PCG_F32, lfa.PCG_F64]
DTYPE_ID = {lfa.PCG_F32: "f32", lfa.PCG_F64: "f64"}
PRECONDS = [lfa.PRECOND_MIC0_TILED, lfa.PRECOND_MULTILEVEL, lfa.PRECOND_MULTIGRID]
PRECOND_ID = {lfa.PRECOND_MIC0_TILED: "mic0_tiled", lfa.PRECOND_MULTILEVEL: "multilevel", lfa.PRECOND_MULTIGRID: "multigrid"}


def margin(what, err, bar):
    print(f"MARGIN {what} {err / bar if bar > 0 else (0.0 if err == 0 else float('inf')):.3f}")


def close(a, b, rel, what):
    """util.assert_close at the max-norm bar `rel`, the margin printed first."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    margin(what, float(np.abs(a - b).max()) if a.size else 0.0, rel * scale)
    util.assert_close(a, b, rel, what)


def pointwise(got, want, bar, what):
    """|got - want| <= bar, entry by entry; prints the largest ratio."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = np.divide(err, bar, out=np.where(err > 0, np.inf, 0.0), where=bar > 0)
    print(f"MARGIN {what} {float(ratio.max()) if ratio.size else 0.0:.3f}")
    worst = int(np.argmax(ratio)) if ratio.size else 0
    assert (err <= bar).all(), f"{what}: {int((err > bar).sum())} of {err.size} entries beyond their bar, worst {ratio.reshape(-1)[worst]:.3g} x at {worst}"


def make_sim(name, **extra):
    size, parts, solid, meta = sc.build(name)
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], density=meta["rho"], method=lfa.APIC, blending=1.0, **extra)
    if solid is not None:
        s.set_solid_cells(solid)
    s.upload_particles(parts)
    return s


def on_the_oracles_grid(name, **extra):
    """A handle that has binned the case's particles and holds the oracle's grid after gravity (fp32-rounded: exactly what the
    oracle went on from)."""
    want = sc.oracle_stages(name, True)
    s = make_sim(name, **extra)
    s.hash()
    s.upload_cells(cells_from(want["grav_vel"], want["type"]))
    return s, want


@pytest.mark.parametrize("name", sc.NAMES)
def test_unknowns_types_and_matrix_bits_exact(name):
    """The device's own binning and P2G (cell types from the particle counts and the solid mask, as in a step - nothing uploaded),
    then k_abits: fluid cells, counts, types and A bits bit for bit."""
    want = sc.oracle_stages(name, True)
    s = make_sim(name)
    s.hash()
    assert np.array_equal(s.fluid_cells(), want["fluid_cells"])
    assert np.array_equal(s.cell_counts(), want["counts"])
    s.p2g()
    s.add_gravity(sc.DT)
    cells = s.cells()
    assert np.array_equal(cells["type"], want["p2g_type"])
    if not np.array_equal(want["type"], want["p2g_type"]):  # `retyped`: the host edits the types between gravity and the solve
        cells["type"] = want["type"]
        s.upload_cells(cells)
    s.build_system(sc.DT)
    assert np.array_equal(s.abits(), want["abits"]), np.flatnonzero(s.abits() != want["abits"])[:10]
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", sc.NAMES)
def test_rhs_and_matrix_probe(name, dtype):
    """k_rhs and lfa_apply_a on the oracle's grid: A bits again (types uploaded this time), b at 1e-6 and the probe A (sin(0.37 i) +
    0.25) at 1e-6 (fp32 vectors) / 1e-13 (fp64) of their maxima."""
    s, want = on_the_oracles_grid(name, precond=lfa.PRECOND_MIC0_EXACT, pcg_dtype=dtype)
    label = f"{name} {DTYPE_ID[dtype]}"
    s.build_system(sc.DT)
    assert np.array_equal(s.abits(), want["abits"])
    close(s.b(), want["b"], 1e-6, f"{label} b")
    close(s.apply_a(sc.probe(len(want["b"]))), want["Aprobe"], 1e-6 if dtype == lfa.PCG_F32 else 1e-13, f"{label} A_probe")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("name", sc.NAMES)
def test_apply_pressure_face_by_face(name, dtype):
    """k_apply_pressure with the oracle's pressure uploaded."""
    size, parts, solid, meta = sc.build(name)
    s, want = on_the_oracles_grid(name, pcg_dtype=dtype)
    label = f"{name} {DTYPE_ID[dtype]} apply"
    s.build_system(sc.DT)
    s.upload_pressure(want["p"])
    s.apply_pressure(sc.DT)
    got = s.cells()["vel"]
    s.close()
    vin, vout = want["grav_vel"], want["apply_exact"]
    ref, cls, scale = sc.apply_pressure_faces(size, want["type"], want["fluid_cells"], vin, want["p"], sc.coeff_of(meta))
    assert np.array_equal(ref, vout)  # the restatement that names the classes is the oracle, bit for bit
    close(got, vout, VEL_REL, f"{label} max_norm")
    same = vout == vin
    zero = (vout == 0.0) & ~same
    rest = ~same & ~zero
    assert same.any() and zero.any() and rest.any()
    print(f"FACES {label} untouched {int(same.sum())} zeroed {int(zero.sum())} computed {int(rest.sum())}")
    assert np.array_equal(got[same], vin[same]), f"{label}: {int((got[same] != vin[same]).sum())} faces changed that the oracle leaves alone"
    assert not got[zero].any(), f"{label}: {int((got[zero] != 0).sum())} faces not exactly 0"
    assert cls["computed-twice"].any() == (name == "retyped")
    bar = np.where(cls["computed-twice"], K_APPLY_TWICE, K_APPLY) * EPS * scale
    for k in sc.FACE_CLASSES:
        m = cls[k] & rest
        if m.any():
            pointwise(got[m], vout[m], bar[m], f"{label} {k}")
    pointwise(got[rest], vout[rest], bar[rest], f"{label} computed_faces")


@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("name", sc.NAMES)
def test_extrapolation_component_by_component(name, sweeps):
    """k_extrapolate with 1 sweep (validity from the particle counts) and with 3 (validity bytes from sweep to sweep), from the oracle's
    applied grid."""
    size, parts, solid, meta = sc.build(name)
    want = sc.oracle_stages(name, True)
    label = f"{name} extrapolate_{sweeps}"
    s = make_sim(name, velocity_extrapolation_iterations=sweeps)
    s.hash()
    s.upload_cells(cells_from(want["apply_vel"], want["type"]))
    s.extrapolate()
    got = s.cells()["vel"]
    s.close()
    vin, vout = want["apply_vel"], want[f"extrap{sweeps}_vel"]
    ref, written, count, born, unit = sc.extrapolate_sweeps(size, want["type"], want["fluid_cells"], vin, sweeps)
    assert np.array_equal(ref, vout)
    close(got, vout, VEL_REL, f"{label} max_norm")
    print(f"FACES {label} untouched {int((~written).sum())} written {int(written.sum())}")
    assert np.array_equal(got[~written], vin[~written]), f"{label}: {int((got[~written] != vin[~written]).sum())} components changed that the oracle leaves alone"
    if written.any():
        pointwise(got[written], vout[written], K_EXTRAP * EPS * unit[written], f"{label} written_components")


@pytest.mark.parametrize("name", sc.NAMES)
def test_exact_schedule_solves_in_the_references_iterations(name):
    s, want = on_the_oracles_grid(name, precond=lfa.PRECOND_MIC0_EXACT, pcg_dtype=lfa.PCG_F64)
    p, res, it, rc = s.solve(sc.DT)
    s.close()
    print(f"ITERS {name} mic0_exact f64 {it} (oracle {int(want['iters'])})")
    assert rc == 0
    assert it == int(want["iters"])
    assert res < 1e-6
    close(p, want["p"], 1e-6, f"{name} exact_schedule p")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("precond", PRECONDS, ids=PRECOND_ID.get)
@pytest.mark.parametrize("name", sc.NAMES)
def test_every_preconditioner_solves_the_system(name, precond, dtype):
    """The answer, not the rate: max_iterations is 1000 here, the iteration count is printed and recorded, not asserted."""
    s, want = on_the_oracles_grid(name, precond=precond, pcg_dtype=dtype, max_iterations=1000)
    p, res, it, rc = s.solve(sc.DT)
    s.close()
    print(f"ITERS {name} {PRECOND_ID[precond]} {DTYPE_ID[dtype]} {it} (oracle {int(want['iters'])})")
    assert rc == 0 and res < 1e-6, (rc, res, it)
    close(p, want["p"], P_REL, f"{name} {PRECOND_ID[precond]} {DTYPE_ID[dtype]} p")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
def test_droplets_under_multigrid_group_by_group(dtype):
    """The pool's pressures are a hundred times a droplet's: a max-norm over everything would hide the droplets. The 64-unknown tile
    (closed: solved on its own), the 65-unknown tile (one too many: stays in the PCG), the pairs across a tile face and the particle
    inside a solid cell are each compared against their OWN largest pressure. The closed-tile flags of k_abits show in the number
    of tiles the PCG iterates over. And the preconditioner, closed tiles included, is symmetric positive definite."""
    size, parts, solid, meta = sc.build("droplets")
    nx, ny, nz = size
    s, want = on_the_oracles_grid("droplets", precond=lfa.PRECOND_MULTIGRID, pcg_dtype=dtype, max_iterations=1000)
    fc = want["fluid_cells"].astype(np.int64)
    s.build_system(sc.DT)
    n = len(fc)
    rng = np.random.default_rng(21)
    x, y = rng.normal(size=n), rng.normal(size=n)
    mx, my = s.apply_precon(x), s.apply_precon(y)
    sym = abs(y @ mx - x @ my)
    bar = (2e-5 if dtype == lfa.PCG_F32 else 1e-11) * (abs(y @ mx) + np.linalg.norm(x) * np.linalg.norm(my))
    margin(f"droplets multigrid {DTYPE_ID[dtype]} precon_symmetry", sym, bar)
    assert sym <= bar
    assert x @ mx > 0 and y @ my > 0
    p, res, it, rc = s.solve(sc.DT)
    iterated, n_ptiles = s.mg_level_tiles()[0], s.counts()["particle_tiles"]
    s.close()
    assert rc == 0 and res < 1e-6, (rc, res, it)
    # closed: 1 .. 64 unknowns and no coupling across a tile face - from the oracle's A bits
    per_tile = sc.unknowns_per_tile(size, fc)
    coupled = sc.couplings_across_tile_faces(size, want["type"], fc, want["abits"])
    closed = {t for t, k in per_tile.items() if k <= sc.CLOSED_MAX and t not in coupled}
    assert meta["tile64"] in closed and meta["tile65"] not in closed and (0, 1, 0) in closed
    assert n_ptiles == len(per_tile)
    assert iterated == n_ptiles - len(closed), (iterated, n_ptiles, sorted(closed))
    for k in ("tile64", "tile65", "straddle_x", "straddle_y", "straddle_z", "in_solid", "on_solid", "interior", "cell7", "walls", "corner"):
        at = np.searchsorted(fc, [cx + nx * (cy + ny * cz) for cx, cy, cz in meta["groups"][k]])
        close(p[at], want["p"][at], P_REL, f"droplets multigrid {DTYPE_ID[dtype]} p_{k}")
    close(p, want["p"], P_REL, f"droplets multigrid {DTYPE_ID[dtype]} p")
