"""GPU tests (-m gpu): pressure solves IN SEQUENCE on one handle, every step against the oracle's cold fp64 answer
(tests/solve_sequence_cases.py; tests/test_solve_sequence_cases.py pins the designs without a device).

The solver keeps state between solves - the epochs that decide a warm start, per handle and per tile, `warm_started`,
`last_rhs_zero`, `pcg_poisoned`, `last_iters`, the multigrid hierarchy and its level-0 list without the closed tiles, the closed-tile
flags - and the sequences walk through its combinations: the same system again, a slightly and a wholly different one, a scene at
rest and moving again, tiles that leave, come back, open and close, nothing but closed tiles, a capped solve, a NaN, another
preconditioner or vector type, and two passes of the whole hot path.

After EVERY step: unknowns and A bits bit for bit, the return code, the residual, no device-side wait given up, and the pressure at
P_REL of the whole field's maximum AND group by group at P_REL of each group's own maximum (the pool's pressures are two hundred
times a droplet's). These are the bars of the cold test on this field (test_droplets_under_multigrid_group_by_group): a
warm-started or re-used handle gets no allowance. A step is checked to its end and the sequence goes on; what missed is listed when
the sequence is over.

Prints `ITERS <sequence> <parameters> step <k> <field> x <f>: <n> (oracle <n>)` and `MARGIN <what> <error / bar>` (pytest -s;
docs/experiments.md records them).
"""
import numpy as np
import pytest

import libfluid_amd as lfa
from tests import solve_sequence_cases as q
from tests import stencil_cases as sc
from tests import util
from tests.test_gpu_parity import P_REL, VEL_ATOL, cells_from
from tests.test_gpu_stencil_edges import DTYPE_ID, DTYPES, PRECOND_ID, PRECONDS, close, margin

pytestmark = pytest.mark.gpu

assert q.P_REL == P_REL
E_NAN = -5
W_NOT_CONVERGED = 1
WARM_ID = {0: "cold", 1: "warm"}
MG, TILED = lfa.PRECOND_MULTIGRID, lfa.PRECOND_MIC0_TILED


class Tally:
    """Checks that are all made before the first of them fails the test."""

    def __init__(self, label):
        self.label, self.missed = label, []

    def that(self, ok, what):
        if not ok:
            self.missed.append(f"{self.label} {what}")

    def close(self, a, b, rel, what):
        try:
            close(a, b, rel, f"{self.label} {what}")
        except AssertionError as e:
            self.missed.append(str(e).splitlines()[0] if str(e) else f"{self.label} {what}")

    def done(self):
        assert not self.missed, f"{len(self.missed)} checks missed:\n" + "\n".join(self.missed)


def new_sim(**extra):
    size, _, solid, meta = sc.build("droplets")
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], density=meta["rho"], method=lfa.APIC, blending=1.0, **extra)
    s.set_solid_cells(solid)
    return s


def hand_over(s, field, rec, rehash):
    """The step's particles (where the field changes) and the oracle's grid after gravity, as on_the_oracles_grid does."""
    if rehash:
        s.upload_particles(q.particles(field))
        s.hash()
    s.upload_cells(cells_from(rec["vel"], rec["type"]))


def pressure_held(t, field, rec, p, what):
    """Whole field and every group against its own maximum, both at P_REL."""
    if p.shape != rec["p"].shape:
        return t.that(False, f"{what}: {p.shape[0]} pressures for {rec['p'].shape[0]} unknowns")
    for g, at in q.group_indices(field, rec).items():
        t.close(p[at], rec["p"][at], P_REL, f"{what} p_{g}")
    t.close(p, rec["p"], P_REL, f"{what} p")


def system_held(t, s, rec, what):
    t.that(np.array_equal(s.fluid_cells(), rec["fluid_cells"]), f"{what}: fluid_cells differ")
    t.that(np.array_equal(s.abits(), rec["abits"]), f"{what}: A bits differ")
    t.that(s.solver_stats()["device_waits_given_up"] == 0, f"{what}: a device-side wait was given up")


def run(name, label, s, params=None, expect=None, steps=None):
    """The sequence on the handle `s`. params[k]: set_params before step k; expect[k]: "ok" (default), "capped" or "nan".
    Returns per step (p, iterations) - None for a NaN step."""
    t = Tally(f"{name} {label}")
    steps = q.SEQUENCES[name] if steps is None else steps
    out, before = [], None
    for k, step in enumerate(steps):
        rec = q.solved(step)
        what = f"step {k} {step.field} x {step.f:g}"
        if params and params.get(k):
            s.set_params(**params[k])
        hand_over(s, step.field, rec, step.field != before)
        before = step.field
        kind = (expect or {}).get(k, "ok")
        if kind == "nan":
            try:
                _, _, _, rc = s.solve(q.DT)
                t.that(False, f"{what}: a NaN right-hand side came back with code {rc}")
            except lfa.LibfluidError as e:
                t.that(e.code == E_NAN, f"{what}: error code {e.code}")
            system_held(t, s, rec, what)
            out.append(None)
            continue
        p, res, it, rc = s.solve(q.DT)
        print(f"ITERS {name} {label} {what}: {it} (oracle {rec['iters']})")
        system_held(t, s, rec, what)
        out.append((p, it))
        if kind == "capped":
            t.that(rc == W_NOT_CONVERGED and it == s.params.max_iterations, f"{what}: capped solve returned {rc} after {it}")
            continue
        t.that(rc == 0, f"{what}: return code {rc}")
        t.that(res < 1e-6, f"{what}: residual {res:.3e}")
        if step.f == 0.0:
            t.that(it == 0, f"{what}: {it} iterations on a zero right-hand side")
            t.that(not p.any(), f"{what}: {int(np.count_nonzero(p))} pressures not exactly 0, largest {np.abs(p).max():.3e}")
            continue
        if s.params.precond == MG:
            lv = s.mg_level_tiles()
            n_pt = s.counts()["particle_tiles"]
            t.that(n_pt == len(rec["tiles"]) and (lv[0] if lv else 0) == n_pt - len(rec["closed"]),
                   f"{what}: the PCG iterates over {lv[0] if lv else 0} of {n_pt} tiles, {len(rec['closed'])} are closed")
        pressure_held(t, step.field, rec, p, what)
    return t, out


# ---------------------------------------------------------------------------------------------------- the sequences
REPEAT = [(pc, dt, 1) for pc in PRECONDS for dt in DTYPES] + [(MG, dt, 0) for dt in DTYPES]


@pytest.mark.parametrize("precond,dtype,warm", REPEAT, ids=[f"{PRECOND_ID[a]}-{DTYPE_ID[b]}-{WARM_ID[c]}" for a, b, c in REPEAT])
def test_repeat(precond, dtype, warm):
    """A, A again, A x 1.001, A x -0.5. Warm: the same system again takes no more iterations than the first time. Cold: it returns
    the same bits in the same iterations."""
    s = new_sim(precond=precond, pcg_dtype=dtype, pcg_warm_start=warm)
    t, out = run("repeat", f"{PRECOND_ID[precond]} {DTYPE_ID[dtype]} {WARM_ID[warm]}", s)
    s.close()
    (p0, it0), (p1, it1) = out[0], out[1]
    if warm:
        t.that(it1 <= it0, f"the same system again, warm: {it1} iterations after {it0}")
    else:
        t.that(it1 == it0 and np.array_equal(p0, p1), f"the same system again, cold: {it1} iterations after {it0}, bits differ")
    t.done()


@pytest.mark.parametrize("warm", [0, 1], ids=WARM_ID.get)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("field", ["A", "S"])
def test_rest(field, dtype, warm):
    """Moving, at rest, at rest, moving: the first zero right-hand side is found on the device (k_check_rhs), the second by the host
    (last_rhs_zero); p is exactly 0 both times, previous pressure or not, and the solve after them is the oracle's again."""
    s = new_sim(precond=MG, pcg_dtype=dtype, pcg_warm_start=warm)
    t, _ = run(f"rest_{field}", f"{DTYPE_ID[dtype]} {WARM_ID[warm]}", s)
    s.close()
    t.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("precond", [MG, TILED], ids=PRECOND_ID.get)
def test_come_and_go(precond, dtype):
    """A, B, A, S, A on one handle, warm: a tile leaves and comes back (its old pressure is no guess), a closed tile opens and closes
    again, the PCG's tile list empties and fills."""
    s = new_sim(precond=precond, pcg_dtype=dtype, pcg_warm_start=1)
    t, _ = run("come_and_go", f"{PRECOND_ID[precond]} {DTYPE_ID[dtype]} warm", s)
    s.close()
    t.done()


def test_capped():
    """A capped solve is no guess: the solve after it equals, bit for bit and in its iterations, the first solve of a fresh handle."""
    s = new_sim(precond=MG, pcg_warm_start=1)
    t, out = run("capped", "multigrid f32 warm", s, params={0: dict(max_iterations=3), 1: dict(max_iterations=200)}, expect={0: "capped"})
    s.close()
    f = new_sim(precond=MG, pcg_warm_start=1)
    t2, fresh = run("capped", "multigrid f32 fresh", f, steps=q.SEQUENCES["capped"][1:])
    f.close()
    t.missed += t2.missed
    t.that(out[1][1] == fresh[0][1] and np.array_equal(out[1][0], fresh[0][0]),
           f"after the capped solve: {out[1][1]} iterations, a fresh handle {fresh[0][1]}, largest difference {np.abs(out[1][0] - fresh[0][0]).max():.3e}")
    t.done()


def test_switch():
    """Another preconditioner, another vector type and the first preconditioner again between solves of one handle."""
    s = new_sim(precond=MG, pcg_dtype=lfa.PCG_F32, pcg_warm_start=1)
    t, _ = run("switch", "warm", s, params={1: dict(precond=TILED), 2: dict(pcg_dtype=lfa.PCG_F64), 3: dict(precond=MG)})
    s.close()
    t.done()


@pytest.mark.parametrize("warm", [0, 1], ids=WARM_ID.get)
@pytest.mark.parametrize("field", ["A", "S"])
def test_nan(field, warm):
    """One NaN face velocity - in a pool cell (A: the PCG meets it), in a droplet of a closed tile (S: only k_mg_solve_closed does) -
    is LFA_E_NAN, and the next solve of the handle is the oracle's."""
    s = new_sim(precond=MG, pcg_warm_start=warm)
    t, _ = run(f"nan_{field}", WARM_ID[warm], s, expect={0: "nan"})
    s.close()
    t.done()


@pytest.mark.parametrize("warm", [0, 1], ids=WARM_ID.get)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_ID.get)
@pytest.mark.parametrize("field", ["A", "S"])
def test_hot(field, dtype, warm):
    """Two step_hot from the field's particles against the oracle's two hot steps: the second system is the device's own (its P2G of
    the velocities its G2P wrote), and with a warm start it begins at the first step's pressure."""
    label = f"{DTYPE_ID[dtype]} {WARM_ID[warm]}"
    t = Tally(f"hot_{field} {label}")
    parts = q.particles(field)
    s = new_sim(precond=MG, pcg_dtype=dtype, pcg_warm_start=warm)
    s.upload_particles(parts)
    for k, rec in enumerate(q.hot_steps(field)):
        what = f"step {k}"
        res, it, rc = s.step_hot(q.DT)
        print(f"ITERS hot_{field} {label} {what}: {it} (oracle {rec['iters']})")
        system_held(t, s, rec, what)
        t.that(rc == 0, f"{what}: return code {rc}")
        t.that(res < 1e-6, f"{what}: residual {res:.3e}")
        pressure_held(t, field, rec, s.pressure(), what)
        try:  # (the bars of test_two_hot_steps_end_to_end)
            vel = s.cells()["vel"]
            margin(f"hot_{field} {label} {what} grid", float(np.abs(vel - rec["grid_vel"]).max()), 1e-4 * float(np.abs(rec["grid_vel"]).max()) + VEL_ATOL)
            util.assert_close(vel, rec["grid_vel"], 1e-4, f"{what} grid", atol=VEL_ATOL)
            got = s.download_particles(into=parts.copy())
            got, want = got[util.order_by_position(got)], rec["parts"]
            assert np.array_equal(got["pos"], want["pos"])
            margin(f"hot_{field} {label} {what} particle_velocity", float(np.abs(got["vel"] - want["vel"]).max()), 1e-4 * float(np.abs(want["vel"]).max()) + VEL_ATOL)
            util.assert_close(got["vel"], want["vel"], 1e-4, f"{what} particle velocity", atol=VEL_ATOL)
            c_got, c_want = (np.concatenate([a["cx"], a["cy"], a["cz"]], axis=1) for a in (got, want))
            margin(f"hot_{field} {label} {what} particle_C", float(np.abs(c_got - c_want).max()), 2e-4 * float(np.abs(c_want).max()) + VEL_ATOL)
            util.assert_close(c_got, c_want, 2e-4, f"{what} particle C", atol=VEL_ATOL)
        except AssertionError as e:
            t.missed.append(f"{t.label} {str(e).splitlines()[0]}")
    s.close()
    t.done()
