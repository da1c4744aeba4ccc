"""CPU tests of tests/vcycle_model.py (the multigrid V-cycle of mg.hip in numpy, fp64) and of the fields of tests/vcycle_cases.py:
the model is a symmetric positive definite operator, PCG under it reaches the oracle's pressure, the new field `terraces` holds what
it is built to hold, and the bars of tests/test_gpu_vcycle.py tell the model from each of its ten one-rule mutants by a factor of
100 at least. No GPU.

Iterations of the model PCG (fp64, the stopping rule of pcg.hip; closed tiles solved on their own) against the oracle's MIC(0):

  field             model PCG   oracle        field             model PCG   oracle
  maze                      7       17        walls_x                   7       12
  maze_h17                  7       16        terraces                 12       43
  maze_h05                  8       17        terraces_shifted         14       32
  droplets                  8       15        terraces_half            13       39
  sheets                    6        7        A                         8       15
  thin_2_9_17               7        9        B                         8       15
  thin_8_8_8               14       20        S                         0        8
  retyped                   5        8        terraces_half_solid      13       39
  (S: every tile is closed - nothing is left to iterate over)
"""
import numpy as np
import pytest

from oracle import loader as orc
from tests import solve_sequence_cases as ssc
from tests import stencil_cases as sc
from tests import vcycle_cases as vc
from tests import vcycle_model as vm

needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
ALL = vc.FIELDS + vc.SEQUENCE_FIELDS + ("terraces_shifted", "terraces_half", "terraces_half_solid")
# (`plate` has no closed tile - asserted below -, so "no_closed" would be the same model again)
SPD = [(n, c) for n in ALL for c in (True, False)] + [("plate", True)]


@pytest.mark.parametrize("name,closed", SPD, ids=[f"{n}-{'closed_tiles' if c else 'no_closed'}" for n, c in SPD])
def test_model_is_symmetric_positive_definite(name, closed):
    H = vc.model(name, closed)
    n = len(H.index[0])
    rng = np.random.default_rng(3)
    x, y = rng.normal(size=n), rng.normal(size=n)
    mx, my = vm.vcycle(H, x), vm.vcycle(H, y)
    assert abs(y @ mx - x @ my) <= 1e-12 * (abs(y @ mx) + np.linalg.norm(x) * np.linalg.norm(my))
    assert x @ mx > 0 and y @ my > 0
    if closed and name in vc.FIELDS:  # ... and on every right-hand side the device is held to (the model's z: computed once, shared)
        for label, r in vc.rhs(name).items():
            assert r @ vc.reference(name, label)[0] > 0, label
    if name == "plate":
        assert not H.closed


@pytest.mark.parametrize("name", ALL)
def test_model_pcg_reaches_the_oracles_pressure(name):
    w = vc.system(name)
    p, it = vc.model_pcg(name)
    print(f"ITERS {name} model_pcg {it} (oracle {w['iters']})")
    assert np.abs(p - w["p"]).max() <= ssc.P_REL * np.abs(w["p"]).max()
    assert it <= w["iters"]


def test_level_grids_halve_until_one_tile():
    assert vm.level_grids(vc.TERRACES_SIZE) == [(70, 37, 53), (35, 19, 27), (18, 10, 14), (9, 5, 7), (5, 3, 4)]
    assert vm.level_grids((8, 8, 8)) == [(8, 8, 8)] and vm.level_grids((2, 9, 17))[1:] == [(1, 5, 9), (1, 3, 5)]
    assert vm.level_grids(vc.PLATE_SIZE)[:2] == [(520, 8, 520), (260, 4, 260)]


def test_terraces_holds_what_it_is_built_for():
    f = vc.build("terraces")[3]["conditions"]  # computed by the builder from the model's own hierarchy
    H = vc.model("terraces")
    assert f["levels"] == 5 and f["last"] == 4
    assert [L.nt for L in H.levels] == [(9, 5, 7), (5, 3, 4), (3, 2, 2), (2, 1, 1), (1, 1, 1)]
    assert f["pruned_with_active_child"] >= 1
    assert f["inactive_fluid_neighbour"] >= 1
    assert f["inactive_octants"] >= 1
    assert all(n >= 1 for n in f["unknowns_per_level"])
    assert sum(n >= 1 for n in f["outside_children"]) == 3 and f["outside_children_fluid"] >= 1
    assert all(all(v) for v in f["cell_0_and_7"]) and len(f["cell_0_and_7"]) == 3
    assert f["unknown_in_inactive_octant"] >= 1
    assert f["closed"] >= 3
    ptiles, closed = vc.tiles_of(vc.system("terraces"))
    assert {(4, 2, 0), (5, 1, 3)} <= closed and (6, 3, 2) in ptiles - closed and (7, 3, 2) in ptiles - closed  # the pair stays open
    z, y, x = H.index
    for d, n in enumerate(vc.TERRACES_SIZE):
        assert ((x, y, z)[d] == n - 1).any()  # fluid in the last ragged layer of each axis
    for m in vm.MUTANTS:
        assert vc.visible("terraces", m), m
    # the impulses beside a pillar exist, sit in tiles the V-cycle runs on, and have a face neighbour in the pillar
    picks, sm, op = vc.designed_unknowns("terraces"), vc.solid_mask("terraces"), vm.open_mask(H)
    assert len(picks) <= 24 and len(set(picks.values())) == len(picks)
    for k, ((x0, x1), (z0, z1)) in vc.PILLARS.items():
        i = picks[f"pillar_{k}"]
        assert op[i] and z0 <= z[i] <= z1 and y[i] <= 25
        assert (x[i] == x0 - 1 and sm[z[i], y[i], x0]) or (x[i] == x1 + 1 and sm[z[i], y[i], x1])
    assert (vc.PILLARS["aligned"][0][0] % 2, vc.PILLARS["unaligned"][0][0] % 2) == (0, 1)
    assert op[picks["by_solid"]] and "group_pair" in picks and "pruned_child" in picks


def test_predicted_level_tiles_of_the_sequence_fields():
    """A: 20 particle tiles, 5 closed; B: 19, 3 closed; S: every tile closed - level 0 is empty and so is every level above it."""
    # 40 x 16 x 16: the level grids have 5 x 2 x 2, 3 x 1 x 1, 2 x 1 x 1 and 1 tiles, and the pool lies under every one of them
    assert vc.model("A").tiles == [15, 3, 2, 1] and len(vc.model("A").closed) == 5
    assert vc.model("B").tiles == [16, 3, 2, 1] and len(vc.model("B").closed) == 3
    assert vc.model("S").tiles == [0, 0, 0, 0] and vc.model("S").last == 0
    assert vc.model("plate").tiles[:2] == [4225, 1089]


@pytest.mark.parametrize("name", vc.FIELDS)
def test_bars_discriminate_every_mutant_the_field_can_see(name):
    """max |V_mutant(r) - V(r)| >= 100 fp32 bars (= 800 d32) on at least one right-hand side of the field."""
    shown = 0
    for m in vm.MUTANTS:
        if not vc.visible(name, m):
            continue
        shown += 1
        Hm, H = vc.model(name, mutant=m), vc.model(name)
        op = vm.open_mask(H)
        best = 0.0
        for label, r in vc.rhs(name).items():
            z, d32 = vc.reference(name, label)
            err = np.abs(vm.vcycle(Hm, r, mutant=m) - z)
            # the V-cycle's share against 8 d32, the closed tiles' against the bar of their own solve (fp32)
            bars = np.where(op, 8.0 * d32, vc.closed_bars(H, r, False))
            ratio = np.divide(err, bars, out=np.where(err > 0, np.inf, 0.0), where=bars > 0)
            best = max(best, float(ratio.max()))
            if best >= 100.0:
                break
        print(f"MUTANT {name} {m} {best:.3g} fp32 bars")
        assert best >= 100.0, (name, m, best)
    assert shown >= 1


@pytest.mark.parametrize("name", ["terraces", "terraces_shifted", "terraces_half"])
def test_terraces_is_well_posed(name):
    w = vc.system(name)
    assert ((w["abits"] & 7) > 0).all()
    assert np.isfinite(w["p"]).all() and np.abs(w["p"]).max() > 0 and 0 < w["iters"] < 200
    assert np.isfinite(w["b"]).all() and np.isfinite(w["vel"]).all()


def test_plate_is_well_posed_and_its_restated_system_is_the_oracles():
    """The plate's level-0 inputs are restated in numpy (vcycle_cases.plate_system_of): on a 24 x 8 x 17 plate the oracle's hash and
    build_system give the same unknowns, counts and A bytes."""
    size = (24, 8, 17)
    mine = vc.plate_system_of(size)
    nx, ny, nz = size
    z, y, x = np.meshgrid(np.arange(nz), np.arange(2), np.arange(nx), indexing="ij")
    parts = np.zeros(x.size, dtype=sc.PARTICLE_DTYPE)
    parts["pos"] = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1) + 0.5
    parts["old_pos"] = parts["pos"]
    s = orc.CpuSim(size, method=sc.APIC, blending=1.0)
    s.set_particles(parts)
    s.hash()
    assert np.array_equal(s.fluid_cells(), mine["fluid_cells"]) and np.array_equal(s.space_hash()[1], mine["counts"])
    s.p2g()
    assert np.array_equal(s.cells()["type"], mine["type"])
    s.build_system(vc.DT)
    assert np.array_equal(s.abits(), mine["abits"])
    s.close()
    w = vc.system("plate")
    assert ((w["abits"] & 7) > 0).all() and len(w["fluid_cells"]) == 520 * 2 * 520
    H = vc.model("plate")
    assert not H.closed and H.last == len(H.levels) - 1


@needs_ref
def test_oracle_is_the_reference_on_terraces():
    """At the stages the model reads: unknowns, counts, types, A bytes (and b, p for the right-hand sides and the model PCG)."""
    want, got = vc.staged("terraces", "ref"), vc.system("terraces")
    for k in ("fluid_cells", "counts", "type", "abits", "iters"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("b", "p", "vel"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
