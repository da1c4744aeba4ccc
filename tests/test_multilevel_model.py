"""CPU tests of tests/multilevel_model.py (the tile-local and the multilevel MIC(0) preconditioner of pcg.hip in numpy, fp64) and of
the fields of tests/multilevel_cases.py: the model's exact form is the oracle's MIC(0) - factor, application, iteration count -, its
tiled and multilevel forms are symmetric positive definite, its coarse operators satisfy the Galerkin identities, the fields hold what
they are there for, and the bars of tests/test_gpu_multilevel.py tell the model from each of its ten one-rule mutants by a factor of
100 at least. No GPU.

The safety branch e < sigma a_ii: the tile factor takes it on 6 unknowns of maze, maze_h17 and maze_h05 and on no other field; the
level-1 factor takes it on no level-1 unknown of any field - the smallest e / a_ii seen there is 0.409 (terraces), against sigma =
0.25. That branch of k_coarse_factor is therefore run by no field here (none was built for it).

The iterations of the model PCG (fp64, on the field's own b) are pinned in ITERATIONS below.
"""
import numpy as np
import pytest

from oracle import loader as orc
from tests import multilevel_cases as mc
from tests import multilevel_model as mm
from tests import solve_sequence_cases as ssc
from tests import stencil_cases as sc
from tests import util
from tests import vcycle_cases as vc
from tests import vcycle_model as vm

GOLDEN = ["apic16", "apic16_solid", "pic_ragged", "apic_tank", "pic_h05", "flip_h17", "apic_h05", "apic_h17"]
SIZES = {"maze": (1926, 18, 1), "terraces": (48188, 145, 2), "plate": (540800, 4225, 81), "plate_holed": (130680, 1022, 24)}
# field -> iterations of the model PCG (exact, tiled, multilevel) and of the oracle's exact MIC(0); asserted below
ITERATIONS = {
    "maze": (17, 17, 19, 17), "maze_h17": (16, 17, 19, 16), "maze_h05": (17, 18, 20, 17), "droplets": (15, 22, 22, 15),
    "sheets": (7, 11, 14, 7), "thin_2_9_17": (9, 12, 15, 9), "thin_8_8_8": (20, 20, 19, 20), "retyped": (8, 11, 12, 8),
    "walls_x": (12, 16, 16, 12), "terraces": (43, 99, 61, 43), "plate_holed": (15, 25, 25, 15),
}
# mutant -> (field, preconditioner, right-hand side) on which it misses the fp32 bar by a factor of 100 at least
SHOWN_ON = {
    "no_level1": ("terraces", mm.MULTILEVEL, "A_smooth"),
    "no_level2": ("plate_holed", mm.MULTILEVEL, "A_smooth"),
    "diag_keeps_inner": ("maze", mm.MULTILEVEL, "A_smooth"),
    "weights_on_minus_face": ("terraces", mm.MULTILEVEL, "A_smooth"),
    "l1_l2_identity": ("plate_holed", mm.MULTILEVEL, "A_smooth"),
    "tile_reads_across_faces": ("terraces", mm.TILED, "b"),
    "no_tau": ("plate_holed", mm.TILED, "A_tile_constant"),
    "no_safety": ("maze", mm.TILED, "random"),
    "coarse_unscaled": ("maze_h05", mm.MULTILEVEL, "A_smooth"),
    "restrict_all_cells": ("maze", mm.MULTILEVEL, "A_tile_constant"),
}


@pytest.mark.parametrize("name", mc.FIELDS)
def test_exact_form_is_the_oracles_mic0(name):
    """Factor, application and solve of the exact form against the oracle on the field's own grid, at the fp64 bars of
    test_system_matrix_rhs_and_exact_mic (1e-13, 1e-12); the solve takes the oracle's iterations and reaches its pressure."""
    M, w = mc.model(name), mc.system(name)
    pre, probe = mc.oracle_exact(name)
    util.assert_close(M.tile_factor(exact=True), pre, 1e-13, "MIC(0) factor")
    util.assert_close(M.tile_apply(sc.probe(M.n), exact=True), probe, 1e-12, "M^-1 probe")
    p, it = M.pcg(w["b"], preconditioner=mm.EXACT)
    print(f"ITERS {name} model_exact {it} (oracle {w['iters']})")
    assert it == w["iters"] == ITERATIONS[name][0] == ITERATIONS[name][3]
    assert np.abs(p - w["p"]).max() <= 1e-9 * np.abs(w["p"]).max()


@pytest.mark.parametrize("name", GOLDEN)
def test_exact_form_is_the_references_golden_factor_and_probe(name):
    """precon0 and Mprobe0 of tests/golden/*.npz came from the real reference."""
    g, c = util.load_golden(name), util.CASES[name]
    h, _, rho = util.case_params(c)
    M = mm.Model(c["size"], g["fluid_cells0"], g["abits0"], util.DT / (rho * h * h))
    util.assert_close(M.tile_factor(exact=True), g["precon0"], 1e-13, "MIC(0) factor")
    util.assert_close(M.tile_apply(sc.probe(M.n), exact=True), g["Mprobe0"], 1e-12, "M^-1 probe")


@pytest.mark.parametrize("name", mc.FIELDS + ("plate_holed",))
def test_tiled_and_multilevel_pcg_reach_the_oracles_pressure(name):
    w = mc.system(name)
    for pc in mc.PRECONDS:
        p, it = mc.model_pcg(name, pc)
        print(f"ITERS {name} model_{pc} {it} (oracle {w['iters']})")
        assert it == ITERATIONS[name][1 + mc.PRECONDS.index(pc)] and w["iters"] == ITERATIONS[name][3]
        assert np.abs(p - w["p"]).max() <= ssc.P_REL * np.abs(w["p"]).max()


@pytest.mark.parametrize("name", mc.FIELDS + mc.PLATES)
def test_model_is_symmetric_positive_definite(name):
    M = mc.model(name)
    rng = np.random.default_rng(3)
    for pc in mc.PRECONDS:
        for _ in range(2):
            x, y = rng.normal(size=M.n), rng.normal(size=M.n)
            mx, my = M.apply(x, preconditioner=pc), M.apply(y, preconditioner=pc)
            assert abs(y @ mx - x @ my) <= 1e-12 * (abs(y @ mx) + np.linalg.norm(x) * np.linalg.norm(my)), pc
            assert x @ mx > 0 and y @ my > 0, pc


@pytest.mark.parametrize("name", mc.FIELDS)
def test_apply_a_is_the_vcycle_models(name):
    M, H = mc.model(name), mc.hierarchy(name)
    v = np.random.default_rng(4).normal(size=M.n)
    assert np.array_equal(M.apply_a(v), vm.apply_a(H, v))


@pytest.mark.parametrize("name", ["maze", "terraces", "plate_holed"])
def test_coarse_operators_are_the_galerkin_products(name):
    """A1 = P^T A P with A from vcycle_model.apply_a, and A2 = P1^T A1 P1. A1 couples face neighbours only, so P^T A P is read off
    27 products A (indicator of the tiles of one colour, coordinates modulo 3): no two tiles of a colour share a neighbour."""
    M, H = mc.model(name), mc.hierarchy(name)
    C = M.coarse
    A1 = M.a1_dense()
    got = np.zeros_like(A1)
    colour = (C.coords[0] % 3) + 3 * (C.coords[1] % 3) + 9 * (C.coords[2] % 3)
    nbrs = [np.arange(C.n1)] + [C.whole.lo[d] for d in range(3)] + [C.whole.up[d] for d in range(3)]
    for c in np.unique(colour):
        on = colour == c
        rows = np.bincount(C.tile, weights=vm.apply_a(H, on[C.tile].astype(np.float64)), minlength=C.n1)
        for nb in nbrs:  # row J belongs to the one tile of the colour that is J or a face neighbour of J
            J = np.flatnonzero((nb < C.n1) & np.append(on, False)[nb])
            got[J, nb[J]] = rows[J]
        quiet = np.ones(C.n1, dtype=bool)
        for nb in nbrs:
            quiet &= ~np.append(on, False)[nb]
        assert not rows[quiet].any()  # no coupling beyond the face neighbours
    tol = 1e-12 * np.abs(A1).max()
    assert np.abs(got - A1).max() <= tol
    assert np.abs(A1 - A1.T).max() == 0
    P1 = M.p1_dense()
    assert not C.regularised
    assert np.abs(P1.T @ A1 @ P1 - C.A2).max() <= tol * 64


def test_fields_hold_what_they_are_there_for():
    f = {name: mc.features(name) for name in mc.FIELDS + mc.PLATES}
    for name, (n, n1, n2) in SIZES.items():
        assert (f[name]["unknowns"], f[name]["level1"], f[name]["level2"]) == (n, n1, n2), name
    assert not any(v["regularised"] for v in f.values())
    # every designed field of vcycle_cases has an identity l1_l2 table and a level 2 of one or two unknowns; the plates do not
    assert all(f[name]["l1_l2_identity"] and f[name]["level2"] <= 2 for name in mc.FIELDS)
    assert f["plate"]["level2"] > 64 and f["plate"]["l1_l2_identity"]  # more than one workgroup's 64 blocks
    h = f["plate_holed"]
    assert h["blocks_in_grid"] == 25 and h["level2"] == 24 and not h["l1_l2_identity"]
    C = mc.model("plate_holed").coarse
    assert np.array_equal(C.blocks[:6], np.arange(6)) and C.blocks[6] == 7  # the list leaves the grid order at position 6
    assert h["level2"] > 16  # more blocks than k_coarse_all has waves
    assert h["missing_across_block_face"] >= 1
    # (an AIR cell sets no A bit, so the weight towards such a tile is 0: the assembly of A2 leaves it at `hw == 0`, before `!hu[j]`)
    assert h["full_face"] == 16 and h["partial_faces"] == 10  # the strip: faces with 4 and 12 couplings instead of 16
    # the last block along x and z holds one row of tiles
    assert (np.bincount(C.block)[[4, 23]] == [8, 1]).all() and (C.coords[0] // 8 == 4).sum() == 33
    fired = {name: v["tile_safety"][0] for name, v in f.items()}
    assert fired["maze"] == 6 and fired["maze_h17"] == 6 and fired["maze_h05"] == 6
    assert all(v == 0 for name, v in fired.items() if not name.startswith("maze"))
    assert all(v["level1_safety"][0] == 0 for v in f.values())
    smallest = min(v["level1_safety"][1] for v in f.values())
    print(f"SAFETY level 1: fires nowhere, smallest e / a_ii {smallest:.3f}")
    assert 0.40 < smallest < 0.42


@pytest.mark.parametrize("mutant", list(mm.MUTANTS))
def test_bars_discriminate_every_mutant(mutant):
    """max |M_mutant^-1 r - M^-1 r| >= 100 fp32 bars (= 800 d32) on the named field, preconditioner and right-hand side."""
    name, pc, label = SHOWN_ON[mutant]
    z, d32 = mc.reference(name, label, pc)
    err = float(np.abs(mc.model(name, mutant).apply(mc.rhs(name)[label], preconditioner=pc) - z).max())
    ratio = err / (vc.F32_BARS * d32)
    print(f"MUTANT {mutant} {name} {pc} {label} {ratio:.3g} fp32 bars")
    assert ratio >= 100.0
    if mutant == "tile_reads_across_faces":
        assert mc.features(name)["level1"] > 1


def test_every_field_sees_the_mutants_it_can():
    """A mutant that a field cannot show leaves its model exactly as it is (no_safety away from the mazes, l1_l2_identity where the
    table is the identity); every other one moves some right-hand side of the field by 100 fp32 bars."""
    for name in mc.FIELDS:
        f = mc.features(name)
        for m in mm.MUTANTS:
            best = 0.0
            for pc in mc.PRECONDS:
                for label in ("random", "b", "A_smooth", "A_tile_constant"):
                    z, d32 = mc.reference(name, label, pc)
                    err = np.abs(mc.model(name, m).apply(mc.rhs(name)[label], preconditioner=pc) - z).max()
                    best = max(best, float(err / (vc.F32_BARS * d32)))
            blind = (m == "l1_l2_identity") or (m == "no_safety" and f["tile_safety"][0] == 0) or \
                    (m in ("tile_reads_across_faces", "weights_on_minus_face") and f["couplings_across_tile_faces"] == 0)
            assert best == 0.0 if blind else best >= 100.0, (name, m, best)


@pytest.mark.parametrize("name,label", [("maze", "b"), ("droplets", "b"), ("terraces", "b"), ("plate_holed", "A_smooth")])
def test_the_order_of_the_dot_products_is_far_below_the_iterates_bar(name, label):
    """The device sums its dot products tile by tile, wave by wave; the model sums them flat. p_3 moves by less than 1 / 100 of the
    fp64 bar of tests/test_gpu_multilevel.py (1e-10 max |p_3|) when the model sums tile by tile."""
    M, b = mc.model(name), mc.rhs(name)[label]
    for pc in mc.PRECONDS:
        p, it = M.pcg(b, 3, pc)
        q, _ = M.pcg(b, 3, pc, dots_by_tile=True)
        assert it == 3
        moved = float(np.abs(p - q).max()) / (vc.F64_REL * float(np.abs(p).max()))
        print(f"DOTS {name} {pc} {moved:.2e} fp64 bars")
        assert moved < 0.01


def test_masked_plate_system_is_the_oracles():
    """vcycle_cases.plate_system_of with a fluid mask: on a 24 x 8 x 17 plate without a tile, a strip and a single cell the oracle's
    hash and build_system give the same unknowns, counts, types and A bytes."""
    size = (24, 8, 17)
    mask = mc.plate_mask(size, None, ((1, 0, 1),), (3, 2, 20))
    mask[16, 1, 23] = False
    mine = vc.plate_system_of(size, mask)
    s = orc.CpuSim(size, method=sc.APIC, blending=1.0)
    s.set_particles(mc.particles_of(mask))
    s.hash()
    assert np.array_equal(s.fluid_cells(), mine["fluid_cells"]) and np.array_equal(s.space_hash()[1], mine["counts"])
    s.p2g()
    assert np.array_equal(s.cells()["type"], mine["type"])
    s.build_system(vc.DT)
    assert np.array_equal(s.abits(), mine["abits"])
    s.close()
    w, mine = mc.system("plate_holed"), vc.plate_system_of(mc.HOLED_SIZE, mc.holed_mask())  # ... and on the holed plate itself
    for k in ("fluid_cells", "counts", "type", "abits"):
        assert np.array_equal(w[k], mine[k]), k
    assert ((w["abits"] & 7) > 0).all() and len(w["fluid_cells"]) == int(mc.holed_mask().sum())
    assert np.isfinite(w["p"]).all() and 3 < w["iters"] < 200


def test_model_says_when_the_top_level_was_regularised():
    """A box full of fluid between walls has no free surface: A, A1 and A2 are singular (A2 = [0] here), the Cholesky of
    coarse_setup fails and the diagonal gets 1e-8 trace / n + 1e-30. No designed field takes that branch (asserted above)."""
    full = np.ones((8, 8, 16), dtype=bool)
    w = vc.plate_system_of((16, 8, 8), full)
    M = mm.Model(w["size"], w["fluid_cells"], w["abits"], vc.DT)
    assert M.coarse.n1 == 2 and M.coarse.n2 == 1 and M.coarse.regularised
    assert M.coarse.A2[0, 0] == 1e-30 and np.abs(M.a1_dense().sum(axis=1)).max() == 0
