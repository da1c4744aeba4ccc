"""CPU tests of tests/slab_face_cases.py: the table of (case, layer bounds) the slab tests run tests what it claims. Every class
of crossing below is a CONDITION on the inputs, counted from the oracle's own results (move_cases.oracle, transfer_cases'
contributions and hats, stencil_cases.oracle_stages) - not from a free-flight estimate, which ignores collisions -: each must be
non-empty for at least one (case, bounds). The counts are printed (pytest -s) and recorded in docs/experiments.md."""
import numpy as np
import pytest

from tests import move_cases as mc
from tests import slab_face_cases as sf
from tests import stencil_cases as sc
from tests import transfer_cases as tc

POS_BAR = 2e-5  # times h: the move stages' bar (tests/test_gpu_move_edges.py)


def test_the_table_names_existing_cases_and_bounds_that_partition_them():
    sf.check_table()
    for family in sf.FAMILIES:
        rows = sf.table(family)
        assert len(set(rows)) == len(rows)
    # every case with nz >= 16 of the three case modules is in the table (fast_*, contrast_9_8_7, thin_17_2_9 ... are thinner)
    for family, (mod, rows) in sf.FAMILIES.items():
        tall = {n for n in mod.CASES if mod.build(n)[0][2] >= 16}
        listed = {n for n, _ in rows}
        if family == "moves":  # y repeats x; tile_reach_h05 and lone_reach are tile_reach_x+ at another h / with one particle
            tall -= {"tile_reach_x-", "tile_reach_y+", "tile_reach_y-", "tile_reach_h05", "lone_reach"}
        assert tall == listed, (family, sorted(tall ^ listed))


def test_owner_stitch_and_poison():
    assert list(sf.owner(np.array([0, 7, 8, 15, 16, 17]), (0, 1, 3))) == [0, 0, 1, 1, 1, 1]
    assert list(sf.owner(np.array([0, 7, 8, 15, 16, 17]), (0, 1, 2, 3))) == [0, 0, 1, 1, 2, 2]
    assert sf.z_range((0, 1, 2, 3), 2, 17) == (16, 17) and sf.z_range((0, 2, 3), 0, 18) == (0, 16)
    assert sf.faces((0, 1, 2, 3)) == [8, 16] and sf.faces((0, 2)) == []
    size, bounds = (2, 3, 17), (0, 1, 2, 3)
    nc = 2 * 3 * 17
    per_rank = [np.full((nc, 3), float(r)) for r in range(3)]
    got = sf.stitch(per_rank, bounds, size).reshape(17, 3, 2, 3)
    assert (got[:8] == 0).all() and (got[8:16] == 1).all() and (got[16:] == 2).all()
    from libfluid_amd.scenes import CELL_DTYPE
    cells = np.zeros(nc, dtype=CELL_DTYPE)
    cells["vel"] = 1.5
    cells["type"] = sc.FLUID
    cells["type"][::5] = sc.SOLID
    out = sf.poison_outside(cells, bounds, 1, ("vel", "type"), size)
    own = sf.own_mask(bounds, 1, size)
    assert own.sum() == 8 * 6 and np.array_equal(out[own], cells[own])
    assert np.isnan(out["vel"][~own]).all()
    solid = cells["type"] == sc.SOLID
    assert (out["type"][~own & solid] == sc.SOLID).all() and (out["type"][~own & ~solid] == sf.POISON_TYPE).all()
    assert (cells["vel"] == 1.5).all()  # the input is left alone
    only_vel = sf.poison_outside(cells, bounds, 1, ("vel",), size)
    assert np.array_equal(only_vel["type"], cells["type"])


class _Handle:
    def __init__(self):
        self.closed = False

    def close(self):
        self.closed = True


def test_run_ranks_collects_errors_and_closes_what_it_ran():
    sims, hub = [_Handle() for _ in range(3)], _Handle()
    res, errors = sf.run_ranks(sims, lambda r, s: 10 * r, timeout=5, hub=hub)
    assert res == [0, 10, 20] and not errors and all(s.closed for s in sims) and hub.closed

    def fails_on_one(r, s):
        if r == 1:
            raise ValueError("rank 1")
        return r

    sims = [_Handle() for _ in range(3)]
    with pytest.raises(AssertionError):
        sf.run_ranks(sims, fails_on_one, timeout=5)
    assert all(s.closed for s in sims)
    sims = [_Handle() for _ in range(3)]
    res, errors = sf.run_ranks(sims, fails_on_one, timeout=5, raise_errors=False)
    assert res == [0, None, 2] and [r for r, _ in errors] == [1] and isinstance(errors[0][1], ValueError)


MOVE_CLASSES = ("up_one", "down_one", "skin_start_crosses_deflected", "ends_in_first_layer", "ends_in_last_layer",
                "ranks_ending_empty", "ranks_starting_empty", "far")


def test_moves_cross_slab_faces_in_every_way():
    """End owner one above / one below the start owner; a start within `skin` of a slab face that ends on the other side after a
    bounce or a push-out; ends in the first and in the last cell layer of a slab; a rank that ends empty, one that starts empty; and
    the far set - end owner two or more ranks from the start owner -, which is exactly slab_face_cases.FAR_MOVES."""
    total = dict.fromkeys(MOVE_CLASSES, 0)
    far = {}
    for name, bounds in sf.table("moves"):
        c = sf.move_counts(name, bounds)
        print(f"COVER moves {name} {sf.bounds_id(bounds)} " + " ".join(f"{k}={c[k]}" for k in MOVE_CLASSES))
        for k in MOVE_CLASSES:
            total[k] += c[k]
        if c["far"]:
            far[(name, bounds)] = c["far"]
            assert np.array_equal(sf.far_movers(name, bounds), np.flatnonzero(np.abs(np.subtract(*sf.move_owners(name, bounds)[:2])) >= 2))
    print("COVER moves total " + " ".join(f"{k}={total[k]}" for k in MOVE_CLASSES))
    for k in MOVE_CLASSES:
        assert total[k] > 0, k
    assert far == sf.FAR_MOVES
    # a split at z+ gives both kinds of empty rank
    c = sf.move_counts("tile_reach_z+", (0, 1, 3))
    assert c["ranks_starting_empty"] == 1 and c["ranks_ending_empty"] == 1 and c["up_one"] == len(mc.build("tile_reach_z+")[1])
    # the deflected crossers come from both kinds of case the issue names or from tile_reach's plate: say which
    for name in ("obstacles", "axis_aligned"):
        best = max(sf.move_counts(n, b)["skin_start_crosses_deflected"] for n, b in sf.table("moves") if n == name)
        print(f"COVER moves {name} skin_start_crosses_deflected (best bounds) {best}")


def test_no_end_position_is_within_the_bar_of_a_slab_face():
    """Who owns a particle at the end is decided by its end cell. The device's end lies within 2e-5 h of the oracle's, so an oracle
    end closer than that to a slab face would leave the owner open - unless it lies ON the face because the particle never moved
    in z (axis_aligned: exact on both sides)."""
    for name, bounds in sf.table("moves"):
        size, parts, solid, meta = mc.build(name)
        z0 = mc.cells_of(parts["pos"], meta)[:, 2]
        z1 = mc.cells_of(mc.oracle(name)["collide"], meta)[:, 2]
        gap = np.min([np.abs(z1 - f) for f in sf.faces(bounds)], axis=0)
        on = gap == 0.0
        assert (z0[on] == z1[on]).all(), name
        print(f"COVER moves {name} {sf.bounds_id(bounds)} smallest_gap_to_a_face {gap[~on].min():.3e} cells, exactly_on_a_face {int(on.sum())}")
        assert gap[~on].min() > 5 * POS_BAR, (name, bounds, gap[~on].min())


TRANSFER_CLASSES = ("u_up", "u_down", "v_up", "v_down", "w_up", "w_down", "into_empty_tile_up", "into_empty_tile_down",
                    "kept_up", "kept_down", "zeroed_up", "zeroed_down", "hat_into_empty_tile")


def test_transfers_cross_slab_faces_in_both_directions():
    """(particle, face) contributions whose face another rank stores, upwards and downwards per component; lone hats across a face,
    kept and zeroed, in each direction; hats whose face lies across the face in a tile that holds no particle. No w contribution
    crosses upwards in any cloud: the w face at z + 1 is stored in cell z and is the topmost w face a particle of cell z reaches -
    that class is asserted EMPTY."""
    total = dict.fromkeys(TRANSFER_CLASSES, 0)
    lone_up = lone_down = False
    for name, bounds in sf.table("transfers"):
        for method in tc.build(name)[3]["methods"]:
            c = sf.transfer_counts(name, method, bounds)
            print(f"COVER transfers {name} {tc.method_id(method)} {sf.bounds_id(bounds)} " + " ".join(f"{k}={c[k]}" for k in TRANSFER_CLASSES))
            for k in TRANSFER_CLASSES:
                total[k] += c[k]
            if name.startswith("lone_hats"):  # a lone particle's contribution: not one term of a sum of hundreds
                lone_up |= c["u_up"] + c["v_up"] > 0
                lone_down |= c["u_down"] + c["v_down"] + c["w_down"] > 0
    print("COVER transfers total " + " ".join(f"{k}={total[k]}" for k in TRANSFER_CLASSES))
    assert total["w_up"] == 0
    for k in TRANSFER_CLASSES:
        assert k == "w_up" or total[k] > 0, k
    assert lone_up and lone_down


@pytest.mark.parametrize("name", [n for n, _ in sf.TRANSFERS if "zmirror" in n or "above" in n])
def test_reflected_and_one_sided_hats_keep_their_weights(name):
    """What test_transfer_cases.py asserts of the three original lone_hats clouds, for the clouds derived from them: the particles are
    isolated, every hat's face carries its target weight to a per cent, and the oracle zeroes exactly the faces below the threshold."""
    size, parts, solid, meta = tc.build(name)
    nx, ny, nz = size
    cells = np.floor((parts["pos"] - np.array(meta["off"])) / meta["h"])
    d = np.abs(cells[:, None, :] - cells[None, :, :]).max(axis=2)
    assert d[~np.eye(len(parts), dtype=bool)].min() >= 3
    assert len(meta["hats"]) == len(parts)
    for method in meta["methods"]:
        sw = tc.face_weight_sums(size, parts, meta["h"], meta["off"], method)
        vel = tc.oracle_stages(name, method)["p2g_vel"]
        for hat in meta["hats"]:
            x, y, z = hat["cell"]
            raw = x + nx * (y + ny * z)
            assert abs(sw[raw, hat["comp"]] - hat["target"]) <= 0.01 * hat["target"], hat
            assert (vel[raw, hat["comp"]] != 0.0) == hat["kept"], hat
    if "above" in name:  # one side of z = 8 holds nothing
        zc = cells[:, 2]
        assert (zc >= 8).all() or (zc < 8).all()
        assert len(sf.hats_across(name, (0, 1, 2))) >= 3


STENCIL_CLASSES = ("a_couplings", "apply_faces_second_pressure_across", "sweep1_from_across", "sweep2_from_sweep1_across")


def test_grid_stages_reach_across_slab_faces():
    """Matrix couplings across a slab face; pressure-gradient faces whose second pressure belongs to the rank above; cells that
    the first extrapolation sweep makes valid from an unknown across the face, and cells the second sweep makes valid from a cell
    that the first sweep made valid across the face (the validity bytes that travel between two sweeps)."""
    total = dict.fromkeys(STENCIL_CLASSES, 0)
    for name, bounds in sf.table("stencils"):
        c = sf.stencil_counts(name, bounds)
        print(f"COVER stencils {name} {sf.bounds_id(bounds)} " + " ".join(f"{k}={c[k]}" for k in STENCIL_CLASSES))
        for k in STENCIL_CLASSES:
            total[k] += c[k]
        if name == "maze":
            assert all(c[k] > 0 for k in STENCIL_CLASSES), (bounds, c)
    print("COVER stencils total " + " ".join(f"{k}={total[k]}" for k in STENCIL_CLASSES))
    for k in STENCIL_CLASSES:
        assert total[k] > 0, k


def test_two_sweeps_of_the_oracle_are_the_restatements():
    """slab_face_cases.oracle_extrapolation(name, 2): stencil_cases records 1 and 3 sweeps only; the restatement that names each written
    component (stencil_cases.extrapolate_sweeps) is the oracle bit for bit at 2 as it is at 1 and 3."""
    for name in ("maze", "sheets"):
        size = sc.build(name)[0]
        want = sc.oracle_stages(name, True)
        ref = sc.extrapolate_sweeps(size, want["type"], want["fluid_cells"], want["apply_vel"], 2)[0]
        assert np.array_equal(ref, sf.oracle_extrapolation(name, 2))
        assert not np.array_equal(ref, want["extrap1_vel"])
        # (maze is so dense that the second sweep reaches every cell; the sheets leave cells for a third)
        assert np.array_equal(ref, want["extrap3_vel"]) == (name == "maze")
