"""CPU tests of tests/stencil_cases.py: the oracle is the reference on exactly these cell fields, stage by stage (without that a
device-against-oracle comparison on them proves nothing), every field is well-posed, and every field holds what it claims to hold -
asserted from the oracle's own output, never from the device's."""
import os

import numpy as np
import pytest

from oracle import loader as orc
from tests import stencil_cases as sc
from tests import util
from tests.golden import make_golden_stencil as gen

needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference sources on this machine)")
REL = 1e-12  # oracle against reference, floating-point fields (measured: 3.4e-13 on p, 5e-15 on the grids)


def staged(name, kind):
    """hash, P2G, gravity; build_system (abits, b, the apply_a probe sin(0.37 i) + 0.25); solve; apply_pressure; the extrapolation
    with 1 and with 3 sweeps from the same applied grid - on the oracle (computed once, shared) or the compiled reference."""
    return sc.oracle_stages(name) if kind == "oracle" else sc.staged(name, kind)


def same(got, want, label):
    assert set(got) == set(want), (label, sorted(set(got) ^ set(want)))
    for k in sorted(want):
        w, g = np.asarray(want[k]), np.asarray(got[k])
        if w.dtype.kind in "iu":
            assert np.array_equal(g, w), f"{label}:{k} differs"
        elif k == "residual":  # an entry of r at the converging iteration: its scale is the right-hand side's
            assert abs(float(g) - float(w)) <= REL * np.abs(want["b"]).max(), f"{label}:{k}"
        else:
            util.assert_close(g, w, REL, f"{label}:{k}", atol=1e-300)


@needs_ref
@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_is_the_reference_on_the_stencil_cases(name):
    same(staged(name, "oracle"), staged(name, "ref"), name)


@needs_ref
@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_is_the_reference_from_fp32_rounded_grids(name):
    """The run the GPU tests compare with: every stage from the fp32-rounded grid of the stage before it. Rounding moves no
    iteration count."""
    same(sc.oracle_stages(name, True), sc.staged(name, "ref", True), name + " rounded")
    assert sc.oracle_stages(name, True)["iters"] == sc.oracle_stages(name)["iters"]


@pytest.fixture(scope="module")
def golden():
    return util.load_golden("stencil_stages")


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_matches_the_golden_reference_vectors(name, golden):
    got = staged(name, "oracle")
    for f in ("fluid_cells", "abits", "iters"):
        assert np.array_equal(got[f], golden[f"{name}.{f}"]), (name, f)
    util.assert_close(got["p"], golden[f"{name}.p"], REL, f"{name}:p")


def test_golden_file_is_small_and_complete(golden):
    assert set(golden) == {f"{n}.{f}" for n in sc.NAMES for f in gen.FIELDS}
    assert os.path.getsize(gen.PATH) < 200 * 1024


@needs_ref
def test_golden_file_is_reproduced_byte_for_byte(tmp_path):
    again = str(tmp_path / "stencil_stages.npz")
    gen.save(again, gen.arrays())
    with open(again, "rb") as a, open(gen.PATH, "rb") as b:
        assert a.read() == b.read()


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_case_is_well_posed(name, golden):
    """Conditions on the inputs, asserted: no unknown without a non-solid neighbour (an empty matrix row), and the REFERENCE's own
    solve (golden file; the live reference too where it is built) is finite and converges - no pocket of fluid sealed off from the
    air, where the reference returns NaN."""
    assert ((golden[f"{name}.abits"] & 7) > 0).all()
    assert np.isfinite(golden[f"{name}.p"]).all() and np.abs(golden[f"{name}.p"]).max() > 0
    assert 0 < int(golden[f"{name}.iters"]) < 200
    for kind in ("oracle", "ref") if orc.have_ref() else ("oracle",):
        st = staged(name, kind)
        assert np.isfinite(st["p"]).all() and st["residual"] < 1e-6 and 0 < st["iters"] < 200, (name, kind)
        for k in ("grav_vel", "b", "Aprobe", "apply_vel", "extrap1_vel", "extrap3_vel"):
            assert np.isfinite(st[k]).all(), (name, kind, k)


def faces(name, rounded=False):
    size, parts, solid, meta = sc.build(name)
    st = sc.oracle_stages(name, rounded)
    return st, sc.apply_pressure_faces(size, st["type"], st["fluid_cells"], st["grav_vel"], st["p"], sc.coeff_of(meta))


@pytest.mark.parametrize("rounded", [False, True], ids=["fp64", "fp32_inputs"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_numpy_restatements_are_the_oracle_and_every_face_class_occurs(name, rounded):
    """The fp64 numpy restatements of apply_pressure and of the extrapolation (they tell the GPU tests which rule applied to which
    face) reproduce the oracle bit for bit; and the faces of the case fall into ALL of k_apply_pressure's classes."""
    size, parts, solid, meta = sc.build(name)
    st, (vel, cls, scale) = faces(name, rounded)
    assert np.array_equal(vel, st["apply_exact"])
    for k in sc.FACE_CLASSES:
        assert cls[k].any(), (name, k)
    untouched = ~np.any([cls[k] for k in sc.FACE_CLASSES], axis=0)
    assert untouched.any() and np.array_equal(vel[untouched], st["grav_vel"][untouched])
    zero = cls["unknown-solid"] | cls["unknown-outside"] | cls["solid-unknown"]
    assert not vel[zero].any() and st["grav_vel"][zero].any()  # (they were not zero before)
    for sweeps in (1, 3):
        out, written, count, born, unit = sc.extrapolate_sweeps(size, st["type"], st["fluid_cells"], st["apply_vel"], sweeps)
        assert np.array_equal(out, st[f"extrap{sweeps}_vel"])
        assert np.array_equal(out[~written], st["apply_vel"][~written]) and (~written[born > 0]).any()
        # a component is written only where the +d neighbour is valid AND of the cell's own type: in the first sweep that is an empty
        # solid cell below a solid cell that holds particles (the maze has them), from the second on air below air that is valid
        # by then (everywhere but in the two grids that are full to the top layer, where the first sweep reaches every cell)
        if name.startswith("maze") or (sweeps == 3 and name not in ("thin_8_8_8", "thin_9_8_8")):
            assert written.any(), (name, sweeps)


def test_extrapolation_covers_every_neighbour_count_and_later_sweeps():
    """Cells with 1 to 6 valid neighbours, and cells made valid only in sweep 2 and only in sweep 3 (in the maze all of that at once)."""
    seen, late = set(), set()
    for name in sc.NAMES:
        size, parts, solid, meta = sc.build(name)
        st = sc.oracle_stages(name)
        _, written, count, born, _ = sc.extrapolate_sweeps(size, st["type"], st["fluid_cells"], st["apply_vel"], 3)
        here = set(np.unique(count[born > 0]).tolist())
        if name == "maze":
            assert here == {1, 2, 3, 4, 5, 6} and (born == 2).any() and (born == 3).any()
        if name in ("droplets", "sheets", "walls_x", "walls_y", "walls_z"):
            assert (born == 2).any() and (born == 3).any() and (born == -1).any(), name  # (and cells no sweep reaches)
        seen |= here
        late |= set(np.unique(born).tolist())
    assert seen == {1, 2, 3, 4, 5, 6} and {0, 1, 2, 3} <= late


def test_maze_has_unknowns_that_are_solid_cells():
    for name in ("maze", "maze_h17", "maze_h05"):
        size, parts, solid, meta = sc.build(name)
        st = sc.oracle_stages(name)
        t = st["type"][st["fluid_cells"].astype(np.int64)]
        assert (t == sc.SOLID).sum() >= 100 and (t == sc.FLUID).sum() >= 1000
        assert set(np.unique(t)) == {sc.FLUID, sc.SOLID}
        assert any(s % 8 for s in size)
        x, y, z = meta["doorway"]
        assert st["type"][x + size[0] * (y + size[1] * z)] != sc.SOLID
    a, b = sc.build("maze"), sc.build("maze_h17")
    assert np.array_equal(sc.oracle_stages("maze")["fluid_cells"], sc.oracle_stages("maze_h17")["fluid_cells"])
    assert np.array_equal(sc.oracle_stages("maze")["fluid_cells"], sc.oracle_stages("maze_h05")["fluid_cells"])
    assert b[3]["h"] == 1.7 and b[3]["rho"] == 2.0 and any(b[3]["off"]) and sc.build("maze_h05")[3]["h"] == 0.5


def test_droplets_hold_the_tiles_and_droplets_they_promise():
    size, parts, solid, meta = sc.build("droplets")
    st = sc.oracle_stages("droplets")
    nx, ny, nz = size
    fc = st["fluid_cells"].astype(np.int64)
    per_tile = sc.unknowns_per_tile(size, fc)
    coupled = sc.couplings_across_tile_faces(size, st["type"], fc, st["abits"])
    assert per_tile[meta["tile64"]] == sc.CLOSED_MAX and meta["tile64"] not in coupled
    assert per_tile[meta["tile65"]] == sc.CLOSED_MAX + 1 and meta["tile65"] not in coupled
    g = meta["groups"]
    assert sum(len(v) for v in g.values()) == len(fc)  # every listed cell is an unknown, none twice
    raw = {k: np.array([x + nx * (y + ny * z) for x, y, z in v]) for k, v in g.items()}
    assert all(np.isin(r, fc).all() for r in raw.values())
    # the pairs across a tile face couple two tiles; the singles in cell 7 of a tile couple nothing
    for d, k in enumerate(("straddle_x", "straddle_y", "straddle_z")):
        (a, b) = g[k]
        assert a[d] % 8 == 7 and b[d] == a[d] + 1
        assert tuple(np.array(a) // 8) in coupled and tuple(np.array(b) // 8) in coupled
    assert (0, 1, 0) not in coupled and per_tile[(0, 1, 0)] == 5
    assert any(c[0] % 8 == 7 for c in g["cell7"]) and any(c[2] % 8 == 7 for c in g["cell7"])
    walls = np.array(g["walls"] + g["corner"])
    assert (walls[:, 0] == 0).any() and (walls[:, 2] == 0).any() and g["corner"][0] == (nx - 1, ny - 1, nz - 1)
    for a in range(3):
        assert (walls[:, a] == size[a] - 1).any()
    assert st["type"][raw["in_solid"][0]] == sc.SOLID and st["type"][raw["on_solid"]].tolist() == [sc.FLUID, sc.FLUID]
    # the pool keeps the PCG busy; the droplets' pressures are not all zero
    where = {k: np.searchsorted(fc, r) for k, r in raw.items()}
    assert all(np.abs(st["p"][w]).max() > 0 for w in where.values())


def test_sheets_thin_grids_and_walls_are_what_they_claim():
    size, parts, solid, meta = sc.build("sheets")
    st = sc.oracle_stages("sheets")
    nx, ny, nz = size
    fc = st["fluid_cells"].astype(np.int64)
    c = np.stack([fc % nx, (fc // nx) % ny, fc // (nx * ny)], axis=1)
    for a in range(3):
        assert size[a] % 8 and (c[:, a] == 7).sum() > 20 and (c[:, a] == 8).sum() > 15 and (c[:, a] == size[a] - 1).sum() > 20
        line = {tuple(t) for t in c // 8}
        assert len({t[a] for t in line}) == -(-size[a] // 8)
    assert [sc.build(n)[0] for n in sc.NAMES if n.startswith("thin")] == [(2, 9, 17), (17, 2, 9), (5, 5, 5), (8, 8, 8), (9, 8, 8)]
    for name in ("thin_8_8_8", "thin_9_8_8"):
        size, parts, solid, meta = sc.build(name)
        n = len(sc.oracle_stages(name)["fluid_cells"])
        assert n == size[0] * (size[1] - 1) * size[2] - 2  # wall to wall below the top layer, but for a bubble and a solid cell
    for axis, name in enumerate(("walls_x", "walls_y", "walls_z")):
        size, parts, solid, meta = sc.build(name)
        st = sc.oracle_stages(name)
        assert size[axis] == 40 and sorted(size) == [9, 10, 40]
        fc = st["fluid_cells"].astype(np.int64)
        c = np.stack([fc % size[0], (fc // size[0]) % size[1], fc // (size[0] * size[1])], axis=1)
        tiles = {tuple(t) for t in c // 8}
        assert meta["block_tile"] not in tiles and meta["far_tile"] not in tiles
        assert not any(max(abs(t[a] - meta["far_tile"][a]) for a in range(3)) <= 1 for t in tiles)  # outside the dilated tile set
        lo = np.array(meta["block_tile"]) * 8
        t3 = st["type"].reshape(size[2], size[1], size[0])
        assert (t3[lo[2]:lo[2] + 8, lo[1]:lo[1] + 8, lo[0]:lo[0] + 8] == sc.SOLID).all()
        assert (c[:, axis] == 7).any() and (c[:, axis] == 16).any()  # flush against both of its sides
        far = np.array(meta["far_tile"]) * 8
        assert (t3[far[2]:far[2] + 8, far[1]:far[1] + 8, far[0]:far[0] + 8] == sc.SOLID).sum() >= 3


def test_retyped_has_unknowns_typed_air_beside_unknowns():
    """What tells "the neighbour is an unknown" from "the neighbour is fluid" on the non-solid side: faces from an unknown up into
    an unknown of type AIR, whose pressure is NOT zero and must not be used (src/pressure_solver.cpp:73-148 takes 0 there)."""
    size, parts, solid, meta = sc.build("retyped")
    st, (vel, cls, scale) = faces("retyped")
    fc = st["fluid_cells"].astype(np.int64)
    edit = meta["retype_air"]
    assert len(edit) == 8 and np.isin(edit, fc).all()
    assert (st["p2g_type"][edit] == sc.FLUID).all() and (st["type"][edit] == sc.AIR).all()
    assert set(np.unique(st["type"][fc])) == {sc.AIR, sc.FLUID}
    p_cell = np.zeros(len(st["type"]))
    p_cell[fc] = st["p"]
    assert p_cell[edit].all() and (np.abs(p_cell[edit]) > 1e-2 * np.abs(st["p"]).max()).sum() >= 6
    stride = (1, size[0], size[0] * size[1])
    n_faces = 0
    for d in range(3):
        below = edit - stride[d]
        coord = (edit // stride[d]) % size[d]
        ok = (coord > 0) & np.isin(below, fc)
        n_faces += int(cls["unknown-air"][below[ok], d].sum())
    assert n_faces >= 6
