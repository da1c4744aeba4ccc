"""GPU tests (-m gpu) of the position correction's block set-up and result stores on the clouds of tests/correction_output_cases.py
- a part that owns nothing, tiles of 3 FINE_CAP / 4 particles and one more, a crowded tile for the second pass next to a normal one,
a last tile one cell wide with a particle on the max face, a tile without any neighbour, tiles of one particle - and on the dyadic
clouds of the three older case modules, fused and correct-then-collide, per particle id against the live oracle on the same inputs;
no particle is left out but the coincident pairs of close_pairs. The bar is the stage's own flat bar, correction_cases.FLAT_BAR * h,
as in tests/test_gpu_correction_halfcells.py.

Every particle's record is written exactly once: the results go back IN PLACE over the particle's key and fractions, so a record
that is not written leaves the particle at its start - tests/test_correction_output_cases.py asserts that this is worth 20 bars and
more for the particles of these clouds - and one written by two work items would have to be written with the same particle's
result twice to pass. (The output arrays are the particle arrays themselves; nothing outside the library can pre-fill them.)

Every comparison prints `MARGIN <what> <error / bar>` before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import correction_cases as cc
from tests import correction_halfcell_cases as hc
from tests import correction_output_cases as oc
from tests import correction_row_cases as rc

pytestmark = pytest.mark.gpu

MODULES = {"output": oc, "halfcells": hc, "rows": rc, "edges": cc}
# (close_pairs_odd is off the lattice and has a bar of its own in tests/test_gpu_correction_edges.py: the flat bar is not its bar)
CLOUDS = [(m, n) for m, mod in MODULES.items() for n in mod.NAMES if (m, n) != ("edges", "close_pairs_odd")]
IDS = [f"{m}-{n}" for m, n in CLOUDS]


def close(got, want, bar, what, keep):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.where(keep, np.abs(got - want).max(axis=1), 0.0)
    worst = int(err.argmax())
    print(f"MARGIN {what} {err[worst] / bar:.3f} (max |dx| {err[worst]:.3e} at particle {worst}, "
          f"{int((err >= bar).sum())} of {int(keep.sum())} beyond the bar)")
    assert err[worst] < bar, (what, worst, got[worst], want[worst])


def keep_of(cloud):
    """All particles but the coincident pairs (close_pairs: the reference pushes those apart at random)."""
    keep = np.ones(len(cloud[1]), dtype=bool)
    keep[cloud[3]["twins"]] = False
    assert (~keep).sum() <= 6
    return keep


def make_sim(cloud):
    size, parts, solid, meta = cloud
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=cc.BLEND)
    if solid is not None:
        s.set_solid_cells(solid)
    s.upload_particles(parts)
    return s


def positions(s, parts):
    out = s.download_particles(into=parts.copy(), write_positions=True)
    assert np.array_equal(out["cx"][:, 0], np.arange(len(parts)))  # upload order = id order: the comparisons are per id
    return out


@functools.lru_cache(maxsize=None)
def device_fused(module, name):
    """hash(); correct_collide(DT): (positions per id, correction_stats_ex)."""
    cloud = MODULES[module].build(name)
    s = make_sim(cloud)
    s.hash()
    s.correct_collide(cc.DT)
    stats = s.correction_stats_ex()
    out = positions(s, cloud[1])["pos"]
    s.close()
    out.setflags(write=False)
    return out, stats


@pytest.mark.parametrize("module,name", CLOUDS, ids=IDS)
def test_correct_collide(module, name):
    cloud = MODULES[module].build(name)
    out, stats = device_fused(module, name)
    close(out, MODULES[module].oracle(name)["collide"], cc.FLAT_BAR * cloud[3]["h"], f"{module} {name} correct_collide", keep_of(cloud))


@pytest.mark.parametrize("module,name", CLOUDS, ids=IDS)
def test_correct_then_collide(module, name):
    """The no-collide variant of the kernels (lfa_correct), then lfa_collide."""
    cloud = MODULES[module].build(name)
    size, parts, solid, meta = cloud
    want, bar, keep = MODULES[module].oracle(name), cc.FLAT_BAR * meta["h"], keep_of(cloud)
    s = make_sim(cloud)
    s.hash()
    s.correct(cc.DT)
    out = positions(s, parts)
    close(out["pos"], want["correct"], bar, f"{module} {name} correct", keep)
    s.collide()
    out = positions(s, parts)
    s.close()
    close(out["pos"], want["collide"], bar, f"{module} {name} correct,collide", keep)


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_tiers_take_the_parts_the_layout_predicts(name):
    """correction_stats_ex() = (parts flagged for the gather kernel, parts in all, parts flagged by the first pass for the second):
    second_pass hands the crowded tile's parts over, next to a tile that stays with the first pass; nobody else hands anything on."""
    cloud = oc.build(name)
    second, gather = hc.prediction(cloud)
    out, (to_gather, total, to_second) = device_fused("output", name)
    assert total == len(hc.layout(cloud)) == 2 * len(oc.tile_counts(cloud))
    assert (to_second, to_gather) == (len(second), len(gather))
    assert to_gather == 0 and (to_second > 0) == name.startswith("second_pass")
