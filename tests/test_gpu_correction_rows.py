"""GPU tests (-m gpu) of the position correction's staging and epilogue (k_correct_fine<CAP, ONLY>: a slot's row from the rows'
first slots, the per-row descriptors, the short cut of interior tiles in open water) on the clouds of
tests/correction_row_cases.py, per particle id against the live oracle on the same inputs; no particle is left out. The bar is the
stage's own flat bar, correction_cases.FLAT_BAR * h: the inputs are dyadic, so what remains is the fp32 arithmetic of the force,
and a record staged from the wrong row, decoded with the wrong row's first cell or missing from the own list is worth at least
100 bars (tests/test_correction_row_cases.py).

Every comparison prints `MARGIN <what> <error / bar>` before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import correction_cases as cc
from tests import correction_row_cases as rc

pytestmark = pytest.mark.gpu


def close(got, want, bar, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want).max(axis=1)
    worst = int(err.argmax())
    print(f"MARGIN {what} {err[worst] / bar:.3f} (max |dx| {err[worst]:.3e} at particle {worst}, "
          f"{int((err >= bar).sum())} of {len(err)} beyond the bar)")
    assert err[worst] < bar, (what, worst, got[worst], want[worst])


def make_sim(cloud):
    size, parts, solid, meta = cloud
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=cc.BLEND)
    s.upload_particles(parts)
    return s


def positions(s, parts):
    out = s.download_particles(into=parts.copy(), write_positions=True)
    assert np.array_equal(out["cx"][:, 0], np.arange(len(parts)))  # upload order = id order: the comparisons are per id
    return out


@functools.lru_cache(maxsize=None)
def device_fused(name):
    """hash(); correct_collide(DT): (positions per id, correction_stats_ex)."""
    cloud = rc.build(name)
    s = make_sim(cloud)
    s.hash()
    s.correct_collide(cc.DT)
    stats = s.correction_stats_ex()
    out = positions(s, cloud[1])["pos"]
    s.close()
    out.setflags(write=False)
    return out, stats


@pytest.mark.parametrize("name", rc.NAMES)
def test_correct_collide(name):
    size, parts, solid, meta = rc.build(name)
    out, stats = device_fused(name)
    close(out, rc.oracle(name)["collide"], cc.FLAT_BAR * meta["h"], f"{name} correct_collide")


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_tiers_take_the_parts_the_layout_predicts(name):
    """correction_stats_ex() = (parts flagged for the gather kernel, parts in all, parts flagged by the first pass for the second):
    long_rows hands one part to the second pass, every other cloud stays with the first."""
    second, gather = rc.prediction(rc.build(name))
    out, (to_gather, total, to_second) = device_fused(name)
    assert total == len(rc.layout(rc.build(name)))
    assert (to_second, to_gather) == (len(second), len(gather)) == ((1, 0) if name == "long_rows" else (0, 0))


@pytest.mark.parametrize("name", rc.NAMES)
def test_correct_then_collide(name):
    cloud = rc.build(name)
    size, parts, solid, meta = cloud
    want, bar = rc.oracle(name), cc.FLAT_BAR * meta["h"]
    s = make_sim(cloud)
    s.hash()
    s.correct(cc.DT)
    out = positions(s, parts)
    close(out["pos"], want["correct"], bar, f"{name} correct")
    close(out["old_pos"], parts["pos"], 1e-6 * meta["h"], f"{name} old_position")
    s.collide()
    out = positions(s, parts)
    s.close()
    close(out["pos"], want["collide"], bar, f"{name} correct,collide")


@pytest.mark.parametrize("name", rc.ISOLATED)
def test_full_time_step(name):
    """One lfa_time_step (the correction on its second stream beside the solve) against the oracle's own time_step."""
    cloud = rc.build(name)
    size, parts, solid, meta = cloud
    s = make_sim(cloud)
    res, it, rc_ = s.time_step(cc.DT)
    out = positions(s, parts)
    s.close()
    assert rc_ >= 0
    close(out["pos"], rc.oracle_time_step(name), cc.FLAT_BAR * meta["h"], f"{name} time_step")
