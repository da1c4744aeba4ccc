"""GPU tests (-m gpu) of the position correction on the clouds of tests/correction_halfcell_cases.py - pairs at the edge of reach and
two half cells apart, across tile faces, on integral products of the half-cell arithmetic, on the grid's max face, block rows
with one record in an outer half cell, a crowded tile for the second pass and the gather kernel - per particle id against the live
oracle on the same inputs; no particle is left out. The bar is the stage's own flat bar, correction_cases.FLAT_BAR * h, as in
tests/test_gpu_correction_rows.py: the inputs are exact in fp32, and a partner the walk misses is worth thousands of bars
(tests/test_correction_halfcell_cases.py). The tests look at results only, not at the layout of the index.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import correction_cases as cc
from tests import correction_halfcell_cases as hc

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
    cloud = hc.build(name)
    s = make_sim(cloud)
    s.hash()
    s.correct_collide(cc.DT)
    stats = s.correction_stats_ex()
    out = positions(s, cloud[1])["pos"]
    s.close()
    out.setflags(write=False)
    return out, stats


@pytest.mark.parametrize("name", hc.NAMES)
def test_correct_collide(name):
    size, parts, solid, meta = hc.build(name)
    out, stats = device_fused(name)
    close(out, hc.oracle(name)["collide"], cc.FLAT_BAR * meta["h"], f"{name} correct_collide")


@pytest.mark.parametrize("name", hc.NAMES)
def test_the_tiers_take_the_parts_the_layout_predicts(name):
    """correction_stats_ex() = (parts flagged for the gather kernel, parts in all, parts flagged by the first pass for the second):
    crowded hands two parts to the second pass, which hands one of them on to the gather kernel."""
    second, gather = hc.prediction(hc.build(name))
    out, (to_gather, total, to_second) = device_fused(name)
    assert total == len(hc.layout(hc.build(name)))
    assert (to_second, to_gather) == (len(second), len(gather)) == ((2, 1) if name == "crowded" else (0, 0))


@pytest.mark.parametrize("name", hc.NAMES)
def test_correct_then_collide(name):
    """The no-collide variant of the kernels (lfa_correct), then lfa_collide."""
    cloud = hc.build(name)
    size, parts, solid, meta = cloud
    want, bar = hc.oracle(name), cc.FLAT_BAR * meta["h"]
    s = make_sim(cloud)
    s.hash()
    s.correct(cc.DT)
    out = positions(s, parts)
    close(out["pos"], want["correct"], bar, f"{name} correct")
    s.collide()
    out = positions(s, parts)
    s.close()
    close(out["pos"], want["collide"], bar, f"{name} correct,collide")
