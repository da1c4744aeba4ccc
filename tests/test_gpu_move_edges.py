"""GPU tests (-m gpu) of the move and collide kernels (k_advect_collide, k_advect_collide_count, k_collide_only) on the adversarial
moves of tests/move_cases.py, per particle id against the live oracle on the same inputs, no particle left out. The bar is the one
these stages have had all along (tests/test_next_rows.py: positions are cell + fp32 fraction on the device, 2^-23 of a cell, plus
the fp32 velocity in x += v dt): 2e-5 h. Every defect the cases aim at - a skipped push-out, a missed or extra bounce, a NaN that
wins a comparison - moves a particle by at least 0.02 cells. tests/test_move_cases.py pins the oracle to the reference on these
very inputs and shows that the cases hold what they are there for.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import move_cases as mc

pytestmark = pytest.mark.gpu

POS_BAR = 2e-5  # times h


def close(got, want, h, what, bar=POS_BAR):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want).max(axis=1)
    worst = int(err.argmax())
    print(f"MARGIN {what} {err[worst] / (bar * h):.3f} (max |dx| {err[worst] / h:.3e} cells at particle {worst}, "
          f"{int((err >= bar * h).sum())} of {len(err)} beyond the bar)")
    assert err[worst] < bar * h, (what, worst, got[worst], want[worst])


def make_sim(cloud, source=None):
    size, parts, solid, meta = cloud
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=mc.BLEND)
    if solid is not None:
        s.set_solid_cells(solid)
    if source is not None:
        s.add_source(source[0], source[1], 2, True, True)
    s.upload_particles(parts)
    return s


def positions(s, parts):
    return s.download_particles(into=parts.copy(), write_positions=True)  # upload order = id order


@functools.lru_cache(maxsize=None)
def device_fused(name):
    cloud = mc.build(name)
    s = make_sim(cloud)
    s.advect_collide(cloud[3]["dt"])
    out = positions(s, cloud[1])
    s.close()
    return out


@pytest.mark.parametrize("name", mc.NAMES)
def test_fused_advect_collide(name):
    size, parts, solid, meta = mc.build(name)
    out = device_fused(name)
    close(out["pos"], mc.oracle(name)["collide"], meta["h"], f"{name} advect_collide")
    assert np.array_equal(out["pos"], out["old_pos"])


@pytest.mark.parametrize("name", mc.NAMES)
def test_split_advect_then_collide(name):
    """lfa_advect leaves the moved, clamped position and the start as old_position; lfa_collide then ends where the fused stage
    ends."""
    cloud = mc.build(name)
    size, parts, solid, meta = cloud
    want = mc.oracle(name)
    s = make_sim(cloud)
    s.advect(meta["dt"])
    out = positions(s, parts)
    close(out["pos"], want["advect"], meta["h"], f"{name} advect")
    close(out["old_pos"], parts["pos"], meta["h"], f"{name} old_position", bar=1e-6)
    s.collide()
    out = positions(s, parts)
    s.close()
    close(out["pos"], want["collide"], meta["h"], f"{name} advect,collide")
    close(out["pos"], device_fused(name)["pos"], meta["h"], f"{name} split_vs_fused")
    assert np.array_equal(out["pos"], out["old_pos"])


@pytest.mark.parametrize("name", mc.ISOLATED)
def test_full_time_step(name):
    """One lfa_time_step - the way into k_advect_collide_count, whose waves take 8 x 64 particles behind an `i < n` guard
    (n = 1, 64, 511, 513 here; tests/test_gpu_binning_edges.py::test_time_step_counts_while_it_advects goes the same way with waves
    of 512 distinct tiles and n around 2 048) - against the oracle's own time_step from the same state. The particles are at least 2 cells apart
    before and after the move, so the position correction moves none of them and the later stages add nothing to a position: the
    bar stays at 2e-5 h."""
    cloud = mc.build(name)
    size, parts, solid, meta = cloud
    s = make_sim(cloud)
    res, it, rc = s.time_step(meta["dt"])
    out = positions(s, parts)
    s.close()
    assert rc >= 0
    close(out["pos"], mc.oracle_time_step(name), meta["h"], f"{name} time_step")


def test_fused_advect_collide_with_a_coercing_source():
    """k_advect_collide<true>: half of the start cells of tile_reach(x, +) belong to a coercing source whose velocity is the 7.98
    move; the coerced particles take the short cut's rule into the plate's skin."""
    cloud, source = mc.coerce_source()
    size, parts, solid, meta = cloud
    want = mc.run_cpu(cloud, "oracle", source)
    s = make_sim(cloud, source)
    s.advect_collide(meta["dt"])
    out = positions(s, parts)
    s.close()
    close(out["pos"], want["collide"], meta["h"], "tile_reach_x+ coerced advect_collide")
    assert np.array_equal(out["vel"], want["vel"])
    taken = (want["vel"] == np.asarray(source[1])).all(axis=1)
    assert 20 <= taken.sum() <= len(parts) - 20
    assert not out["cx"][taken].any() and np.array_equal(out["cx"][~taken], parts["cx"][~taken])
