"""GPU tests (-m gpu) of the transfer kernels on the adversarial clouds of tests/transfer_cases.py: P2G (LDS-binned and
global-atomic scatter, finalize) and G2P (tile kernel, leaver kernel) against the live oracle on the same inputs, at the bars of
tests/test_gpu_parity.py. tests/test_transfer_cases.py pins the oracle to the reference on these very inputs and asserts that no
face lies near the reference's weight threshold, so every face and every particle is compared - nothing is masked out.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts (pytest -s shows them; docs/experiments.md records them).
"""
import functools

import numpy as np
import pytest

import libfluid_amd as lfa
from oracle import loader as orc
from tests import transfer_cases as tc
from tests import util
from tests.test_gpu_parity import VEL_REL, cells_from

pytestmark = pytest.mark.gpu

DT_CORR = 0.1  # a position correction that moves particles by up to a cell (tests/test_next_rows.py)
C_REL = 5e-5  # APIC C after G2P (tests/test_gpu_parity.py: test_apply_pressure_extrapolate_g2p)
VARIANTS = [lfa.P2G_LDS_BINNED, lfa.P2G_GLOBAL_ATOMIC]
VARIANT_ID = {lfa.P2G_LDS_BINNED: "binned", lfa.P2G_GLOBAL_ATOMIC: "atomic"}
CASE_METHODS = tc.case_methods()
IDS = [f"{n}-{tc.method_id(m)}" for n, m in CASE_METHODS]


def close(a, b, rel, what):
    """util.assert_close at the max-norm bar `rel`, the margin printed first."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    err = float(np.abs(a - b).max()) if a.shape == b.shape and a.size else 0.0
    print(f"MARGIN {what} {err / (rel * scale):.3f}")
    util.assert_close(a, b, rel, what)


def g2p_bar(method):
    return VEL_REL * (2 if method == tc.FLIP else 1)


def c_of(parts):
    return np.concatenate([parts["cx"], parts["cy"], parts["cz"]], axis=1)


def make_sim(cloud, method, **extra):
    size, parts, solid, meta = cloud
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=method, blending=tc.BLEND[method], **extra)
    if solid is not None:
        s.set_solid_cells(solid)
    s.upload_particles(parts)
    return s


def run_p2g(cloud, method, variant):
    """hash, p2g, add_gravity on the device; everything the P2G tests compare."""
    s = make_sim(cloud, method, p2g_variant=variant)
    out = {}
    s.hash()
    out["fluid_cells"], out["counts"] = s.fluid_cells(), s.cell_counts()
    s.p2g()
    cells = s.cells()
    out["p2g_vel"], out["p2g_type"] = cells["vel"].copy(), cells["type"].copy()
    if method == tc.FLIP:
        out["old_vel"] = s.old_cells()["vel"].copy()
    s.add_gravity(tc.DT)
    out["grav_vel"] = s.cells()["vel"].copy()
    out["deferred"] = s.solver_stats()["p2g_deferred_scatters"]
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def device_p2g(name, method, variant):
    return run_p2g(tc.build(name), method, variant)


def check_p2g(got, want, method, label):
    assert np.array_equal(got["fluid_cells"], want["fluid_cells"]), label
    assert np.array_equal(got["counts"], want["counts"]), label
    assert np.array_equal(got["p2g_type"], want["p2g_type"]), label
    close(got["p2g_vel"], want["p2g_vel"], VEL_REL, f"{label} p2g_vel")
    if method == tc.FLIP:
        close(got["old_vel"], want["old_vel"], VEL_REL, f"{label} flip_old_grid")
    close(got["grav_vel"], want["grav_vel"], VEL_REL, f"{label} grav_vel")


@pytest.mark.parametrize("variant", VARIANTS, ids=[VARIANT_ID[v] for v in VARIANTS])
@pytest.mark.parametrize("name,method", CASE_METHODS, ids=IDS)
def test_p2g_on_adversarial_clouds(name, method, variant):
    """Cell counts, fluid cells and types exact, face velocities after the P2G (FLIP: and the old grid) and after gravity at VEL_REL
    against the oracle, and the two scatter variants against each other at the same bar. lone_hats: a face whose only weight is
    5e-7 or 2e-7 is exactly 0, one at 2e-6 or 5e-6 carries the particle's own w v / w."""
    size, parts, solid, meta = tc.build(name)
    label = f"{name} {VARIANT_ID[variant]} {tc.method_id(method)}"
    got, want = device_p2g(name, method, variant), tc.oracle_stages(name, method)
    check_p2g(got, want, method, label)
    # (after a first binning the LDS-binned scatter reads v, C through the binning's source index; the global-atomic one never does)
    assert got["deferred"] == (1 if variant == lfa.P2G_LDS_BINNED else 0)
    other = device_p2g(name, method, VARIANTS[1 - VARIANTS.index(variant)])
    assert np.array_equal(got["p2g_type"], other["p2g_type"])
    close(got["p2g_vel"], other["p2g_vel"], VEL_REL, f"{label} p2g_vel_vs_other_variant")
    if "hats" in meta:
        nx, ny, nz = size
        for hat in meta["hats"]:
            x, y, z = hat["cell"]
            comp, p = hat["comp"], parts[hat["index"]]
            face = got["p2g_vel"][x + nx * (y + ny * z), comp]
            if not hat["kept"]:
                assert face == 0.0, (label, hat, face)
                continue
            own = p["vel"][comp]
            if method == tc.APIC:
                stag = np.full(3, 0.5)
                stag[comp] = 1.0
                own = own + p[("cx", "cy", "cz")[comp]] @ (np.array(meta["off"]) + (np.array(hat["cell"]) + stag) * meta["h"] - p["pos"])
            bar = VEL_REL * np.linalg.norm(p["vel"])
            print(f"MARGIN {label} lone_hat_{hat['target']:g} {abs(face - own) / bar:.3f}")
            assert abs(face - own) <= bar, (label, hat, face, own)


@pytest.mark.parametrize("seq", ["hash,hash", "hash,correct,hash", "hash,download"])
@pytest.mark.parametrize("method", tc.ALL_METHODS, ids=tc.method_id)
@pytest.mark.parametrize("name", ["tile_counts_deferred", "contrast_21_13_18", "contrast_9_8_7"])
def test_p2g_with_a_deferred_binning(name, method, seq):
    """The LDS-binned scatter reads v and C through the source index of the binning (`from`, one and two rounds ahead in its
    pipeline) whenever a binning is still deferred, and in place once something has completed it. "hash,hash" and
    "hash,correct,hash" leave it deferred - the counter of such scatters says so -, "hash,download" does not: the in-place path,
    which the plain hash - p2g sequence of every other test never takes. The oracle is given the device's own downloaded particles
    (the position correction has moved them; the device reports cell + fp32 fraction, exact in fp64 at cell_size 1)."""
    cloud = tc.build(name)
    size, parts, solid, meta = cloud
    assert meta["h"] == 1.0
    s = make_sim(cloud, method, p2g_variant=lfa.P2G_LDS_BINNED)
    s.hash()
    now = parts
    if seq == "hash,correct,hash":
        s.correct_collide(1e-3)
        now = s.download_particles(write_positions=True)  # (completes the first binning; the second one defers again)
        assert not np.array_equal(now["pos"], parts["pos"])
        s.hash()
    elif seq == "hash,hash":
        s.hash()
    else:
        s.download_particles(write_positions=True)  # completes the binning
    got = {"fluid_cells": s.fluid_cells(), "counts": s.cell_counts()}
    before = s.solver_stats()["p2g_deferred_scatters"]
    s.p2g()
    assert s.solver_stats()["p2g_deferred_scatters"] - before == (0 if seq == "hash,download" else 1)
    cells = s.cells()
    got["p2g_vel"], got["p2g_type"] = cells["vel"].copy(), cells["type"].copy()
    if method == tc.FLIP:
        got["old_vel"] = s.old_cells()["vel"].copy()
    s.add_gravity(tc.DT)
    got["grav_vel"] = s.cells()["vel"].copy()
    # nothing was lost on the way: every particle still has its own v and C
    after = s.download_particles()
    s.close()
    assert np.array_equal(after["vel"], now["vel"].astype(np.float32)) and np.array_equal(c_of(after), c_of(now).astype(np.float32))
    want = tc.staged_cloud((size, now, solid, meta), method) if seq == "hash,correct,hash" else tc.oracle_stages(name, method)
    check_p2g(got, want, method, f"{name} {seq} {tc.method_id(method)}")


@pytest.mark.parametrize("name,method", CASE_METHODS, ids=IDS)
def test_g2p_on_adversarial_clouds(name, method):
    """The G2P stage alone from the oracle's extrapolated grid (FLIP: the old grid is the device's own P2G's): v and C per particle,
    and the CFL figure - its max |v|^2 rides in the kernel, guarded by `> 0`."""
    cloud = tc.build(name)
    size, parts, solid, meta = cloud
    want = tc.oracle_stages(name, method)
    label = f"{name} g2p {tc.method_id(method)}"
    s = make_sim(cloud, method)
    s.hash()
    if method == tc.FLIP:
        s.p2g()
        close(s.old_cells()["vel"], want["old_vel"], VEL_REL, f"{label} flip_old_grid")
    s.upload_cells(cells_from(want["extrap_vel"], want["extrap_type"]))
    s.g2p()
    cfl = s.cfl()
    out = s.download_particles(into=parts.copy())
    s.close()
    close(out["vel"], want["g2p_vel"], g2p_bar(method), f"{label} g2p_vel")
    if method == tc.APIC:
        close(c_of(out), want["g2p_c"], C_REL, f"{label} g2p_c")
    else:  # PIC and FLIP carry C through unchanged
        assert np.array_equal(c_of(out).astype(np.float32), c_of(parts).astype(np.float32))
    assert np.isfinite(want["cfl"]) and abs(cfl - want["cfl"]) <= 1e-4 * want["cfl"], (label, cfl, want["cfl"])


@pytest.mark.parametrize("method", tc.ALL_METHODS, ids=tc.method_id)
def test_stale_order_g2p_with_more_leavers_than_the_tile_list_holds(method):
    """A G2P on the order of the last binning after the position correction has moved the particles: a tile lists up to
    G2P_LV_CAP = 256 leavers in LDS and reserves that many slots of the global list with one atomic; further ones go to the global
    list one by one. 32 particles per cell make the correction push more than 256 out of each tile of the crowded block; a tile with
    64 particles loses a few, one with three lone particles none. Expected values: the oracle's G2P of the device's downloaded
    positions on the device's own grid; and, as before, a handle that binned again before its G2P."""
    cloud = tc.crowded_tiles()
    size, parts, solid, meta = cloud
    outs = {}
    for rebin in (False, True):
        s = make_sim(cloud, method)
        s.hash(); s.p2g(); s.add_gravity(tc.DT)
        s.solve(tc.DT); s.apply_pressure(tc.DT)
        s.correct_collide(DT_CORR)
        s.extrapolate()
        if rebin:
            s.hash()
        else:
            grid = s.cells()
        s.g2p()
        cfl = s.cfl()
        outs[rebin] = s.download_particles(into=parts.copy(), write_positions=True)  # upload order
        if not rebin:
            cfl_stale = cfl
        s.close()
    got = outs[False]
    # leavers per tile of the binning, counted on the host from the cells the device reports
    top = np.asarray(size) - 1
    t0 = np.minimum(np.floor(parts["pos"]).astype(np.int64), top) // 8
    t1 = np.minimum(np.floor(got["pos"]).astype(np.int64), top) // 8
    left = (t0 != t1).any(axis=1)
    key = t0[:, 0] + 5 * (t0[:, 1] + 3 * t0[:, 2])
    lost = {int(k): int(left[key == k].sum()) for k in np.unique(key)}
    print("leavers per tile:", lost)
    assert any(n > 256 for n in lost.values()), lost
    assert any(1 <= n <= 255 for n in lost.values()), lost
    assert any(n == 0 for n in lost.values()), lost
    # the oracle: old grid (FLIP) from its own P2G of the particles as uploaded, then the moved particles with the velocities
    # they had before the G2P (nothing but the G2P writes them), on the device's extrapolated grid
    o = orc.CpuSim(size, method=method, blending=tc.BLEND[method])
    o.set_particles(parts)
    o.hash(); o.p2g()
    moved = parts.copy()
    moved["pos"] = got["pos"]
    o.set_particles(moved)
    o.set_cells(grid)
    o.g2p()
    want = o.particles()  # (no hash since: the order of `moved`)
    want_cfl = o.cfl()
    o.close()
    assert np.array_equal(want["pos"], got["pos"])
    label = f"crowded_tiles stale_g2p {tc.method_id(method)}"
    close(got["vel"], want["vel"], g2p_bar(method), f"{label} g2p_vel")
    close(got["vel"][left], want["vel"][left], g2p_bar(method), f"{label} g2p_vel_leavers")
    if method == tc.APIC:
        close(c_of(got), c_of(want), C_REL, f"{label} g2p_c")
        close(c_of(got)[left], c_of(want)[left], C_REL, f"{label} g2p_c_leavers")
    assert abs(cfl_stale - want_cfl) <= 1e-4 * want_cfl, (cfl_stale, want_cfl)
    assert np.abs(got["vel"] - parts["vel"]).max() > 1e-2 * np.abs(got["vel"]).max()  # the transfer did change velocities
    # the cross-check of test_g2p_on_the_order_of_the_last_binning_equals_g2p_after_rebinning, on this cloud
    b = outs[True]
    assert np.abs(got["pos"] - b["pos"]).max() < 1e-5
    for f in ("vel", "cx", "cy", "cz") if method == tc.APIC else ("vel",):
        assert np.abs(got[f] - b[f]).max() < 2e-4 * np.abs(got[f]).max(), f


FIX_LIMIT = 2.0 ** 15  # |w (v + c . (face - p))| of one contribution, LDS-binned scatter (include/libfluid_amd.h, lfa_p2g)


@functools.lru_cache(maxsize=None)
def fast_cloud_at_the_limit():
    unit = tc.fast(1.0)
    m1 = tc.max_single_wv(unit[0], unit[1], method=tc.APIC)
    cloud = tc.fast(0.9 * FIX_LIMIT / m1)
    return cloud, {m: tc.staged_cloud(cloud, m) for m in tc.ALL_METHODS}


@pytest.mark.parametrize("variant", VARIANTS, ids=[VARIANT_ID[v] for v in VARIANTS])
@pytest.mark.parametrize("method", tc.ALL_METHODS, ids=tc.method_id)
def test_p2g_near_the_fixed_point_range(method, variant):
    """The LDS-binned scatter converts every contribution w (v + c . (face - p)) to 64-bit fixed point with a conversion that is
    valid below 2^15 (world units of one step). The largest contribution of this cloud is 0.9 * 2^15 - computed on the host and
    asserted -: the in-range side of the limit holds the usual bar. Nothing beyond the limit is run."""
    cloud, oracle = fast_cloud_at_the_limit()
    size, parts, solid, meta = cloud
    m = tc.max_single_wv(size, parts, method=tc.APIC)
    assert abs(m - 0.9 * FIX_LIMIT) <= 1e-9 * FIX_LIMIT and m < FIX_LIMIT
    assert tc.max_single_wv(size, parts, method=method) <= m
    got = run_p2g(cloud, method, variant)
    check_p2g(got, oracle[method], method, f"fast_at_0.9_of_the_limit {VARIANT_ID[variant]} {tc.method_id(method)}")
