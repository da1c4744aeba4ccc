"""GPU tests (-m gpu) of the position correction (k_build_fine_index, k_correct_fine<CAP, ONLY>, k_correct_collide) on the
adversarial clouds of tests/correction_cases.py, per particle id against the live oracle on the same inputs. No particle is left
out but the coincident pairs of close_pairs (meta["twins"]: the reference pushes those apart at random), whose number is fixed by
construction. The bar is the one this stage has had all along (tests/test_next_rows.py): 5e-5 h. The inputs are dyadic, every
pair offset is formed without rounding on the device, and a missed or mis-decoded partner is worth at least 100 bars
(tests/test_correction_cases.py), so a deviation is a logic error. close_pairs_odd alone is off the lattice and is held to
correction_cases.bound(), derived per particle from the rounding of the staged coordinates.

Every comparison prints `MARGIN <what> <error / bar>` before it asserts (pytest -s shows them)."""
import functools
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import correction_cases as cc
from tests.test_correction_cases import cap_edge_prediction

pytestmark = pytest.mark.gpu

METHODS = {"flip": lfa.FLIP_BLEND, "apic": lfa.APIC, "pic": lfa.PIC}


def bar_of(name):
    """The flat bar (world units), or the per-particle bound of close_pairs_odd."""
    return cc.bound(name) if name == "close_pairs_odd" else cc.FLAT_BAR * cc.build(name)[3]["h"]


def close(got, want, bar, what, keep=None):
    """max over the particles `keep` (default: all) of |got - want| / bar; bar in world units, a number or one per particle."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    keep = np.ones(len(got), dtype=bool) if keep is None else keep
    ratio = np.where(keep, np.abs(got - want).max(axis=1) / bar, 0.0)
    worst = int(ratio.argmax())
    print(f"MARGIN {what} {ratio[worst]:.3f} (max |dx| / bar at particle {worst}: |dx| = {np.abs(got - want)[worst].max():.3e}, "
          f"{int((ratio >= 1.0).sum())} of {int(keep.sum())} beyond the bar)")
    assert ratio[worst] < 1.0, (what, worst, got[worst], want[worst])


def keep_of(name):
    size, parts, solid, meta = cc.build(name)
    keep = np.ones(len(parts), dtype=bool)
    keep[meta["twins"]] = False
    assert (~keep).sum() == (6 if name == "close_pairs" else 0)
    return keep


def make_sim(cloud, method=lfa.FLIP_BLEND):
    size, parts, solid, meta = cloud
    s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=method, blending=cc.BLEND)
    if solid is not None:
        s.set_solid_cells(solid)
    s.upload_particles(parts)
    return s


def positions(s, parts):
    out = s.download_particles(into=parts.copy(), write_positions=True)
    assert np.array_equal(out["cx"][:, 0], np.arange(len(parts)))  # upload order = id order: the comparisons are per id
    return out


def check_twins(name, out, want):
    """The coincident pairs: finite, pushed apart, and - the hashed push is a unit-box vector times corr - within corr sqrt 3 of
    the oracle, which leaves the pair's own force out."""
    size, parts, solid, meta = cc.build(name)
    twins = meta["twins"]
    if not len(twins):
        return
    h = meta["h"]
    assert np.isfinite(out[twins]).all()
    apart = np.abs(out[twins[0::2]] - out[twins[1::2]]).max(axis=1)
    off = np.sqrt(((out[twins] - want[twins]) ** 2).sum(axis=1))
    limit = (cc.CORR * np.sqrt(3.0) + cc.FLAT_BAR) * h
    print(f"MARGIN {name} twins_apart {1e-4 * h / apart.min():.3f} (the closest end {apart.min():.3e} apart)")
    print(f"MARGIN {name} twins_near_the_oracle {off.max() / limit:.3f}")
    assert (apart > 1e-4 * h).all() and (off < limit).all()


@functools.lru_cache(maxsize=None)
def device_fused(name):
    """hash(); correct_collide(DT): (positions per id, correction_stats_ex)."""
    cloud = cc.build(name)
    s = make_sim(cloud)
    s.hash()
    s.correct_collide(cc.DT)
    stats = s.correction_stats_ex()
    out = positions(s, cloud[1])["pos"]
    s.close()
    out.setflags(write=False)
    return out, stats


@pytest.mark.parametrize("name", cc.NAMES)
def test_correct_collide(name):
    size, parts, solid, meta = cc.build(name)
    out, stats = device_fused(name)
    want = cc.oracle(name)["collide"]
    close(out, want, bar_of(name), f"{name} correct_collide", keep_of(name))
    check_twins(name, out, want)
    if name != "cap_edge":
        assert stats[0] == 0 and stats[2] == 0  # nothing but the first pass ran


def test_cap_edge_hands_over_exactly_the_parts_the_model_predicts():
    """correction_stats_ex() = (parts flagged by the second pass for the gather kernel, parts in all, parts flagged by the first
    pass for the second): a part that stages FINE_CAP stays with the first pass, FINE_CAP + 1 goes to the second, FINE_CAP_BIG
    stays there, FINE_CAP_BIG + 1 goes on to the gather kernel."""
    second, gather = cap_edge_prediction()
    out, (to_gather, total, to_second) = device_fused("cap_edge")
    assert total == 2 * 6  # two parts of each of the six tiles with particles
    assert (to_second, to_gather) == (len(second), len(gather)) == (3, 1)


@pytest.mark.parametrize("name", cc.NAMES)
def test_correct_then_collide(name):
    """lfa_correct leaves the moved, clamped position and the start as old_position (the oracle's _correct_positions alone);
    lfa_collide then ends where the fused stage ends."""
    cloud = cc.build(name)
    size, parts, solid, meta = cloud
    want, keep, bar = cc.oracle(name), keep_of(name), bar_of(name)
    s = make_sim(cloud)
    s.hash()
    s.correct(cc.DT)
    out = positions(s, parts)
    close(out["pos"], want["correct"], bar, f"{name} correct", keep)
    close(out["old_pos"], parts["pos"], 1e-6 * meta["h"], f"{name} old_position")
    check_twins(name, out["pos"], want["correct"])
    s.collide()
    out = positions(s, parts)
    s.close()
    close(out["pos"], want["collide"], bar, f"{name} correct,collide", keep)


@pytest.mark.parametrize("name", ["faces", "solids", "lone_dense_tile"])
def test_correct_collide_begin_end(name):
    """The correction on the second stream, grid-only stages beside it."""
    cloud = cc.build(name)
    s = make_sim(cloud)
    s.hash()
    s.p2g()
    s.correct_collide_begin(cc.DT)
    s.add_gravity(cc.DT)
    s.correct_collide_end()
    out = positions(s, cloud[1])
    s.close()
    close(out["pos"], cc.oracle(name)["collide"], bar_of(name), f"{name} correct_collide_begin,_end")


@pytest.mark.parametrize("seq", ["hash,p2g", "hash,hash", "hash,download", "hash,correct,hash"])
@pytest.mark.parametrize("name", ["faces", "solids", "lone_dense_tile"])
def test_correct_collide_after_a_p2g_and_with_a_deferred_binning(name, seq):
    """"hash,hash" and "hash,correct,hash" leave a binning deferred, "hash,download" completes it, "hash,p2g" has read v and C
    through it. After "hash,correct,hash" the oracle starts from the device's own downloaded particles (cell + fp32 fraction,
    exact in fp64 at cell_size 1); they are off the lattice then, by partners at 2^-4 cells and more: the rounding of the staged
    coordinates is worth corr (k / d + |k'|) sqrt 3 2^-20 <= 1e-5 cells, inside the bar."""
    cloud = cc.build(name)
    size, parts, solid, meta = cloud
    assert meta["h"] == 1.0
    s = make_sim(cloud)
    s.hash()
    want = None
    if seq == "hash,p2g":
        s.p2g()
    elif seq == "hash,hash":
        s.hash()
    elif seq == "hash,download":
        s.download_particles(write_positions=True)
    else:
        s.correct_collide(1e-3)
        now = positions(s, parts)
        assert not np.array_equal(now["pos"], parts["pos"])
        want = cc.run_cpu((size, now, solid, meta))["collide"]
        s.hash()
    s.correct_collide(cc.DT)
    out = positions(s, parts)
    s.close()
    close(out["pos"], cc.oracle(name)["collide"] if want is None else want, bar_of(name), f"{name} {seq},correct_collide")


@pytest.mark.parametrize("seq", ["hash", "hash,download"])
@pytest.mark.parametrize("method", ["apic", "pic"])
@pytest.mark.parametrize("name", ["faces", "lone_dense_tile"])
def test_correct_collide_with_apic_and_pic(name, method, seq):
    """The correction keeps its cell-ordered records in arrays that are free at that point: which ones depends on the method and
    on whether the binning is still deferred."""
    cloud = cc.build(name)
    s = make_sim(cloud, METHODS[method])
    s.hash()
    if seq == "hash,download":
        s.download_particles(write_positions=True)
    s.correct_collide(cc.DT)
    out = positions(s, cloud[1])
    s.close()
    close(out["pos"], cc.oracle(name)["collide"], bar_of(name), f"{name} {method} {seq},correct_collide")
    for f in ("vel", "cx", "cy", "cz"):  # and nothing it borrowed is missing afterwards
        assert np.array_equal(out[f].astype(np.float32), cloud[1][f].astype(np.float32)), f


@pytest.mark.parametrize("bounds", [[0, 1, 3], [0, 1, 2, 3]], ids=["2slabs", "3slabs"])
@pytest.mark.parametrize("name", ["faces", "triads", "solids"])
def test_correct_collide_on_virtual_slabs(name, bounds):
    """z = 24: three tile layers. A dumbbell across z = 8 or 16 has its partner only as a ghost record behind the live ones; the
    union of the ranks' particles per id - those the push has moved across a slab face included - against the same oracle."""
    cloud = cc.build(name)
    size, parts, solid, meta = cloud
    want = cc.oracle(name)["collide"]
    n = len(bounds) - 1
    hub = lfa.LocalHub(n)
    sims = []
    for r in range(n):
        s = lfa.Sim(size, cell_size=meta["h"], offset=meta["off"], method=lfa.FLIP_BLEND, blending=cc.BLEND)
        if solid is not None:
            s.set_solid_cells(solid)
        s.init_local_slab(hub.h, r, bounds)
        s.upload_particles(parts)  # (every rank is handed the whole set and keeps what lies in its layers)
        sims.append(s)
    errors = []

    def worker(r):
        try:
            sims[r].hash()
            sims[r].correct_collide(cc.DT)
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), "slab threads hung"
    got, ids, rank = [], [], []
    for r, s in enumerate(sims):
        got.append(s.download_particles())
        ids.append(s.particle_ids())
        rank.append(np.full(len(got[-1]), r))
    for s in sims:
        s.close()
    hub.close()
    got, ids, rank = np.concatenate(got), np.concatenate(ids).astype(np.int64), np.concatenate(rank)
    assert np.array_equal(np.sort(ids), np.arange(len(parts))), "a particle was lost or is resident on two ranks"
    assert np.array_equal(got["cx"][:, 0], ids.astype(np.float64))
    out = np.empty((len(parts), 3))
    out[ids] = got["pos"]
    close(out, want, bar_of(name), f"{name} slabs {bounds} correct_collide")
    # who owns what: the slab of the start and the slab of the end
    edges = 8.0 * np.asarray(bounds[1:-1])
    home = np.searchsorted(edges, cc.cells_of(parts["pos"], meta)[:, 2], side="right")
    end = np.searchsorted(edges, cc.cells_of(want, meta)[:, 2], side="right")
    owner = np.empty(len(parts), dtype=np.int64)
    owner[ids] = rank
    i, j = meta["pairs"].T
    print(f"{name} slabs {bounds}: {int((home != end).sum())} particles change slab, "
          f"{int((home[i] != home[j]).sum())} designed pairs straddle a slab face")
    assert np.array_equal(owner, end)  # every particle is resident where it ended: the migrants have been handed over
    if name == "solids":  # (a dumbbell ACROSS a face pushes its ends away from it: only here does the push carry particles over)
        assert (home != end).any(), "the case is meant to push particles across a slab face"
    else:  # partners across a slab face: the other end is a ghost record
        assert (home[i] != home[j]).sum() >= 2 * (n - 1)
