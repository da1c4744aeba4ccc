"""lfa_seed_box / lfa_seed_sphere with LFA_SEED_COLLECTIVE on virtual slabs (N handles on one GPU, in-process transport) against
tests/seed_model.py: every rank keeps the model's particles whose clamped cell lies in its tile layers, byte for byte and in order,
numbered by their index in the single-domain list. tests/test_seed_slab_cases.py checks on the CPU that the scenes reach the ranks
they are meant to reach.

The seeding calls are made one rank after the other on the test's own thread: they send no message, so none waits for another.
The collectives (hash_particles, time_step) run on one host thread per rank, as in tests/test_gpu_slabs.py."""
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import seed_model as sm
from tests import seed_slab_cases as sc
from tests import util

pytestmark = pytest.mark.gpu


def collective(sims, fn):
    """fn(rank, sim) on one thread per rank; the results in rank order."""
    out, errors = [None] * len(sims), []

    def worker(r):
        try:
            out[r] = fn(r, sims[r])
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(len(sims))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), "slab threads hung"
    return out


def make_slabs(grid, bounds, **kw):
    hub = lfa.LocalHub(len(bounds) - 1)
    sims = [lfa.Sim(**grid, **kw) for _ in bounds[1:]]
    for r, s in enumerate(sims):
        s.init_local_slab(hub.h, r, bounds)
    return hub, sims


def close_all(hub, sims):
    for s in sims:
        s.close()
    hub.close()


def seed(sim, call, state, vel=sc.VEL, flags=lfa.SEED_COLLECTIVE, **kw):
    kind, a, b, density, ltr = call
    fn = sim.seed_box if kind == "box" else sim.seed_sphere
    return fn(a, b, velocity=vel, density=density, rng_state=state, flags=flags | (lfa.SEED_DRAW_LTR if ltr else 0), **kw)


def single_domain(grid, calls, vel=sc.VEL, flags=0, **kw):
    """A single-domain handle seeded by the same calls: (handle, state after)."""
    sim, state = lfa.Sim(**grid, **kw), sm.initial_state()
    for call in calls:
        _, state, _ = seed(sim, call, state, vel=vel, flags=flags)
    return sim, state


def gather(sims):
    """The ranks' downloads, concatenated and ordered by id: (records, ids). The handles must be binned."""
    parts = [s.download_particles(write_positions=True) for s in sims]
    ids = np.concatenate([s.particle_ids() for s in sims])
    order = np.argsort(ids, kind="stable")
    return np.concatenate(parts)[order], ids[order]


def check_partition(grid, calls, bounds):
    """What test 1 asks of a sequence of calls on the slabs `bounds`."""
    want = sc.model(sc.key(grid), tuple(calls))
    hub, sims = make_slabs(grid, bounds)
    state, first, resident = sm.initial_state(), 0, [0] * len(sims)
    for call, (pos, state_after, n_cand) in zip(calls, want):
        own = sc.owner(grid, pos, bounds)
        for r, s in enumerate(sims):
            mine = pos[own == r]
            n, got_state, got = seed(s, call, state, positions=True)
            assert n == len(mine), (call, r, n, len(mine))
            assert got.tobytes() == mine.tobytes(), (call, r)
            assert got_state == state_after, (call, r)
            assert s.seed_last() == (n_cand, len(pos), first), (call, r)
            resident[r] += n
            assert s.num_particles == resident[r], (call, r)  # (an upload would report the whole set)
        state, first = state_after, first + len(pos)
    collective(sims, lambda r, s: s.hash())
    assert [s.num_particles for s in sims] == resident
    got, ids = gather(sims)
    close_all(hub, sims)
    assert np.array_equal(ids, np.arange(first, dtype=np.uint32))  # unique, and exactly 0 .. total - 1
    one, one_state = single_domain(grid, calls)
    ref = one.download_particles(write_positions=True)
    one.close()
    assert one_state == state and len(ref) == first
    assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("bounds", sc.BOUNDS, ids=str)
@pytest.mark.parametrize("name", list(sc.PARTITION_CASES))
def test_partition_is_bit_exact(name, bounds):
    grid, calls = sc.PARTITION_CASES[name]
    check_partition(grid, calls, bounds)


@pytest.mark.parametrize("bounds", sc.BOUNDS, ids=str)
def test_appending_carries_the_numbering(bounds):
    """The testbed's scene 2: the box's ids start at the sphere's job-wide total on every rank (seed_last()[2] in check_partition),
    also on a rank that kept nothing of the sphere."""
    check_partition(sc.GRID, sc.APPEND_CALLS, bounds)


def test_a_rank_that_keeps_nothing_stays_usable():
    bounds = [0, 1, 3]
    (pos, state_after, n_cand), = sc.model(sc.key(sc.GRID), sc.LOW_CALLS)
    hub, sims = make_slabs(sc.GRID, bounds)
    kept = []
    for s in sims:
        n, state, got = seed(s, sc.LOW_CALLS[0], sm.initial_state(), positions=True)
        assert state == state_after and s.seed_last() == (n_cand, len(pos), 0)
        kept.append(n)
        assert len(got) == n
    assert kept == [len(pos), 0] and sims[1].num_particles == 0
    collective(sims, lambda r, s: s.hash())
    for _ in range(2):
        rcs = collective(sims, lambda r, s: s.time_step(util.DT)[2])
        assert all(rc >= 0 for rc in rcs)
    assert sum(s.num_particles for s in sims) == len(pos)
    # and the numbering went on with the job's on the rank that kept nothing
    for s in sims:
        n, _, _ = seed(s, sc.LOW_CALLS[0], state_after)
        assert s.seed_last()[2] == len(pos)
    close_all(hub, sims)


def test_both_scan_forms():
    """307 200 candidates on 3 slabs: 4 800 counts per scan, several tiles of its one-workgroup form (the small grids: one)."""
    check_partition(sc.BIG, sc.BIG_CALLS, [0, 1, 2, 3])


def run_steps(method, bounds, steps=8):
    """STEP_BOX seeded collectively (bounds = None: on a single domain), then `steps` time steps. Returns the handles (binned or
    stale, as the last step leaves them), the hub and the per-rank counts before / after."""
    kw = dict(method=method, blending=0.95, precond=lfa.PRECOND_MIC0_TILED, pcg_dtype=lfa.PCG_F64)
    if bounds is None:
        hub, sims = None, [lfa.Sim(**sc.STEP_GRID, **kw)]
    else:
        hub, sims = make_slabs(sc.STEP_GRID, bounds, **kw)
    for s in sims:
        seed(s, sc.STEP_BOX, sm.initial_state(), vel=sc.STEP_VEL)
    before = [s.num_particles for s in sims]

    def step(r, s):
        for _ in range(steps):
            assert s.time_step(util.DT)[2] == 0

    collective(sims, step)
    return hub, sims, before, [s.num_particles for s in sims]


def by_id(sims):
    if len(sims) == 1:
        return sims[0].download_particles(write_positions=True)  # single domain: record i is particle i
    return gather(sims)[0]


@pytest.mark.parametrize("name", ["apic", "flip"])
def test_steps_on_seeded_slabs(name):
    """The trajectories of collectively seeded particles, compared by id with the single domain's as
    test_virtual_slabs_full_time_step_with_migration compares them. FLIP: C lives in its home array, indexed by the job-wide id."""
    method = lfa.APIC if name == "apic" else lfa.FLIP_BLEND
    _, one, _, _ = run_steps(method, None)
    p1 = by_id(one)
    one[0].close()
    hub, sims, before, after = run_steps(method, sc.STEP_BOUNDS[name])
    pn = by_id(sims)
    close_all(hub, sims)
    assert len(pn) == len(p1) == sum(before)
    assert before != after, "the scene is meant to push particles across a slab face"
    dpos = np.abs(pn["pos"] - p1["pos"]).max()
    print("max position difference", dpos)
    assert dpos < 2e-3, dpos
    util.assert_close(pn["vel"], p1["vel"], 1e-2, "particle velocities after full steps, seeded slabs vs single domain",
                      atol=1e-3 * 981.0 * util.DT)
    for k in ("cx", "cy", "cz"):
        assert np.isfinite(pn[k]).all()
    if name == "flip":  # FLIP never changes C: what the seeding zeroed is still zero, whichever rank the particle is on now
        assert not pn["cx"].any() and not pn["cy"].any() and not pn["cz"].any()


def test_seeding_again_after_the_steps():
    """Binned, migrated records (holes where particles left, arrivals behind): a collective sphere is appended behind them."""
    (dam, state, _), = sc.model(sc.key(sc.STEP_GRID), (sc.STEP_BOX,))
    (want, want_state, n_cand), = sc.model(sc.key(sc.STEP_GRID), (sc.STEP_SPHERE,), state)
    bounds = sc.STEP_BOUNDS["apic"]
    own = sc.owner(sc.STEP_GRID, want, bounds)
    _, one, _, _ = run_steps(lfa.APIC, None)
    hub, sims, before, after = run_steps(lfa.APIC, bounds)
    assert before != after
    n1, state1, _ = seed(one[0], sc.STEP_SPHERE, state, flags=0)
    assert (n1, state1) == (len(want), want_state) and one[0].seed_last() == (n_cand, len(want), len(dam))
    for r, s in enumerate(sims):
        n, got_state, got = seed(s, sc.STEP_SPHERE, state, positions=True)
        assert got.tobytes() == want[own == r].tobytes() and got_state == want_state
        assert s.seed_last() == (n_cand, len(want), len(dam))  # the new ids continue the job's numbering
        assert s.num_particles == after[r] + n
    assert sum(s.num_particles for s in sims) == one[0].num_particles == len(dam) + len(want)
    collective(sims, lambda r, s: s.hash())
    got, ids = gather(sims)
    assert np.array_equal(ids, np.arange(len(dam) + len(want), dtype=np.uint32))
    bound = sc.STEP_GRID["cell_size"] * 2.0 ** -23
    assert np.abs(got["pos"][len(dam):] - want).max() <= bound
    ref = one[0].download_particles(write_positions=True)
    assert np.abs(ref["pos"][len(dam):] - want).max() <= bound
    assert np.array_equal(got["vel"][len(dam):], ref["vel"][len(dam):])
    # the resident particles were carried through the append untouched: still the single domain's trajectories
    assert np.abs(got["pos"][:len(dam)] - ref["pos"][:len(dam)]).max() < 2e-3
    rcs = collective(sims, lambda r, s: s.time_step(util.DT)[2])
    assert all(rc >= 0 for rc in rcs)
    assert one[0].time_step(util.DT)[2] >= 0
    assert sum(s.num_particles for s in sims) == one[0].num_particles == len(dam) + len(want)
    one[0].close()
    close_all(hub, sims)


def test_the_flag_on_a_single_domain_changes_nothing():
    calls = sc.APPEND_CALLS
    a, state_a = single_domain(sc.GRID, calls)
    b, state_b = single_domain(sc.GRID, calls, flags=lfa.SEED_COLLECTIVE)
    assert state_a == state_b and a.seed_last() == b.seed_last() and a.num_particles == b.num_particles > 0
    assert a.download_particles(write_positions=True).tobytes() == b.download_particles(write_positions=True).tobytes()
    want = sc.model(sc.key(sc.GRID), calls)
    assert a.seed_last() == (want[1][2], len(want[1][0]), len(want[0][0]))  # on a single domain [1] is n_seeded
    a.close()
    b.close()


def test_short_positions_buffer_on_one_rank():
    bounds = [0, 1, 3]
    (sphere, state, _), = sc.model(sc.key(sc.GRID), (sc.APPEND_CALLS[0],))
    (box, state_after, n_cand), = sc.model(sc.key(sc.GRID), (sc.APPEND_CALLS[1],), state)
    mine = box[sc.owner(sc.GRID, box, bounds) == 1]
    hub, sims = make_slabs(sc.GRID, bounds)
    for s in sims:
        seed(s, sc.APPEND_CALLS[0], sm.initial_state())
    collective(sims, lambda r, s: s.hash())
    s = sims[1]
    before, last = s.download_particles(write_positions=True), s.seed_last()
    assert len(before) > 0 and len(mine) > 1
    with pytest.raises(lfa.LibfluidError) as e:
        seed(s, sc.APPEND_CALLS[1], state, positions=len(mine) - 1)
    assert e.value.code == -1  # LFA_E_INVALID
    assert s.num_particles == len(before) and s.seed_last() == last
    assert s.download_particles(write_positions=True).tobytes() == before.tobytes()  # (still binned: nothing was touched)
    # an exact fit is accepted, and numbers its particles as if the refused call had never been made
    n, got_state, got = seed(s, sc.APPEND_CALLS[1], state, positions=len(mine))
    assert n == len(mine) and got.tobytes() == mine.tobytes() and got_state == state_after
    assert s.seed_last() == (n_cand, len(box), len(sphere)) and s.num_particles == len(before) + n
    close_all(hub, sims)
