"""lfa_update_sources_rng / lfa_set_source_rng with LFA_SEED_COLLECTIVE on virtual slabs (N handles on one GPU, in-process
transport) against tests/source_model.py, in the scenes of tests/source_slab_cases.py: every rank keeps the model's new particles
whose key lies in its tile layers, byte for byte and in draw order, numbered by their index in the single-domain draw order; the
ranks' downloads gathered by id are the single-domain handle's download. tests/test_source_slab_cases.py checks on the CPU that
the scenes reach the ranks, and cross the slab faces, they are meant to.

The call exchanges a message (one all-reduce) and ends with the re-binning, so it runs on one host thread per rank."""
import ctypes as C
import threading

import numpy as np
import pytest

import libfluid_amd as lfa
from tests import seed_model as sm
from tests import source_model as srcm
from tests import source_slab_cases as ssc

pytestmark = pytest.mark.gpu

NO_PARTS = np.zeros(0, dtype=lfa.PARTICLE_DTYPE)
NOTHING_AGAIN = ("A", "B", "E_root16", "F_ltr_B")  # as in tests/test_gpu_source_rng.py: a second call finds every cell full


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


def make_slabs(grid, bounds, parts, sources, binned=True):
    """Every rank is handed the whole record set (it keeps what lies in its layers) and the whole source list."""
    hub = lfa.LocalHub(len(bounds) - 1)
    sims = [lfa.Sim(**grid) for _ in bounds[1:]]
    for r, s in enumerate(sims):
        s.init_local_slab(hub.h, r, bounds)
        s.upload_particles(NO_PARTS if parts is None else parts)
        for cells, vel, root, active in sources:
            s.add_source(cells, vel, root, active, False)
    if binned:
        collective(sims, lambda r, s: s.hash())
    return hub, sims


def single_domain(grid, parts, sources):
    one = lfa.Sim(**grid)
    one.upload_particles(NO_PARTS if parts is None else parts)
    one.hash()
    for cells, vel, root, active in sources:
        one.add_source(cells, vel, root, active, False)
    return one


def close_all(hub, sims):
    for s in sims:
        s.close()
    hub.close()


def gather(sims):
    """The handles' downloads, concatenated and ordered by id: (records, ids). The handles must be binned."""
    parts = [s.download_particles(write_positions=True) for s in sims]
    ids = np.concatenate([s.particle_ids() for s in sims])
    order = np.argsort(ids, kind="stable")
    return np.concatenate(parts)[order], ids[order]


def check_partition(name, bounds):
    """What test 1 asks of a case on the slabs `bounds`; returns the positions every rank was handed."""
    grid, parts, sources, ltr = ssc.case(name)
    pos, _, _, state = ssc.expected(name)
    own = ssc.owner(grid, pos, bounds)
    ltr_flag = lfa.SEED_DRAW_LTR if ltr else 0
    first, s0 = 0 if parts is None else len(parts), sm.initial_state()
    hub, sims = make_slabs(grid, bounds, parts, sources)
    one = single_domain(grid, parts, sources)
    try:
        resident = [s.num_particles for s in sims]
        assert sum(resident) == first
        res = collective(sims, lambda r, s: s.update_sources_rng(s0, flags=lfa.SEED_COLLECTIVE | ltr_flag, positions=True))
        for r, (s, (n, got_state, got_pos)) in enumerate(zip(sims, res)):
            mine = pos[own == r]
            print(name, bounds, "rank", r, "kept", n, "of", len(pos), "model", len(mine))
            assert n == len(mine), (r, n, len(mine))
            assert got_pos.tobytes() == mine.tobytes(), r
            assert got_state == state, r
            assert s.source_last() == (len(pos), len(mine), first), r
            assert s.num_particles == resident[r] + n, r
        n1, state1, _ = one.update_sources_rng(s0, flags=ltr_flag)
        assert (n1, state1) == (len(pos), state) and one.source_last() == (n1, n1, first)
        got, ids = gather(sims)
        ref, ref_ids = gather([one])
        assert np.array_equal(ids, np.arange(first + len(pos), dtype=np.uint32))  # the new ids: first .. first + total - 1, each once
        assert np.array_equal(ref_ids, ids)
        assert got.tobytes() == ref.tobytes()
        # a second call: what the single domain's second call creates
        n2, state2, _ = one.update_sources_rng(state, flags=ltr_flag)
        res2 = collective(sims, lambda r, s: s.update_sources_rng(state, flags=lfa.SEED_COLLECTIVE | ltr_flag))
        assert sum(n for n, _, _ in res2) == n2
        assert all(st == state2 for _, st, _ in res2)
        if name in NOTHING_AGAIN:
            assert n2 == 0 and state2 == state  # nothing to create: the state is left alone
        if n2:
            assert all(s.source_last() == (n2, n, first + len(pos)) for s, (n, _, _) in zip(sims, res2))
            got, ids = gather(sims)
            ref, ref_ids = gather([one])
            assert np.array_equal(ids, ref_ids) and got.tobytes() == ref.tobytes()
        return [p for _, _, p in res]
    finally:
        one.close()
        close_all(hub, sims)


@pytest.mark.parametrize("name,bounds", [p for p in ssc.PAIRS if p[0] != "X_face"], ids=lambda v: str(v).replace(" ", ""))
def test_partition_is_bit_exact(name, bounds):
    check_partition(name, bounds)


def test_positions_that_round_across_a_slab_face():
    """X_face: particles of the cell layer below a slab face whose position rounds onto the face are created on the rank above."""
    bounds, = ssc.BOUNDS["X_face"]
    got = check_partition("X_face", bounds)
    grid = ssc.case("X_face")[0]
    pos, cells, _, _ = ssc.expected("X_face")
    by_source = ssc.source_owner(cells, bounds)
    for r in (1, 2):
        from_below = pos[(ssc.owner(grid, pos, bounds) == r) & (by_source == r - 1)]
        assert len(from_below) >= 10
        mine = {row.tobytes() for row in got[r]}
        assert all(row.tobytes() in mine for row in from_below)


MODE_GRID = dict(size=(16, 16, 32), cell_size=1.0, offset=(0.0, 0.0, 0.0))
MODE_BOUNDS = [0, 2, 4]
MODE_SOURCES = [([(x, 15, z) for z in range(12, 21) for x in range(5, 11)], (0.0, -30.0, 0.0), 2, True)]  # across the face z = 16


@pytest.mark.parametrize("before_attach", [False, True], ids=["mode-after-attach", "mode-before-attach"])
def test_handle_mode_in_time_steps(before_attach):
    s0 = sm.initial_state()
    pos, _, _, s1 = srcm.update_sources(MODE_GRID["size"], 1.0, MODE_GRID["offset"], np.zeros(16 * 16 * 32), MODE_SOURCES, s0)
    hub = lfa.LocalHub(2)
    sims = [lfa.Sim(**MODE_GRID) for _ in range(2)]
    for r, s in enumerate(sims):
        if before_attach:
            s.set_source_rng(True, s0, lfa.SEED_COLLECTIVE)
        s.init_local_slab(hub.h, r, MODE_BOUNDS)
        if not before_attach:
            s.set_source_rng(True, s0, lfa.SEED_COLLECTIVE)
        assert s.get_source_rng() == (True, s0)
        s.upload_particles(NO_PARTS)
        s.add_source(*MODE_SOURCES[0], False)
    try:
        state, total = s0, 0
        for step in range(2):
            rcs = collective(sims, lambda r, s: s.time_step(0.004)[2])
            assert all(rc >= 0 for rc in rcs)
            n = sum(s.num_particles for s in sims)
            state = sm.advance(state, 6 * (n - total))
            assert [s.get_source_rng() for s in sims] == [(True, state)] * 2
            assert all(s.source_last()[0] == n - total and s.source_last()[2] == total for s in sims)
            if step == 0:
                assert n == len(pos) == 8 * len(MODE_SOURCES[0][0]) and state == s1
                assert all(s.num_particles > 0 for s in sims)
            else:
                assert n > total
            total = n
            collective(sims, lambda r, s: s.hash())
            _, ids = gather(sims)
            assert np.array_equal(ids, np.arange(total, dtype=np.uint32))
    finally:
        close_all(hub, sims)


def test_refusals():
    grid, parts, sources, _ = ssc.case("C")
    bounds, s0 = [0, 1, 2], 0x0123456789ABCDEF
    # ---- an unbinned slab handle: LFA_E_INVALID on every rank, before any message
    hub, sims = make_slabs(grid, bounds, parts, sources, binned=False)
    for s in sims:
        state = C.c_uint64(s0)
        assert s.lib.lfa_update_sources_rng(s.h, C.byref(state), lfa.SEED_COLLECTIVE, None, None, 0) == -1
        assert state.value == s0 and s.source_last() == (0, 0, 0)
    collective(sims, lambda r, s: s.hash())
    before = [s.download_particles(write_positions=True) for s in sims]
    for s, rec in zip(sims, before):
        state = C.c_uint64(s0)
        # without the flag: LFA_E_UNSUPPORTED; an unknown flag: LFA_E_INVALID
        assert s.lib.lfa_update_sources_rng(s.h, C.byref(state), 0, None, None, 0) == -6
        assert b"slab" in s.lib.lfa_last_error(s.h)
        assert s.lib.lfa_update_sources_rng(s.h, C.byref(state), lfa.SEED_DRAW_LTR, None, None, 0) == -6
        assert s.lib.lfa_update_sources_rng(s.h, C.byref(state), lfa.SEED_COLLECTIVE | 4, None, None, 0) == -1
        for flags, code in ((0, -6), (lfa.SEED_COLLECTIVE | 8, -1)):
            with pytest.raises(lfa.LibfluidError) as e:
                s.set_source_rng(True, s0, flags)
            assert e.value.code == code
        assert state.value == s0 and s.get_source_rng() == (False, 0) and s.source_last() == (0, 0, 0)
        assert s.download_particles(write_positions=True).tobytes() == rec.tobytes()
    # ---- a short positions buffer on one rank fails that rank alone; its peer's re-binning is told at once, and the job ends
    pos = ssc.expected("C")[0]
    mine = pos[ssc.owner(grid, pos, bounds) == 1]
    assert len(mine) > 1

    def call(r, s):
        try:
            s.update_sources_rng(sm.initial_state(), flags=lfa.SEED_COLLECTIVE, positions=len(mine) - 1 if r == 1 else True)
        except lfa.LibfluidError as e:
            return e.code
        return 0

    codes = collective(sims, call)
    assert codes[1] == -1 and codes[0] < 0, codes
    assert sims[1].num_particles == len(before[1]) and sims[1].source_last() == (0, 0, 0)
    close_all(hub, sims)


def test_the_flag_on_a_single_domain_changes_nothing():
    grid, parts, sources, _ = ssc.case("C")
    a, b = single_domain(grid, parts, sources), single_domain(grid, parts, sources)
    ra = a.update_sources_rng(sm.initial_state(), positions=True)
    rb = b.update_sources_rng(sm.initial_state(), flags=lfa.SEED_COLLECTIVE, positions=True)
    assert ra[:2] == rb[:2] == (len(ssc.expected("C")[0]), ssc.expected("C")[3])
    assert ra[2].tobytes() == rb[2].tobytes() and a.source_last() == b.source_last()
    assert a.download_particles(write_positions=True).tobytes() == b.download_particles(write_positions=True).tobytes()
    assert np.array_equal(a.particle_ids(), b.particle_ids())
    b.set_source_rng(True, ra[1], lfa.SEED_COLLECTIVE)  # the handle mode takes the flag too
    assert a.update_sources_rng(ra[1])[0] == b.update_sources() > 0
    assert b.get_source_rng()[1] == sm.advance(ra[1], 6 * a.source_last()[0])
    assert a.download_particles(write_positions=True).tobytes() == b.download_particles(write_positions=True).tobytes()
    a.close()
    b.close()


def test_counter_based_default_is_untouched():
    """Plain update_sources on slabs: handles whose mode was switched on with the collective flag and off again seed what handles
    that never heard of the mode seed - ids in rank order, the generator's sequence - and no pcg32 seeding is recorded."""
    grid, parts, sources, _ = ssc.case("C")
    bounds = [0, 1, 2]
    hub_a, plain = make_slabs(grid, bounds, parts, sources)
    hub_b, toggled = make_slabs(grid, bounds, parts, sources)
    for s in toggled:
        s.set_source_rng(True, 12345, lfa.SEED_COLLECTIVE | lfa.SEED_DRAW_LTR)
        s.set_source_rng(False)
        assert s.get_source_rng() == (False, 0)
    for _ in range(2):
        na = collective(plain, lambda r, s: s.update_sources())
        nb = collective(toggled, lambda r, s: s.update_sources())
        assert na == nb and sum(na) > 0
        for a, b in zip(plain, toggled):
            assert a.download_particles(write_positions=True).tobytes() == b.download_particles(write_positions=True).tobytes()
            assert np.array_equal(a.particle_ids(), b.particle_ids())
            assert b.source_last() == (0, 0, 0)
    close_all(hub_a, plain)
    close_all(hub_b, toggled)


def test_counter_based_default_against_the_model():
    """Plain update_sources on two slabs: every rank creates the model's records of its own cell layers, the ids continue in rank
    order; gathered by id they are the model's with id_base per rank, byte for byte, in two consecutive calls."""
    from tests import source_cases as sc
    hub, sims = make_slabs(sc.COUNTER_GRID, [0, 1, 2], sc.counter_parts(), sc.COUNTER_SOURCES)
    try:
        held, held_ids = gather(sims)
        assert np.array_equal(held_ids, np.arange(3))
        for per_rank, n_want in zip(sc.counter_expected(2, ranks_z=((0, 8), (8, 16))), ((52, 34), (19, 0))):
            assert tuple(len(rec) for rec, _ in per_rank) == n_want
            assert tuple(collective(sims, lambda r, s: s.update_sources())) == n_want
            got, ids = gather(sims)
            want = np.concatenate([held] + [rec for rec, _ in per_rank])
            assert np.array_equal(ids, np.concatenate([held_ids] + [i for _, i in per_rank]))
            assert np.array_equal(ids, np.arange(len(want)))
            assert got.tobytes() == want.tobytes()
            held, held_ids = got, ids
    finally:
        close_all(hub, sims)
