"""CPU check of the scenes tests/test_gpu_seed_slabs.py seeds on slabs, from tests/seed_model.py alone: the GPU tests compare
every rank with the model's particles filtered by owner, which proves nothing on a rank the scene gives no particle to.

The box of tests/test_gpu_seed.py ends at z = 9.2, below tile layer 2, and its corner sphere starts at z = 13.1, above tile
layer 0: on their own neither can reach every rank of every bounds list. So the demand is made of the cases of the partition
test TOGETHER - under every bounds list every rank is given particles by at least one of them, each of the two is cut by at
least one bounds list - and of the tall box, which spans all three layers, on its own."""
import numpy as np
import pytest

from tests import seed_slab_cases as sc


def per_rank(grid, calls, bounds):
    pos = np.concatenate([p for p, _, _ in sc.model(sc.key(grid), calls)])
    return np.bincount(sc.owner(grid, pos, bounds), minlength=len(bounds) - 1), len(pos)


@pytest.mark.parametrize("bounds", sc.BOUNDS)
def test_every_rank_is_given_particles(bounds):
    counts = {name: per_rank(grid, calls, bounds)[0] for name, (grid, calls) in sc.PARTITION_CASES.items()}
    got = np.sum(list(counts.values()), axis=0)
    assert (got > 0).all(), counts
    assert (counts["tall-box-d2"] > 0).all(), counts
    for calls in (sc.APPEND_CALLS, sc.BIG_CALLS):
        grid = sc.BIG if calls is sc.BIG_CALLS else sc.GRID
        assert (per_rank(grid, calls, [0, 1, 2, 3])[0] > 0).all()


@pytest.mark.parametrize("name", ["box-d2", "box-d3", "corner-sphere-d2"])
def test_the_shapes_of_the_single_domain_tests_are_cut_by_a_slab_face(name):
    grid, calls = sc.PARTITION_CASES[name]
    assert any((per_rank(grid, calls, b)[0] > 0).sum() > 1 for b in sc.BOUNDS)


def test_the_low_box_leaves_the_upper_ranks_empty():
    counts, n = per_rank(sc.GRID, sc.LOW_CALLS, [0, 1, 3])
    assert n > 0 and counts.tolist() == [n, 0]
    counts, _ = per_rank(sc.GRID, sc.LOW_CALLS, [0, 1, 2, 3])
    assert counts.tolist() == [n, 0, 0]


@pytest.mark.parametrize("bounds", sc.BOUNDS)
def test_the_owner_rule_is_a_partition(bounds):
    cases = list(sc.PARTITION_CASES.values()) + [(sc.GRID, sc.APPEND_CALLS), (sc.GRID, sc.LOW_CALLS)]
    for grid, calls in cases:
        pos = np.concatenate([p for p, _, _ in sc.model(sc.key(grid), calls)])
        own = sc.owner(grid, pos, bounds)
        assert own.min() >= 0 and own.max() <= len(bounds) - 2  # every particle has an owner among the ranks ...
        # ... exactly one: the ranks' layer ranges are disjoint and cover the grid's layers
        lay = sc.layer(grid, pos)
        member = np.stack([(lay >= bounds[r]) & (lay < bounds[r + 1]) for r in range(len(bounds) - 1)])
        assert (member.sum(axis=0) == 1).all() and np.array_equal(member.argmax(axis=0), own)
        assert lay.max() <= (grid["size"][2] - 1) >> 3


def test_the_step_scenes_lie_at_their_faces():
    """The dam ends below the face at z = 16 (it has to cross it by moving), the sphere seeded after the steps lies across it."""
    for b in sc.STEP_BOUNDS.values():
        counts, n = per_rank(sc.STEP_GRID, (sc.STEP_BOX,), b)
        assert n > 0 and counts[-1] == 0, (b, counts)
    counts, n = per_rank(sc.STEP_GRID, (sc.STEP_SPHERE,), sc.STEP_BOUNDS["apic"])
    assert n > 0 and (counts > 0).all(), counts
