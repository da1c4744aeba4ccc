"""The scenes of tests/source_slab_cases.py do, on the model, what tests/test_gpu_source_rng_slabs.py needs them for."""
import numpy as np
import pytest

from tests import source_slab_cases as ssc


def test_x_face_particles_change_rank_upward_only():
    grid, _, _, _ = ssc.case("X_face")
    bounds, = ssc.BOUNDS["X_face"]
    pos, cells, _, _ = ssc.expected("X_face")
    assert len(pos) == 5 * 4096
    by_key, by_source = ssc.owner(grid, pos, bounds), ssc.source_owner(cells, bounds)
    assert not (by_key < by_source).any()
    for z, rank in ((7, 1), (15, 2)):  # the cell layers below the two slab faces
        moved = (cells[:, 2] == z) & (by_key == rank)
        assert moved.sum() >= 10 and (by_source[moved] == rank - 1).all()
    assert (by_key > by_source).sum() == sum(((cells[:, 2] == z) & (by_key > by_source)).sum() for z in (7, 15))
    # z = 8 and z = 6 cross a cell face inside a rank, z = 23 is clamped at the grid's top
    layer = ssc.ssc.layer(grid, pos)
    g = (pos[:, 2] - grid["offset"][2]) / grid["cell_size"]
    for z in (6, 8):
        assert ((cells[:, 2] == z) & (np.floor(g) == z + 1)).sum() >= 1
        assert (by_key[cells[:, 2] == z] == by_source[cells[:, 2] == z]).all()
    assert ((cells[:, 2] == 23) & (g >= 24.0)).sum() >= 1 and (layer[cells[:, 2] == 23] == 2).all()


@pytest.mark.parametrize("bounds", ssc.BOUNDS["I_interleave"], ids=str)
def test_interleave_spreads_every_rank_over_the_scan(bounds):
    grid, _, sources, _ = ssc.case("I_interleave")
    pos, cells, _, _ = ssc.expected("I_interleave")
    assert len(sources[0][0]) >= 300
    own = ssc.owner(grid, pos, bounds)
    for r in range(len(bounds) - 1):
        draws = np.flatnonzero(own == r)
        assert len(draws) > 0
        assert draws[-1] - draws[0] + 1 > len(draws)  # not one contiguous block of draw numbers


def test_b_leaves_rank_1_empty():
    grid, _, _, _ = ssc.case("B")
    pos, _, _, _ = ssc.expected("B")
    own = ssc.owner(grid, pos, [0, 1, 2])
    assert len(pos) > 0 and not (own == 1).any()


def test_c_interleaves_the_ranks():
    grid, _, _, _ = ssc.case("C")
    pos, _, _, _ = ssc.expected("C")
    own = ssc.owner(grid, pos, [0, 1, 2])
    assert np.count_nonzero(np.diff(own)) >= 3  # the owner changes several times along the draw order


@pytest.mark.parametrize("name,bounds", ssc.PAIRS, ids=str)
def test_bounds_fit_the_grid(name, bounds):
    grid = ssc.case(name)[0]
    assert bounds[0] == 0 and bounds[-1] == (grid["size"][2] + 7) // 8 and all(a < b for a, b in zip(bounds, bounds[1:]))
