"""The clouds of tests/test_gpu_pos_record.py hold what they are chosen for (no GPU): the residues of tile_start, holes in every
chunk of every wave of a slab rank, round-trip counts around a record, four records and a workgroup, a particle on the max face, and
a second pass and a gather pass that are actually taken per the layout restated in tests/correction_halfcell_cases.py."""
import numpy as np

from tests import correction_cases as cc
from tests import correction_halfcell_cases as hc
from tests import correction_output_cases as oc
from tests import pos_record_cases as pc
from tests import streaming_tail_cases as sc
from tests.test_correction_cases import cap_edge_prediction


def test_tile_start_takes_every_residue_mod_4():
    size, parts, solid, meta = pc.build("residues")
    start, count = pc.tile_starts(size, parts["pos"])
    assert tuple(count) == pc.RESIDUE_COUNTS and len(parts) == sum(pc.RESIDUE_COUNTS)
    assert set(int(s) % 4 for s in start) == {0, 1, 2, 3}
    assert all((start % 4 == r).sum() >= 2 for r in range(4))
    # dyadic and inside the grid: upload and download are exact at h = 1
    assert (parts["pos"] > 0).all() and (parts["pos"] < np.asarray(size)).all()
    assert np.array_equal(parts["pos"] * sc.Q, np.rint(parts["pos"] * sc.Q))
    # shuffled: the upload order is not the binned order
    assert (np.diff(pc.tile_ids(size, parts["pos"])) < 0).any()


def test_round_trip_counts_sit_on_the_tails_of_a_16_byte_access():
    assert pc.ROUND_TRIP_COUNTS == (1, 3, 4, 5, 255, 257)
    for n in pc.ROUND_TRIP_COUNTS:
        size, parts, solid, meta = sc.lattice(n)
        assert size == (24, 17, 17) and len(parts) == n
        assert np.array_equal(parts["pos"] * sc.Q, np.rint(parts["pos"] * sc.Q))  # exact in cell + fp32 fraction


def test_every_chunk_of_a_slab_rank_has_holes_lane_by_lane():
    size, parts, solid, meta = sc.build(f"lattice_n{sc.SLAB_N}")
    mine = np.floor(parts["pos"][:, 2]) < 8 * sc.SLAB_BOUNDS[1]  # rank 0 keeps these; to rank 1 they are holes, and the reverse
    full = len(parts) // 64 * 64
    per_chunk = mine[:full].reshape(-1, 64).sum(axis=1)
    assert per_chunk.min() >= 4 and per_chunk.max() <= 60  # both ranks see particles and holes in every chunk of 64
    assert len(parts) > sc.WAVE  # more than one wave of the advection


def test_mixed_has_particles_on_the_max_face():
    size, parts, solid, meta = sc.build("mixed")
    face = np.array([k == "max_face" for k in meta["kind"]])
    assert face.sum() >= 8 and (parts["pos"][face, 1] == size[1]).all() and (parts["pos"][~face] < np.asarray(size)).all()


def test_the_second_pass_and_the_gather_pass_are_taken():
    for name in ("second_pass", "second_pass_spread"):
        second, gather = hc.prediction(oc.build(name))
        assert len(second) > 0 and len(gather) == 0
    second, gather = cap_edge_prediction()
    assert len(gather) > 0 and len(second) > len(gather)
    assert "cap_edge" in cc.NAMES
