"""lfa_frame_stats / lfa_download_positions on virtual slabs (N handles on one GPU, in-process transport, set up as in
tests/test_gpu_seed_slabs.py): every rank summarises the records it owns, and the ranks' results combine - counts, sums and grids
add, max_speed2 / hi take the maximum, lo the minimum - to the model of the union of the ranks' downloads.

A block that straddles every slab face moves in z for two time steps, so the handles hold leavers' holes, arrivals and ghosts.
A 16 x 16 x 32 grid has four tile layers: two slabs, three uneven ones and the (only, even) split into four; four UNEVEN slabs need
a fifth layer and run on 16 x 16 x 40."""
import numpy as np
import pytest

import libfluid_amd as lfa
from libfluid_amd import scenes
from tests import frame_model as fm
from tests import util
from tests.test_gpu_seed_slabs import close_all, collective, make_slabs

pytestmark = pytest.mark.gpu

OFFSET = (0.0, 0.0, 0.0)
H = 1.0
GRAVITY = (0.0, -981.0, 0.0)
CASES = {"2 slabs": (32, [0, 2, 4]), "3 uneven slabs": (32, [0, 1, 2, 4]), "4 slabs": (32, [0, 1, 2, 3, 4]),
         "4 uneven slabs": (40, [0, 1, 2, 4, 5])}
KW = dict(method=lfa.APIC, precond=lfa.PRECOND_MIC0_TILED, pcg_dtype=lfa.PCG_F64)


def block(nz):
    parts = scenes.seed_block((4, 2, 4), (12, 10, nz - 4))
    up = (parts["pos"][:, 0] < 8.0)
    parts["vel"] = np.where(up[:, None], [1.0, 0.0, 45.0], [-1.0, 0.0, -45.0])  # both ways across every face
    return parts


@pytest.mark.parametrize("name", list(CASES))
def test_ranks_combine_to_the_single_domain_model(name):
    nz, bounds = CASES[name]
    size = (16, 16, nz)
    grid = dict(size=size, cell_size=H, offset=OFFSET)
    hub, sims = make_slabs(grid, bounds, gravity=GRAVITY, **KW)
    parts = block(nz)
    for s in sims:
        s.upload_particles(parts)
    # unbinned: refused like the download, with its message
    for s in sims:
        for call in (s.frame_stats, s.positions):
            with pytest.raises(lfa.LibfluidError) as e:
                call()
            assert e.value.code == -1 and "lfa_hash_particles" in str(e.value)
    collective(sims, lambda r, s: s.hash())
    before = [s.num_particles for s in sims]

    def steps(r, s):
        for _ in range(2):
            assert s.time_step(util.DT)[2] >= 0

    collective(sims, steps)
    after = [s.num_particles for s in sims]
    assert sum(after) == sum(before) == len(parts) and after != before, "the block is meant to cross the slab faces"

    got = [s.frame_stats() for s in sims]           # before the downloads: the calls under test meet the state the steps left
    pos = [s.positions() for s in sims]
    again = [s.frame_stats() for s in sims]
    down = [s.download_particles(write_positions=True) for s in sims]
    close_all(hub, sims)
    for r, ((st, occ), p, d) in enumerate(zip(got, pos, down)):
        m = fm.summary(d, size, OFFSET, H, GRAVITY)
        bound = fm.energy_bound(len(d), m["energy_abs"])
        print(name, "rank", r, "n", st.n, "energy", st.energy, "model", m["energy"], "bound", bound)
        assert st.n == len(d) == after[r] and st.n_in_grid == m["n_in_grid"]
        assert np.array_equal(occ, m["occupation"])
        assert p.tobytes() == np.ascontiguousarray(d["pos"]).tobytes()
        assert abs(st.energy - m["energy"]) <= bound and abs(st.energy_abs - m["energy_abs"]) <= bound
        assert bytes(memoryview(st)) == bytes(memoryview(again[r][0])) and np.array_equal(occ, again[r][1])
    whole = fm.summary(np.concatenate(down), size, OFFSET, H, GRAVITY)
    assert np.array_equal(sum(occ.astype(np.uint64) for _, occ in got), whole["occupation"].astype(np.uint64))
    assert sum(st.n for st, _ in got) == whole["n"] == len(parts)
    assert sum(st.n_in_grid for st, _ in got) == whole["n_in_grid"]
    assert max(st.max_speed2 for st, _ in got) == whole["max_speed2"]
    assert np.array_equal(np.min([np.array(st.lo) for st, _ in got], axis=0), whole["lo"])
    assert np.array_equal(np.max([np.array(st.hi) for st, _ in got], axis=0), whole["hi"])
