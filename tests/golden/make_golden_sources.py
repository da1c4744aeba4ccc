"""Generates tests/golden/source_seeding.npz from the REAL reference (oracle/_ref/libref.so): the particles its fluid sources
seed (simulation::_update_sources, src/simulation.cpp:756-765) in the scenes of tests/source_cases.py, from a freshly constructed
simulation's generator. Per case: <name>_pos float64[n, 3] (rows sorted lexicographically: the reference's sort by cell is
unstable), <name>_raw uint64[n] (raw_cell_index: the SOURCE cell) and <name>_vel float64[n, 3] in the same order. Needs
oracle/_ref/libref.so (oracle.loader.build()). Data only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import loader as orc  # noqa: E402
from tests import source_cases as sc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_seeds(name):
    """(positions, raw_cell_index, velocities) of the records the reference's update_sources adds, as sorted rows."""
    grid, parts, sources, _ = sc.case(name)
    s = orc.CpuSim(grid["size"], cell_size=grid["cell_size"], offset=grid["offset"], kind="ref")
    if parts is not None:
        s.set_particles(parts)
    s.hash()
    for cells, vel, root, active in sources:
        s.add_source(cells, vel, root, active, False)
    s.update_sources()
    after = s.particles()
    s.close()
    if parts is not None and len(parts):  # the new records: those whose position no resident particle has
        old = {p.tobytes() for p in np.ascontiguousarray(parts["pos"])}
        new = np.array([p.tobytes() not in old for p in np.ascontiguousarray(after["pos"])])
        assert new.sum() == len(after) - len(parts)
        after = after[new]
    assert not after["cx"].any() and not after["cy"].any() and not after["cz"].any()
    assert np.array_equal(after["old_pos"], after["pos"])
    return sc.sorted_rows(after["pos"].copy(), after["raw"].copy(), after["vel"].copy())


if __name__ == "__main__":
    orc.build()
    if not orc.have_ref():
        sys.exit("oracle/_ref/libref.so is not built")
    out = {}
    for name in sc.RTL:
        pos, raw, vel = reference_seeds(name)
        out.update({f"{name}_pos": pos, f"{name}_raw": raw, f"{name}_vel": vel})
        print(name, pos.shape)
    path = os.path.join(HERE, "source_seeding.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")
