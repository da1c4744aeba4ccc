"""simulation::_update_sources / seed_cell restated in numpy, built on tests/seed_model.py: what the g++-built reference's fluid
sources seed from its pcg32 (src/simulation.cpp:756-765, 136-151).

The active sources are walked in order and their cells in list order. A cell whose hash count is below target = root^3 gets
target - count particles at (grid_offset + cell * cell_size) + (dx, dy, dz), each coordinate a uniform_real_distribution<double>(0,
cell_size) of two 32-bit draws, z drawn first (g++ evaluates the arguments of `vec3d(dist(random), dist(random), dist(random))`
right to left); then the count is set to target UNCONDITIONALLY (:150), also when it was larger. So new particle k of a call
starts at draw 6 k. tests/test_source_model.py pins this model to the compiled reference and to its recorded particles; the GPU
tests take their expected values from it."""
import numpy as np

from tests import seed_model as sm


def update_sources(grid_size, cell_size, offset, counts, sources, state, ltr=False):
    """counts: the space hash's particle count per cell (x fastest, any shape with nx * ny * nz entries; not modified).
    sources: [(cells int[k, 3], velocity, target_density_cubic_root, active), ...] (further entries are ignored).
    Returns (positions float64[n, 3] in draw order, source_cells int64[n, 3], velocities float64[n, 3], state afterwards)."""
    nx, ny, nz = (int(v) for v in grid_size)
    count = np.array(counts, dtype=np.int64).reshape(-1).copy()
    assert count.size == nx * ny * nz
    off, h = np.asarray(offset, dtype=np.float64), np.float64(cell_size)
    pos, cells, vels = [], [], []
    for src in sources:
        xyz, velocity, root, active = src[0], src[1], int(src[2]), bool(src[3])
        if not active:
            continue
        target = root ** 3
        for cell in np.asarray(xyz, dtype=np.int64).reshape(-1, 3):
            raw = int(cell[0] + nx * (cell[1] + ny * cell[2]))
            k = target - int(count[raw])
            count[raw] = target
            if k <= 0:
                continue
            st = sm._advance_each(state, np.arange(k, dtype=np.uint64) * np.uint64(6))
            u0, st = sm._uniform(st, h)
            u1, st = sm._uniform(st, h)
            u2, st = sm._uniform(st, h)
            u = (u0, u1, u2) if ltr else (u2, u1, u0)  # g++: the last argument is evaluated first
            corner = off + cell.astype(np.float64) * h  # one multiply, then one add, per axis
            pos.append(np.stack([corner[a] + u[a] for a in range(3)], axis=1))
            cells.append(np.broadcast_to(cell, (k, 3)))
            vels.append(np.broadcast_to(np.asarray(velocity, dtype=np.float64), (k, 3)))
            state = sm.advance(state, 6 * k)
    if not pos:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3)), state
    return np.concatenate(pos), np.concatenate(cells), np.concatenate(vels), state


def cell_counts(grid_size, cell_size, offset, positions):
    """The count half of the space hash after update_and_hash_particles (src/simulation.cpp:251-291): clamped cell of every
    position, true division in fp64."""
    n = np.asarray(grid_size, dtype=np.int64)
    g = (np.asarray(positions, dtype=np.float64).reshape(-1, 3) - np.asarray(offset, dtype=np.float64)) / np.float64(cell_size)
    idx = np.minimum(np.maximum(g, 0.0).astype(np.int64), n - 1)
    raw = idx[:, 0] + n[0] * (idx[:, 1] + n[1] * idx[:, 2])
    return np.bincount(raw, minlength=int(n.prod()))


def records(positions, velocities):
    """The 152-byte records seed_cell builds (raw_cell_index is recomputed by the device on upload)."""
    from libfluid_amd.scenes import PARTICLE_DTYPE
    out = np.zeros(len(positions), dtype=PARTICLE_DTYPE)
    out["pos"] = positions
    out["old_pos"] = positions
    out["vel"] = velocities
    return out


# ---- the counter-based default of lfa_update_sources (no pcg32): k_source_seed, mix64 keyed on the particle's id
_M64 = (1 << 64) - 1


def _mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & _M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & _M64
    return x ^ (x >> 31)


def blocked_index(grid_size, x, y, z):
    """The device's cell numbering: 8 x 8 x 8 tiles, x fastest among the tiles and inside one."""
    ntx, nty = (int(grid_size[0]) + 7) // 8, (int(grid_size[1]) + 7) // 8
    return ((x >> 3) + ntx * ((y >> 3) + nty * (z >> 3))) * 512 + ((x & 7) | ((y & 7) << 3) | ((z & 7) << 6))


def counter_entries(grid_size, counts, sources, z_range=None):
    """The flattened entry rule of lfa_sources_sync: [(cell, source index, need), ...] in list order. The first entry of a cell tops
    it up from the binning's count, a later one from the previous entry's target; an entry whose target does not exceed that is
    dropped (and still leaves its target behind). z_range: the cell layers [lo, hi) of a slab rank (the others' entries are not its)."""
    nx, ny, _ = (int(v) for v in grid_size)
    count = np.asarray(counts, dtype=np.int64).reshape(-1)
    last, out = {}, []
    for si, src in enumerate(sources):
        if not src[3]:
            continue
        target = int(src[2]) ** 3
        for x, y, z in np.asarray(src[0], dtype=np.int64).reshape(-1, 3).tolist():
            if z_range is not None and not z_range[0] <= z < z_range[1]:
                continue
            have = last.get((x, y, z))
            last[(x, y, z)] = target
            if have is not None and target <= have:
                continue
            if have is None:
                have = int(count[x + nx * (y + ny * z)])
            out.append(((x, y, z), si, max(target - have, 0)))
    return out


def counter_update_sources(grid_size, cell_size, offset, counts, sources, epoch, id_base, z_range=None):
    """What call number `epoch` (1 for a handle's first) of the plain lfa_update_sources creates: (the records a download with
    positions reports, uint32 ids). New particle k of the call has id = id_base + k, lies in its source cell at the fractions
    t[a] = float32(r >> 40) 2^-24, r = mix64(seed + ((id_base + k) 3 + a + 1) 0x9E3779B97F4A7C15 + (blocked cell << 40)) mod 2^64,
    seed = 0x5EED50 + epoch 0x632BE59BD9B4E019, and carries its source's velocity as float32 and C = 0."""
    from libfluid_amd.scenes import PARTICLE_DTYPE
    seed = 0x5EED50 + epoch * 0x632BE59BD9B4E019 & _M64
    off, h = np.asarray(offset, dtype=np.float64), np.float64(cell_size)
    cells, ts, vels = [], [], []
    for cell, si, need in counter_entries(grid_size, counts, sources, z_range):
        b = blocked_index(grid_size, *cell)
        for _ in range(need):
            pid = id_base + len(cells)
            r = [_mix64(seed + (pid * 3 + a + 1) * 0x9E3779B97F4A7C15 + (b << 40) & _M64) for a in range(3)]
            cells.append(cell)
            ts.append([np.float32(v >> 40) * np.float32(2.0 ** -24) for v in r])
            vels.append(np.asarray(sources[si][1], dtype=np.float32))
    out = np.zeros(len(cells), dtype=PARTICLE_DTYPE)
    if len(cells):
        c = np.asarray(cells, dtype=np.int64)
        out["pos"] = off + (c.astype(np.float64) + np.asarray(ts, dtype=np.float32).astype(np.float64)) * h  # k_export's sum
        out["old_pos"] = out["pos"]
        out["vel"] = np.asarray(vels, dtype=np.float32).astype(np.float64)
        out["raw"] = c[:, 0] + int(grid_size[0]) * (c[:, 1] + int(grid_size[1]) * c[:, 2])
    return out, (id_base + np.arange(len(cells))).astype(np.uint32)
