"""What the reference's hosts compute from simulation::particles() after a step, restated in numpy on a PARTICLE_DTYPE array.

  * the testbed's update_simulation (testbed/main.cpp:50-88): "total energy" = sum of 0.5 |v|^2 - g . x, and the occupation grid,
    indexed by vec3s(vec3i((position - grid_offset) / cell_size)) - an fp64 division truncated toward zero, counted iff every index
    is inside the grid;
  * its post_grid_to_particle_transfer_callback (:117-123): the largest |v|^2, from 0, std::max skipping a NaN.
The per-particle terms are formed like the callers form them: squared_length adds vx vx, vy vy, vz vz in that order, dot adds
gx x, gy y, gz z. tests/test_frame_model.py pins this to the compiled reference's recorded outputs; the GPU tests apply it to an
LFA_DL_POSITIONS download of the handle they query."""
import numpy as np


def cells(pos, offset, cell_size):
    """int64[n, 3]: vec3i((position - grid_offset) / cell_size), truncation toward zero."""
    g = (np.asarray(pos, dtype=np.float64) - np.asarray(offset, dtype=np.float64)[None, :]) / np.float64(cell_size)
    return np.trunc(g).astype(np.int64)


def occupation(pos, size, offset, cell_size):
    """(uint32[nz, ny, nx], particles counted)"""
    nx, ny, nz = (int(v) for v in size)
    c = cells(pos, offset, cell_size)
    ok = ((c >= 0) & (c < np.array([nx, ny, nz]))).all(axis=1)
    raw = c[ok, 0] + nx * (c[ok, 1] + ny * c[ok, 2])
    grid = np.bincount(raw, minlength=nx * ny * nz).astype(np.uint32)
    return grid.reshape(nz, ny, nx), int(ok.sum())


def terms(parts, gravity):
    """(0.5 |v|^2, g . x, |v|^2) per particle, each in the callers' order of operations."""
    v, x = parts["vel"], parts["pos"]
    g = np.asarray(gravity, dtype=np.float64)
    sq = v[:, 0] * v[:, 0]
    sq = sq + v[:, 1] * v[:, 1]
    sq = sq + v[:, 2] * v[:, 2]
    dot = g[0] * x[:, 0]
    dot = dot + g[1] * x[:, 1]
    dot = dot + g[2] * x[:, 2]
    return 0.5 * sq, dot, sq


def summary(parts, size, offset, cell_size, gravity):
    """The fields of lfa_frame_stats plus the occupation grid, as a dict."""
    n = len(parts)
    half, dot, sq = terms(parts, gravity)
    occ, n_in = occupation(parts["pos"], size, offset, cell_size)
    finite = sq[~np.isnan(sq)]
    out = dict(n=n, n_in_grid=n_in, occupation=occ,
               energy=float(np.sum(half - dot)), energy_abs=float(np.sum(half + np.abs(dot))),
               max_speed2=float(finite.max()) if len(finite) else 0.0)
    out["max_speed2"] = max(out["max_speed2"], 0.0)
    out["lo"] = parts["pos"].min(axis=0) if n else np.full(3, np.inf)
    out["hi"] = parts["pos"].max(axis=0) if n else np.full(3, -np.inf)
    return out


def energy_bound(n, energy_abs):
    """|difference| of two fp64 summation orders of the same n terms (n eps sum |term| to first order, each side), plus one
    rounding of every term: 2 n 2^-53 energy_abs."""
    return 2.0 * n * 2.0 ** -53 * energy_abs
