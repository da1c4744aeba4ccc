"""Adversarial inputs of the surface mesher: particle clouds for the sampling path (k_count_particles, k_scatter_particles,
k_sort_groups, k_gather_positions, k_sample_surface and the three scan kernels) and fields for the extraction path (k_mc_classify,
k_mc_vertices, k_mc_triangles). Pure numpy, fixed seeds.

Every designed decision is dyadic: cell sizes 1 or 0.5, grid offsets multiples of 1/4, positions multiples of 2^-20 cells, dyadic
extents and radii r. (p - offset) / cell_size is then exact, device and reference see the same bits, and a deviation is a logic
error, not rounding. Exceptions, on purpose: `kernel_edge` (offsets of 2^-30 of the extent: the squares round, identically in both
codes), `radii` (extent 0.9 x radius) and `offgrid` (cell size 0.7).

cloud(id) -> (particles float64[n, 3], settings as in tests/mesher_cases.py, r included); field(id) -> (values float64[nz + 1, ny + 1,
nx + 1], dict(size, grid_offset, cell_size)). The second half of the file restates in numpy what the cases hold; the counts are
asserted by tests/test_mesher_edge_cases.py."""
import functools

import numpy as np

Q = 2.0 ** -20          # the position lattice, in cells
SCAN_BLOCK = 2048       # entries per workgroup of the device scan (mesher.hip)
PER2 = 1024 * SCAN_BLOCK  # from this many cells on a thread of k_scan_block_sums holds two block sums
SCAN_COUNTS = {255: (3, 5, 17), 256: (4, 8, 8), 257: (257, 1, 1), 2047: (23, 89, 1), 2048: (8, 16, 16), 2049: (3, 683, 1),
               4096: (16, 16, 16)}
RADII = (1, 2, 5, 9, 20, 64)
GAP_RADII = (3, 9)
GAP_BLOCKS = {"highest": (2, 2, 2), "middle": (1, 1, 1), "corner": (0, 0, 0)}
OFFGRID_RADII = (1, 4)
UNREPRESENTABLE = (np.nan, np.inf, -np.inf, 1e300, -1e300, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 1.0)

CLOUD_IDS = (["cell_faces", "cell_faces_h05", "unrepresentable", "kernel_edge"] + [f"radii-{r}" for r in RADII] +
             [f"block_gaps-{r}-{v}" for r in GAP_RADII for v in GAP_BLOCKS] + ["heavy_cells"] +
             [f"scan_edges-{n}" for n in SCAN_COUNTS] + ["wide_sheet"] + [f"offgrid-{r}" for r in OFFGRID_RADII])
FIELD_IDS = ["extremes", "near_ties"] + [f"scan_edges-{n}" for n in SCAN_COUNTS] + ["wide_sheet_field"]


def _settings(size, radius, extent, r, cell_size=1.0, grid_offset=(0.0, 0.0, 0.0)):
    return dict(size=tuple(size), grid_offset=tuple(grid_offset), cell_size=cell_size, particle_extent=extent, cell_radius=radius, r=r)


def _world(cells, kw):
    """Cell coordinates -> world positions (exact for lattice coordinates and the dyadic settings)."""
    return np.asarray(kw["grid_offset"])[None, :] + kw["cell_size"] * np.asarray(cells, dtype=np.float64)


def _lattice(rng, lo, hi, n):
    """n x 3 coordinates uniform on the 2^-20 lattice of [lo, hi) (per axis)."""
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (3,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (3,))
    k = rng.integers(0, ((hi - lo) / Q).astype(np.int64), size=(n, 3))
    return lo[None, :] + k * Q


# ------------------------------------------------------------------------------------------------------------ clouds
def cell_faces_coordinates(size):
    """Cell coordinates of the keep / drop decisions of particle_cell, axis by axis: 2^-20 either side of and exactly on the faces
    k = 0, 1, 2, n - 1, n, and - 0.5 and - 1.5 cells (truncation toward zero: index 0, dropped as such; index - 1, outside). The other
    two coordinates sit mid-cell in the interior."""
    out = []
    for a in range(3):
        n = size[a]
        along = [k + d for k in (0, 1, 2, n - 1, n) for d in (-Q, 0.0, Q)] + [-0.5, -1.5]
        for j, c in enumerate(along):
            p = [0.0, 0.0, 0.0]
            p[a] = c
            p[(a + 1) % 3] = 2.5 + j % 3
            p[(a + 2) % 3] = 2.5 + (j // 3) % 3
            out.append(p)
    return np.array(out)


def _cell_faces(cell_size, grid_offset):
    # (extent and r are world lengths: at cell size 0.5 the extent is 3 cells, more than the 2 cells a grid point looks at)
    kw = _settings((9, 8, 7), 2, 1.5, 0.5, cell_size, grid_offset)
    c = cell_faces_coordinates(kw["size"])
    return _world(c[np.random.default_rng(31).permutation(len(c))], kw), kw


def _unrepresentable():
    """cell_faces plus particles with one coordinate no int can hold, spread through the input order (the kept particles keep their
    relative order, so the expected values and mesh are those of cell_faces)."""
    p, kw = _cell_faces(1.0, (0.0, 0.0, 0.0))
    bad = []
    for a in range(3):
        for j, v in enumerate(UNREPRESENTABLE):
            q = [0.0, 0.0, 0.0]
            q[a] = v
            q[(a + 1) % 3] = 3.25 + j % 2
            q[(a + 2) % 3] = 2.75 + j % 3
            bad.append(q)
    bad = np.array(bad)
    out, at = [], np.linspace(0, len(p), len(bad)).astype(int)  # the first one in front of everything, the last one behind
    for i in range(len(p) + 1):
        out += [bad[k] for k in np.nonzero(at == i)[0]]
        if i < len(p):
            out.append(p[i])
    return np.array(out), kw


KERNEL_EDGE_SITES = ("at_extent", "beyond", "inside", "beyond_pair", "grid_point", "coincident", "coincident", "weightless",
                     "inside_pair")


def _kernel_edge():
    """Lone particles, one per site (two at `coincident`), the sites 4 cells apart: no grid point sees two sites. Extent 0.625 =
    |(0.5, 0.375, 0)|. `at_extent` sits exactly that far from its two nearest grid points and farther from all others: w = 1 - 1 = 0,
    every point that sees it is 0 / 0. `beyond` and `inside` sit at (0.5, 0.375, 0) (1 +- 2^-30) from a grid point, extent x (1 +- 2^-30)
    exactly: w^3 of 6e-27 is the only weight `inside` has anywhere; `beyond` has none at that point and 1e-28 at the next point along
    x, which it has come closer to. No position is at extent x (1 +- 2^-30) from TWO grid points and
    representable, so `beyond_pair` and `inside_pair` are the nearest there is: (0.5, 0.375 +- 2^-30, 0) from two points, 0.625 (1 +-
    0.96 2^-30): no weight at all, and the same w^3 of 5e-27 as the only weight of either point. `grid_point` lies on a grid point
    (value exactly - r), `weightless` in a cell centre (0.87 from every point)."""
    kw = _settings((17, 9, 5), 2, 0.625, 0.25)
    e = 2.0 ** -30
    c = np.array([[2.5, 2.375, 2.0],
                  [6.0 + 0.5 * (1 + e), 2.0 + 0.375 * (1 + e), 2.0],
                  [10.0 + 0.5 * (1 - e), 2.0 + 0.375 * (1 - e), 2.0],
                  [14.5, 2.375 + e, 2.0],
                  [2.0, 6.0, 2.0],
                  [6.25, 6.25, 2.0],
                  [6.25, 6.25, 2.0],
                  [10.5, 6.5, 2.5],
                  [14.5, 6.375 - e, 2.0]])
    return _world(c, kw), kw


def _radii(radius):
    kw = _settings((20, 11, 9), radius, 0.9 * radius, 0.5)  # a ragged 3 x 2 x 2 grid of 8^3 blocks
    return _world(_lattice(np.random.default_rng(32), -1.0, np.array(kw["size"]) + 1.0, 600), kw), kw


def _block_gaps(radius, variant):
    """Particles in one 8^3 block of a 26^3 grid (blocks 0, 1, 2 and a ragged fourth of two cells per axis): every other block flag
    stays 0, so a grid point's value depends on the pre-check of k_sample_surface finding that one block wherever it lies among the
    blocks the neighbourhood overlaps."""
    kw = _settings((26, 26, 26), radius, 0.75 * radius, 0.5)
    b = np.array(GAP_BLOCKS[variant], dtype=np.float64)
    lo = np.maximum(8.0 * b, 1.0)  # (cells with an index 0 keep nothing)
    return _world(_lattice(np.random.default_rng(33), lo, 8.0 * b + 8.0, 40), kw), kw


HEAVY = {"heavy": ((5, 5, 5), 3000), "beside": ((6, 5, 5), 257), "single": ((5, 7, 5), 1)}


def _heavy_cells():
    """One cell of 3 000 particles on a 2^-16 lattice (64 of them coincident in pairs), a cell of 257 beside it, a cell of 1, all
    other cells empty; shuffled: k_sort_groups (one thread per cell) has real work, and the sums are order dependent."""
    kw = _settings((12, 12, 12), 3, 2.0, 0.5)
    rng = np.random.default_rng(34)
    parts = []
    for cell, n in HEAVY.values():
        distinct = n - 32 if n == 3000 else n
        k = rng.choice(65536 ** 3, size=distinct, replace=False)
        c = np.stack([k % 65536, (k // 65536) % 65536, k // 65536 ** 2], axis=1) * 2.0 ** -16 + np.array(cell, dtype=np.float64)
        parts.append(np.concatenate([c, c[:n - distinct]]))
    c = np.concatenate(parts)
    return _world(c[rng.permutation(len(c))], kw), kw


def _scan_edges_cloud(ncell):
    """Every cell with all indices > 0 holds (cell index mod 3) particles, the last cell at least one. Grids with an extent of 1
    (257, 2 047 and 2 049 cells have no other factorisation) keep no particle: every cell start is 0 and every value 1."""
    kw = _settings(SCAN_COUNTS[ncell], 2, 1.5, 0.5)
    nx, ny, nz = kw["size"]
    rng = np.random.default_rng(35)
    cells = []
    for c in range(ncell):
        x, y, z = c % nx, (c // nx) % ny, c // (nx * ny)
        if x > 0 and y > 0 and z > 0:
            cells += [(x, y, z)] * (max(c % 3, 1) if c == ncell - 1 else c % 3)
    cells = np.array(cells, dtype=np.float64).reshape(-1, 3)
    c = cells + _lattice(rng, 0.0, 1.0, len(cells))
    return _world(c[rng.permutation(len(c))], kw), kw


def _wide_sheet():
    """1025 x 1025 x 2 = 2 101 250 cells: 1 027 scan blocks, two per thread of k_scan_block_sums."""
    kw = _settings((1025, 1025, 2), 1, 1.0, 0.5)
    return _world(_lattice(np.random.default_rng(36), (1.0, 1.0, 1.0), (1025.0, 1025.0, 2.0), 200000), kw), kw


def _offgrid(radius):
    """The non-dyadic case: the shape of test_oracle_matches_live_reference, here also at cell_radius 1 and 4."""
    kw = _settings((9, 8, 10), radius, 1.3, 0.45, 0.7, (0.3, -0.2, 0.1))
    return np.random.default_rng(37).uniform(-0.4, 7.5, size=(900, 3)), kw


@functools.lru_cache(maxsize=None)
def _cloud(cid):
    name, *arg = cid.split("-")
    if name == "cell_faces":
        return _cell_faces(1.0, (0.0, 0.0, 0.0))
    if name == "cell_faces_h05":
        return _cell_faces(0.5, (0.25, -1.5, 3.0))
    if name == "unrepresentable":
        return _unrepresentable()
    if name == "kernel_edge":
        return _kernel_edge()
    if name == "radii":
        return _radii(int(arg[0]))
    if name == "block_gaps":
        return _block_gaps(int(arg[0]), arg[1])
    if name == "heavy_cells":
        return _heavy_cells()
    if name == "scan_edges":
        return _scan_edges_cloud(int(arg[0]))
    if name == "wide_sheet":
        return _wide_sheet()
    if name == "offgrid":
        return _offgrid(int(arg[0]))
    raise KeyError(cid)


def cloud(cid):
    p, kw = _cloud(cid)
    return p.copy(), dict(kw)


# ------------------------------------------------------------------------------------------------------------ fields
EXTREME_VALUES = np.array([0.0, -0.0, 4.9e-324, -4.9e-324, 2.0 ** -1022, -2.0 ** -1022, 1.0, -1.0, 1e308, -1e308, np.inf, -np.inf,
                           np.nan])
# how often each is drawn: the infinities and NaN stay rare, so that most vertices are finite (asserted on the CPU)
EXTREME_WEIGHTS = np.array([3, 3, 3, 4, 3, 4, 3, 4, 3, 4, 0.6, 0.6, 0.8])
_FIELD_GRID = dict(grid_offset=(0.25, -1.5, 3.0), cell_size=0.5)


def _extremes():
    rng = np.random.default_rng(41)
    v = rng.choice(EXTREME_VALUES, size=(5, 6, 7), p=EXTREME_WEIGHTS / EXTREME_WEIGHTS.sum())
    return v, dict(size=(6, 5, 4), **_FIELD_GRID)


TIE_ROW = np.array([1.0, 1.0 + 2.0 ** -52, 1.0, 1.0 - 2.0 ** -52, 1.0, 1.0 + 2.0 ** -52])
RATIO_ROW = np.array([1.0, 2.0 ** -60, 1.0, 2.0 ** -1000, 1.0, 2.0 ** -60])


def _near_ties():
    """A checkerboard of signs (every edge carries a vertex); along x the magnitudes of neighbours are a (1, 1 +- 2^-52) in the even
    rows and differ by 2^-60 or 2^-1000 in the odd ones, both ways round."""
    rng = np.random.default_rng(42)
    z, y, x = np.indices((6, 6, 6))
    a = rng.choice([0.75, 1.0, 1.5, 3.0], size=(6, 6, 1))
    mag = a * np.where((y + z) % 2 == 0, TIE_ROW[x], RATIO_ROW[x])
    return np.where((x + y + z) % 2 == 0, -mag, mag), dict(size=(5, 5, 5), **_FIELD_GRID)


def _random_signs(rng, shape, p_negative):
    mag = rng.integers(256, 1024, size=shape) * 2.0 ** -10
    return np.where(rng.random(shape) < p_negative, -mag, mag)


def _scan_edges_field(ncell):
    """Random signs, magnitudes on a 2^-10 lattice; the last grid point is inside and its three neighbours outside, so the last cell
    creates its three own vertices."""
    nx, ny, nz = SCAN_COUNTS[ncell]
    v = _random_signs(np.random.default_rng(43), (nz + 1, ny + 1, nx + 1), 0.5)
    v[-1, -1, -1] = -abs(v[-1, -1, -1])
    for s in ((-1, -1, -2), (-1, -2, -1), (-2, -1, -1)):
        v[s] = abs(v[s])
    return v, dict(size=(nx, ny, nz), **_FIELD_GRID)


def _wide_sheet_field():
    """2049 x 1025 x 1 = 2 100 225 cells (per = 2): one grid point in 96 is inside, about one cell in 12 has such a corner."""
    return _random_signs(np.random.default_rng(44), (2, 1026, 2050), 1.0 / 96.0), dict(size=(2049, 1025, 1), **_FIELD_GRID)


@functools.lru_cache(maxsize=None)
def _field(fid):
    name, *arg = fid.split("-")
    if name == "extremes":
        return _extremes()
    if name == "near_ties":
        return _near_ties()
    if name == "scan_edges":
        return _scan_edges_field(int(arg[0]))
    if name == "wide_sheet_field":
        return _wide_sheet_field()
    raise KeyError(fid)


def field(fid):
    v, kw = _field(fid)
    return v.copy(), dict(kw)


def results(cid, kind, is_field=False):
    """(values, positions, indices) of a cloud or field from the oracle (kind="oracle") or the compiled reference (kind="ref")."""
    from oracle import loader as orc
    if is_field:
        v, kw = field(cid)
        return (v, *orc.mesher_mesh(None, values=v, kind=kind, **kw))
    p, kw = cloud(cid)
    v = orc.mesher_surface(p, kind=kind, **kw)
    return (v, *orc.mesher_mesh(p, kind=kind, **kw))


def summary(values, pos, idx):
    """What tests/golden/mesher_edges.npz keeps of a result: (counts int64[4]: points, NaN points, vertices, indices; uint8[3, 32]:
    SHA-256 of the value, position and index bytes, every NaN replaced by the one default quiet NaN first)."""
    import hashlib
    sha = [np.frombuffer(hashlib.sha256(np.where(np.isnan(a), np.nan, a).astype("<f8").tobytes()).digest(), dtype=np.uint8)
           for a in (values, pos)]
    sha.append(np.frombuffer(hashlib.sha256(np.ascontiguousarray(idx, dtype="<u8").tobytes()).digest(), dtype=np.uint8))
    return np.array([values.size, np.isnan(values).sum(), len(pos), len(idx)], dtype=np.int64), np.stack(sha)


# ------------------------------------------------------------------------------------- what the cases hold, in numpy
KEPT, INDEX0, OUTSIDE = 0, 1, 2


def particle_indices(p, kw):
    """(index float64[n, 3], class int[n]) as particle_cell decides: truncation toward zero; OUTSIDE when an axis has no index an
    int can hold or one outside [0, n), else INDEX0 when an index is 0 (the reference's `> 0`), else KEPT."""
    n = np.asarray(kw["size"], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc((np.asarray(p) - np.asarray(kw["grid_offset"])[None, :]) / kw["cell_size"])
        ok = np.isfinite(t) & (np.abs(t) < 2.0 ** 31)
        outside = (~ok | (t < 0) | (t >= n[None, :])).any(axis=1)
        cls = np.where(outside, OUTSIDE, np.where((t == 0).any(axis=1), INDEX0, KEPT))
    return t, cls


def kept_cells(p, kw):
    """Linear cell index (x fastest) of the kept particles, in input order."""
    t, cls = particle_indices(p, kw)
    t = t[cls == KEPT].astype(np.int64)
    return t[:, 0] + kw["size"][0] * (t[:, 1] + kw["size"][1] * t[:, 2])


def weights(p, kw):
    """Brute force over (grid point, kept particle), for small cases: sees bool[points, particles] (the particle's cell lies in the
    point's neighbourhood [g - R, g + R - 1]), w float64[points, particles] (mesher::_kernel with the device's operation order),
    sq float64[points, particles]; points in storage order (x fastest)."""
    t, cls = particle_indices(p, kw)
    q, c = np.asarray(p)[cls == KEPT], t[cls == KEPT]
    nx, ny, nz = kw["size"]
    gz, gy, gx = np.indices((nz + 1, ny + 1, nx + 1)).reshape(3, -1)
    g = np.stack([gx, gy, gz], axis=1).astype(np.float64)
    R = kw["cell_radius"]
    sees = ((c[None, :, :] >= g[:, None, :] - R) & (c[None, :, :] <= g[:, None, :] + R - 1)).all(axis=2)
    d = q[None, :, :] - (np.asarray(kw["grid_offset"])[None, :] + kw["cell_size"] * g)[:, None, :]
    sq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    w = 1.0 - sq / (kw["particle_extent"] * kw["particle_extent"])
    return sees, np.where(w > 0.0, w * w * w, 0.0), sq


def point_census(p, kw):
    """(points that come out NaN: they see a particle and every weight is 0; points with value exactly - r: a particle on the point
    carries the only weight; points with a finite value: a positive weight), for small cases."""
    sees, w, sq = weights(p, kw)
    seen, tw = sees.any(axis=1), np.where(sees, w, 0.0).sum(axis=1)
    hit = (sees & (sq == 0.0)).any(axis=1) & ((sees & (w > 0.0)).sum(axis=1) == (sees & (sq == 0.0)).sum(axis=1))
    return int((seen & (tw == 0.0)).sum()), int(hit.sum()), int((seen & (tw > 0.0)).sum())


def block_kinds(kw, block):
    """For every grid point (storage order) and axis, where `block` (8^3 cells) lies among the blocks the point's neighbourhood
    overlaps: 'L' the lowest one (or the only one), 'M' between lowest and highest, 'H' the highest (and not the lowest), '-' none.
    char[points, 3]."""
    R, out = kw["cell_radius"], []
    for a in range(3):
        n = kw["size"][a]
        g = np.arange(n + 1)
        lo, hi = np.maximum(g - R, 0) >> 3, (np.minimum(g + R, n) - 1) >> 3  # (hi >= lo: a neighbourhood is never empty for R >= 1)
        b = block[a]
        out.append(np.where((b < lo) | (b > hi), "-", np.where(b == lo, "L", np.where(b == hi, "H", "M"))))
    kz, ky, kx = np.meshgrid(out[2], out[1], out[0], indexing="ij")
    return np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1)


def grid_edges(values):
    """Every edge of the point grid as the cell that creates its vertex sees it: (v1, v2, owner) per direction x, y, z, flattened.
    An edge belongs to the cell at (index - 1, clamped to 0) across it, as its edge 5, 6 or 10 or, on the low faces, 0 .. 4, 7 .. 9, 11;
    those run from the low to the high end except the x edges off the y = 0 face and the y edges on the x = 0 face (edges 2, 6 and
    3, 7 of mc_tables.h). owner: linear cell index, the order the vertices are numbered in."""
    v = np.asarray(values)
    pz, py, px = v.shape
    nx, ny = max(px - 1, 1), max(py - 1, 1)
    z, y, x = np.indices(v.shape)
    own = lambda cx, cy, cz: cx + nx * (cy + ny * cz)  # noqa: E731
    m1 = lambda a: np.maximum(a - 1, 0)  # noqa: E731
    out = []
    lo, hi, flip = v[:, :, :-1], v[:, :, 1:], (y[:, :, :-1] > 0)
    out.append((np.where(flip, hi, lo).ravel(), np.where(flip, lo, hi).ravel(), own(x, m1(y), m1(z))[:, :, :-1].ravel()))
    lo, hi, flip = v[:, :-1, :], v[:, 1:, :], (x[:, :-1, :] == 0)
    out.append((np.where(flip, hi, lo).ravel(), np.where(flip, lo, hi).ravel(), own(m1(x), y, m1(z))[:, :-1, :].ravel()))
    out.append((v[:-1].ravel(), v[1:].ravel(), own(m1(x), m1(y), z)[:-1].ravel()))
    return out


def vertex_edges(values):
    """(v1, v2, owner) of the edges that carry a vertex (`f < 0` differs between the ends), all directions together."""
    v1, v2, own = (np.concatenate(a) for a in zip(*grid_edges(values)))
    keep = (v1 < 0) != (v2 < 0)
    return v1[keep], v2[keep], own[keep]


def cell_cases(values):
    """Case byte of every cell (bit i: corner i of mc_tables.h is inside), uint8[nz, ny, nx]."""
    v = np.asarray(values) < 0
    corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    nz, ny, nx = (s - 1 for s in v.shape)
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    for i, (dx, dy, dz) in enumerate(corners):
        occ |= v[dz:dz + nz, dy:dy + ny, dx:dx + nx].astype(np.uint8) << i
    return occ
