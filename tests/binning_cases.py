"""Designed clouds and grids for the binning (core.hip: k_tile_count, k_tile_flags, k_tile_scatter, k_gather_vc, k_cell_count,
k_dilate_slots, lfa_exclusive_scan_u32; common.h: lfa_wave_tile_ranks; particles.hip: k_advect_collide_count), and a numpy model of
what a binning must leave behind, whatever the order inside a tile. Pure numpy, deterministic from fixed seeds; every builder returns
(size, parts, solid, meta) with meta = dict(h=cell size, off=grid offset, ...).

Every case is DYADIC: a position is off + (cell + k / 16) h with an integer cell, k in 0 .. 15 (16 only on a max face of the grid),
h in {1, 0.5} and an offset that is a multiple of 1/8. So (p - off) / h and its floor are exact in fp64 - in the reference, the oracle,
numpy and k_ingest alike -, the fp32 fraction k / 16 is exact, and the position a download rebuilds, off + (cell + t) h, is the
uploaded one bit for bit.

Every particle carries its upload index i (which is its id on the device) in numbers that are exact in fp32: vel = (i, i mod 1024 -
512, i div 1024) and C[k] = ((k + 2) i + k) mod 65521 with cx[0] = i. A record that ends up under a wrong id - a slot written twice
or never, a from[] of another particle, a C taken from the wrong home - is then visibly wrong; no comparison needs a tolerance.

  round_robin            upload i lies in tile (stride i) mod 512 of a 64^3 grid: a wave of k_tile_count (8 x 64 consecutive
                         particles) sees 512 distinct tiles, one round of lfa_wave_tile_ranks (common.h:460) each; n on the edges
                         of the wave (512) and of the workgroup (2 048, core.hip:1154)
  two_tiles_alternating  lanes alternate between two tiles: `base += popcll(same[c])` (common.h:484) carries a tile's rank base
                         across all 8 chunks, and many waves and workgroups add to the same two counters (common.h:479)
  one_tile_prime         1 000 003 particles in the one tile of an 8^3 grid: `cnt % 1000003u != 0` (core.hip:989) is false for
                         the first time; its twin holds 1 000 002 and is shuffled
  singletons             one particle per corner, edge-centre and interior tile: k_dilate_slots' clipping (core.hip:1074) and
                         n_dtiles; ragged grids, where the last tile is cut
  scan_tiles             grids whose tile count nt puts the two scanned lengths, nt + 1 (tile_start, core.hip:1160) and nt (the
                         flags, core.hip:1081), on the boundaries between k_scan_local, k_scan_serial and reduce / recurse / local
                         (core.hip:119-137)
  scan_recursion         4 300 800 cells: lfa_number_unknowns (core.hip:1306) scans one entry per cell, 2 100 blocks, so the inner
                         scan of the block sums (core.hip:133) is k_scan_serial and no longer one launch
  with_solids            particles inside solid cells: counted, and listed by _fluid_cells like every other cell that holds one
"""
import functools
import itertools

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE

TILE = 8
TILE_CELLS = 512
PRIME = 1000003             # core.hip:989, the multiplier of k_tile_scatter's shuffle
WAVE_PARTICLES = 8 * 64     # common.h:449, TC_CHUNKS x 64: what one wave of k_tile_count ranks
GROUP_PARTICLES = 256 * 8   # core.hip:1154, 256 * TC_CHUNKS: what one workgroup of k_tile_count takes
SCAN_TILE = 2048            # core.hip:31, SCAN_BS * SCAN_IPT: the entries of one k_scan_local workgroup
SCAN_SERIAL_MAX = 8192      # core.hip:93, 4 * SCAN_TILE: the longest scan k_scan_serial takes
OFF_DYADIC = (0.25, -0.5, 1.125)


def scan_form(n):
    """Which of its forms lfa_exclusive_scan_u32 takes for n entries (scan_rec, core.hip:118-138): 'none' (n = 0, core.hip:141),
    'local' (one k_scan_local launch, core.hip:125), 'serial' (k_scan_serial, core.hip:120) or 'reduce+<form of the block sums>'."""
    if n == 0:
        return "none"
    nb = -(-n // SCAN_TILE)
    if nb > 1 and n <= SCAN_SERIAL_MAX:
        return "serial"
    if nb == 1:
        return "local"
    return "reduce+" + scan_form(nb)


def tiles_of(size):
    return tuple(-(-int(s) // TILE) for s in size)


def identity(n):
    """(vel float64[n, 3], C float64[n, 9]) that name upload index i; integers below 2^24."""
    i = np.arange(n, dtype=np.int64)
    vel = np.stack([i, i % 1024 - 512, i // 1024], axis=1).astype(np.float64)
    c = np.stack([((k + 2) * i + k) % 65521 for k in range(9)], axis=1).astype(np.float64)
    c[:, 0] = i
    assert np.abs(vel).max(initial=0) < 2 ** 24 and np.abs(c).max(initial=0) < 2 ** 24
    return vel, c


def c_of(parts):
    return np.concatenate([parts["cx"], parts["cy"], parts["cz"]], axis=1)


def _cloud(size, cell, k16, h=1.0, off=(0.0, 0.0, 0.0), solid=None, **meta):
    size = tuple(int(s) for s in size)
    cell = np.asarray(cell, dtype=np.int64).reshape(-1, 3)
    k16 = np.asarray(k16, dtype=np.int64).reshape(-1, 3)
    n = len(cell)
    assert len(k16) == n and ((cell >= 0) & (cell < np.asarray(size))).all()
    assert ((k16 >= 0) & (k16 <= 16)).all() and (cell[k16 == 16] == np.broadcast_to(np.asarray(size) - 1, cell.shape)[k16 == 16]).all()
    assert h in (1.0, 0.5) and all(float(o * 8).is_integer() for o in off)
    parts = np.zeros(n, dtype=PARTICLE_DTYPE)
    parts["pos"] = np.asarray(off, dtype=np.float64)[None, :] + (cell + k16 / 16.0) * h
    parts["old_pos"] = parts["pos"]
    vel, c = identity(n)
    parts["vel"] = vel
    parts["cx"], parts["cy"], parts["cz"] = c[:, 0:3], c[:, 3:6], c[:, 6:9]
    if solid is not None:
        solid = np.unique(np.asarray(solid, dtype=np.int32).reshape(-1, 3), axis=0)
    return size, parts, solid, dict(h=float(h), off=tuple(float(o) for o in off), cell=cell, k16=k16, **meta)


# ---------------------------------------------------------------------------------------------------- the model
def model(size, pos, h=1.0, off=(0.0, 0.0, 0.0), solid=None):
    """What a binning of particles at `pos` leaves (src/simulation.cpp:251-291 for the cells; the tiles are the device's):
      raw              uint64[n]   x-fastest index of each particle's clamped cell
      tile             int64[n]    its 8^3 tile, x fastest among the tiles (common.h:327)
      tile_counts      int64[nt]   particles per tile
      counts           uint32[nc]  particles per cell, x fastest
      fluid_cells      uint64[]    ascending raw indices of the cells that hold a particle - solid or not: _fluid_cells is filled
                                   from the particles alone (src/simulation.cpp:277, 284); the solver drops the solid ones later (:90)
      fluid_not_solid  uint64[]    those of them that are not solid
      particle_tiles   int         tiles that hold a particle
      processed_tiles  int         tiles in the union of their 27-neighbourhoods, clipped to the grid (core.hip:1067-1077)"""
    n3 = np.asarray(size, dtype=np.int64)
    g = (np.asarray(pos, dtype=np.float64).reshape(-1, 3) - np.asarray(off, dtype=np.float64)) / np.float64(h)
    idx = np.minimum(np.maximum(g, 0.0).astype(np.int64), n3 - 1)
    raw = idx[:, 0] + n3[0] * (idx[:, 1] + n3[1] * idx[:, 2])
    ntx, nty, ntz = tiles_of(size)
    t3 = idx >> 3
    tile = t3[:, 0] + ntx * (t3[:, 1] + nty * t3[:, 2])
    tile_counts = np.bincount(tile, minlength=ntx * nty * ntz)
    counts = np.bincount(raw, minlength=int(n3.prod())).astype(np.uint32)
    fluid = np.flatnonzero(counts).astype(np.uint64)
    is_solid = np.zeros(int(n3.prod()), dtype=bool)
    if solid is not None and len(solid):
        s = np.asarray(solid, dtype=np.int64)
        is_solid[s[:, 0] + n3[0] * (s[:, 1] + n3[1] * s[:, 2])] = True
    occupied = (tile_counts > 0).reshape(ntz, nty, ntx)
    padded = np.zeros((ntz + 2, nty + 2, ntx + 2), dtype=bool)
    padded[1:-1, 1:-1, 1:-1] = occupied
    near = np.zeros_like(occupied)
    for dz, dy, dx in itertools.product(range(3), repeat=3):
        near |= padded[dz:dz + ntz, dy:dy + nty, dx:dx + ntx]
    return dict(raw=raw.astype(np.uint64), tile=tile, tile_counts=tile_counts, counts=counts, fluid_cells=fluid,
                fluid_not_solid=fluid[~is_solid[fluid.astype(np.int64)]], particle_tiles=int(occupied.sum()),
                processed_tiles=int(near.sum()))


def model_of(cloud):
    size, parts, solid, meta = cloud
    return model(size, parts["pos"], meta["h"], meta["off"], solid)


# ---------------------------------------------------------------------------------------------------- round_robin
RR_SIZE = (64, 64, 64)
RR_NS = (512, 2047, 2048, 2049, 4096 + 1)
RR_SITES_X = (40, 80, 127)       # sixteenths of a cell inside the tile: 2.5, 5 and 7.9375
RR_SITES_YZ = (24, 80)           # 1.5 and 5


def round_robin(n, stride=1, h=1.0, off=(0.0, 0.0, 0.0)):
    """Upload i lies in tile (stride i) mod 512 of the 8 x 8 x 8 tiles (stride odd: a bijection of every 512 consecutive i), so
    each wave of the first binning holds 512 distinct tiles: lfa_wave_tile_ranks (common.h:460) runs 512 rounds of one particle,
    each with an atomic of its own (common.h:479), and no lane shares a round. stride = 1 is the issue's `i % 512`; stride = 201
    changes the tile LAYER (z) from one lane to the next, so that on two slab ranks split at layer 4 every wave holds the invalid
    keys 0xFFFFFFFF of the other rank's particles (core.hip:546, :940) lane by lane between its own.
    Visit j = i div 512 of tile t takes one of 12 sites: x = {2.5, 5, 7.9375}[(j + t) mod 3], y and z in {1.5, 5} cells from the
    tile's corner by j div 3, plus k / 16, k in 0 .. 3, on y and z: two particles are at least 2.5 - 3/16 cells apart on some axis (next tile's 2.5 is 2.56 from
    7.9375), and stay more than 2 apart after moves of at most 1/8 cell - the correction of a time step moves none of them."""
    assert stride % 2 == 1 and n <= 12 * 512
    i = np.arange(n, dtype=np.int64)
    t = (stride * i) % 512
    j = i // 512
    t3 = np.stack([t % 8, (t // 8) % 8, t // 64], axis=1)
    jit = np.stack([np.zeros(n, dtype=np.int64), (i * 7) % 4, (i * 5 + 1) % 4], axis=1)
    site = np.stack([np.take(RR_SITES_X, (j + t) % 3), np.take(RR_SITES_YZ, (j // 3) % 2), np.take(RR_SITES_YZ, j // 6)], axis=1) + jit
    cell = t3 * 8 + site // 16
    return _cloud(RR_SIZE, cell, site % 16, h, off, stride=stride)


def with_moves(cloud, dt=1.0 / 64):
    """The cloud with velocities that move every particle by a multiple of 1/16 cell, at most 1/8 per axis, in the step dt (exact:
    dt is a power of two) - upload i moves by ((i mod 5) - 2, (i div 5 mod 5) - 2, (i div 25 mod 5) - 2) / 16. The particles at
    x = 7.9375 that move by +1/8 change tiles; in the last tile column they end in the wall's skin instead. cx[0] still names the
    particle (FLIP carries C through a time step). Returns (cloud, dt)."""
    size, parts, solid, meta = cloud
    parts = parts.copy()
    i = np.arange(len(parts), dtype=np.int64)
    m16 = np.stack([i % 5 - 2, (i // 5) % 5 - 2, (i // 25) % 5 - 2], axis=1)
    parts["vel"] = (m16 / 16.0) * (meta["h"] / dt)
    return (size, parts, solid, dict(meta, dt=float(dt), m16=m16)), float(dt)


# ---------------------------------------------------------------------------------------------------- two_tiles_alternating
def two_tiles_alternating(n=6001):
    """24 x 8 x 8 cells = three tiles in a row; upload i lies in tile 0 (i even) or tile 2 (i odd). Every chunk of every wave holds
    32 lanes of each, so a round of lfa_wave_tile_ranks takes 256 particles from all 8 chunks and `base += popcll(same[c])`
    (common.h:484) carries the tile's rank base from chunk to chunk seven times; 12 waves in 3 workgroups add to the same two
    counters (common.h:479), so a wave's base is whatever the atomics of the others left. n is odd: the last wave is cut inside a
    chunk (`i < n`, core.hip:939). The particles cycle through the 512 cells of their tile."""
    i = np.arange(n, dtype=np.int64)
    c = (i // 2 * 37) % 512
    cell = np.stack([(i % 2) * 16 + (c & 7), (c >> 3) & 7, c >> 6], axis=1)
    k16 = np.stack([i % 16, (i // 16) % 16, (i * 3 + 5) % 16], axis=1)
    return _cloud((24, 8, 8), cell, k16, 0.5, OFF_DYADIC)


# ---------------------------------------------------------------------------------------------------- one_tile_prime
def one_tile_prime(n=PRIME):
    """n particles in the single tile of an 8^3 grid, cycling through its 512 cells. With n = 1 000 003 the tile's count is a
    multiple of the shuffle's prime: r -> r 1000003 mod cnt would send every rank to slot 0, and `cnt % 1000003u != 0`
    (core.hip:989) keeps the rank instead. The twin, n = 1 000 002, is shuffled. Every 97th particle lies ON a max face of the grid
    (k = 16 in the last cell of one axis; every 291st on an edge: two axes): its unclamped index equals the size and is clamped
    (common.h:416), its fraction is 1."""
    i = np.arange(n, dtype=np.int64)
    c = i % 512
    cell = np.stack([c & 7, (c >> 3) & 7, c >> 6], axis=1)
    k16 = np.stack([(i // 512) % 16, (i // 8192) % 16, (i * 7 + 3) % 16], axis=1)
    face = np.flatnonzero(i % 97 == 0)
    for a in range(3):
        on = face[((face // 97) % 3 == a) | (((face // 97) % 3 == (a + 1) % 3) & (face % 291 == 0))]
        cell[on, a] = 7
        k16[on, a] = 16
    return _cloud((8, 8, 8), cell, k16, on_face=face)


# ---------------------------------------------------------------------------------------------------- singletons
SINGLETON_SIZES = ((24, 40, 56), (7, 5, 3), (17, 9, 25))


def singleton_tiles(size):
    """Tile coordinates: the 8 corners, the 12 edge centres (two coordinates at an end, one in the middle) and the centre tile -
    fewer where an axis has too few tiles for them to differ."""
    nt = tiles_of(size)
    ends = [sorted({0, n - 1}) for n in nt]
    mid = [n // 2 for n in nt]
    out = set(itertools.product(*ends))
    for a in range(3):
        out |= set(itertools.product(*[[mid[b]] if b == a else ends[b] for b in range(3)]))
    out.add(tuple(mid))
    return sorted(out, key=lambda t: (t[2], t[1], t[0]))


def singletons(size):
    """One particle in each tile of singleton_tiles(size). k_dilate_slots (core.hip:1067-1077) marks the 27 tiles around each and
    clips with `(unsigned)x < (unsigned)g.ntx`: a corner tile keeps 8 of its 27, an edge centre 12, the interior one all 27, and
    the sets overlap - counts()['processed_tiles'] is the size of their union, on 3 x 5 x 7 tiles the whole grid. So the GPU test
    also bins every one of them alone (`lone`), where a neighbour that is not marked is marked by nobody else. In a corner tile the particle sits in the grid's
    corner cell; 7 x 5 x 3 is one cut tile, 17 x 9 x 25 ends in tiles of 1 x 1 x 1 cells."""
    tiles = np.asarray(singleton_tiles(size), dtype=np.int64)
    nt, n3 = np.asarray(tiles_of(size)), np.asarray(size)
    cell = np.where(tiles == nt - 1, n3 - 1, np.where(tiles == 0, 0, tiles * 8 + 3))
    i = np.arange(len(tiles), dtype=np.int64)
    k16 = np.stack([(5 * i + 1) % 16, (3 * i + 2) % 16, (7 * i + 3) % 16], axis=1)
    return _cloud(size, cell, k16, 0.5, OFF_DYADIC, tiles=tiles)


def lone(cloud, i):
    """Particle i of a cloud alone (as particle 0 of a cloud of one): nothing but its own tile marks its neighbours."""
    size, parts, solid, meta = cloud
    return _cloud(size, meta["cell"][i], meta["k16"][i], meta["h"], meta["off"], solid)


# ---------------------------------------------------------------------------------------------------- scan_tiles
# nt -> cells. 8 191 is prime: a grid has nt = ntx nty ntz with every factor <= 512, so no grid has 8 191 tiles - the lengths
# 8 191 = 8 190 + 1 and 8 192 are reached from their neighbours (8 192 as a flag scan, 8 193 = 8 192 + 1 as the first reduce).
SCAN_GRIDS = {
    2046: (528, 248, 8),    # 66 x 31 x 1
    2047: (184, 712, 8),    # 23 x 89 x 1
    2048: (128, 128, 64),   # 16 x 16 x 8
    8190: (720, 728, 8),    # 90 x 91 x 1
    8192: (128, 128, 256),  # 16 x 16 x 32
}
# (form of the tile_start scan over nt + 1 entries, form of the flag scan over nt entries)
SCAN_FORMS = {
    2046: ("local", "local"),
    2047: ("local", "local"),
    2048: ("serial", "local"),
    8190: ("serial", "serial"),
    8192: ("reduce+local", "serial"),
}


def scan_tiles(nt):
    """A seeded half of the nt tiles of SCAN_GRIDS[nt] hold one to three particles each, so that neither scanned array is constant;
    always the first tile, the last, and the tiles 2 048 k - 1 and 2 048 k on either side of every block boundary of the scans
    (SCAN_TILE, core.hip:31: where k_scan_local adds block_offsets, core.hip:83, and k_scan_serial its carry, core.hip:112).
    tile_start is the scan of nt + 1 counts (core.hip:1160), the tile lists come from scans of nt flags (core.hip:1081): with
    nt = 2 046, 2 047, 2 048, 8 190, 8 192 the two lengths lie on every side of 2 048 and 8 192. The upload order is shuffled."""
    size = SCAN_GRIDS[nt]
    ntx, nty, ntz = tiles_of(size)
    assert ntx * nty * ntz == nt and max(size) <= 4096
    rng = np.random.default_rng(7000 + nt)
    chosen = rng.random(nt) < 0.5
    forced = {0, nt - 1} | {t for b in range(SCAN_TILE, nt + 1, SCAN_TILE) for t in (b - 1, b) if t < nt}
    chosen[sorted(forced)] = True
    tiles = np.repeat(np.flatnonzero(chosen), rng.integers(1, 4, size=int(chosen.sum())))
    tiles = tiles[rng.permutation(len(tiles))]
    n = len(tiles)
    t3 = np.stack([tiles % ntx, (tiles // ntx) % nty, tiles // (ntx * nty)], axis=1)
    cell = t3 * 8 + rng.integers(0, 8, size=(n, 3))
    return _cloud(size, cell, rng.integers(0, 16, size=(n, 3)), forced=sorted(forced), chosen=chosen)


# ---------------------------------------------------------------------------------------------------- scan_recursion
RECURSION_SIZE = (168, 160, 160)  # 21 x 20 x 20 = 8 400 tiles, 4 300 800 cells


def scan_recursion():
    """The one scan above 2 048 x 2 048 = 4 194 304 entries, reached through lfa_number_unknowns (core.hip:1299-1312; fluid_cells()
    and counts()['unknowns'] call it): it scans one 0 / 1 flag per CELL in raw order, here 4 300 800 of them = 2 100 blocks, so the
    scan of the block sums (core.hip:133) is k_scan_serial over two tiles where every smaller grid has one k_scan_local launch. A
    particle lies in the first cell, in the last, in the cells 2 048 k - 1 and 2 048 k around every block boundary (k = 2 048:
    the boundary between the two tiles of the inner scan) and in 3 000 seeded cells, a quarter of which hold two: the flags are
    a designed 0 / 1 pattern and out[raw_scan[r]] = r (core.hip:1325) is the ascending list of the model. With 8 400 tiles the
    tile arrays take reduce / local as well."""
    size = RECURSION_SIZE
    nc = size[0] * size[1] * size[2]
    rng = np.random.default_rng(4300800)
    k = np.arange(1, -(-nc // SCAN_TILE), dtype=np.int64) * SCAN_TILE
    raw = np.unique(np.concatenate([[0, nc - 1], k - 1, k, rng.integers(0, nc, size=3000)]))
    raw = np.concatenate([raw, raw[rng.random(len(raw)) < 0.25]])
    raw = raw[rng.permutation(len(raw))]
    cell = np.stack([raw % size[0], (raw // size[0]) % size[1], raw // (size[0] * size[1])], axis=1)
    return _cloud(size, cell, rng.integers(0, 16, size=(len(raw), 3)), scanned=nc)


# ---------------------------------------------------------------------------------------------------- with_solids
def with_solids():
    """19 x 16 x 11 cells, h = 0.5, a solid block [4, 9) x [3, 8) x [2, 10) and a solid plate z = 0. 240 seeded particles, every
    third inside a solid cell. The hash counts them like any other (src/simulation.cpp:266-291), and _fluid_cells lists their
    cells too: it is filled from the particles alone (:277, :284), cell types play no part until the solver skips solid entries
    (:90). k_raw_unknown_flags (core.hip:1295) must not look at `solid` either."""
    size = (19, 16, 11)
    rng = np.random.default_rng(1911)
    solid = [(x, y, z) for x in range(4, 9) for y in range(3, 8) for z in range(2, 10)]
    solid += [(x, y, 0) for x in range(size[0]) for y in range(size[1])]
    solid = np.asarray(solid, dtype=np.int64)
    n = 240
    cell = np.stack([rng.integers(0, s, size=n) for s in size], axis=1)
    inside = np.arange(n) % 3 == 0
    cell[inside] = solid[rng.integers(0, len(solid), size=int(inside.sum()))]
    return _cloud(size, cell, rng.integers(0, 16, size=(n, 3)), 0.5, OFF_DYADIC, solid=solid, inside=inside)


# ---------------------------------------------------------------------------------------------------- the cases by name
CASES = {f"round_robin_n{n}": functools.partial(round_robin, n) for n in RR_NS}
CASES["round_robin_h05_n2049"] = functools.partial(round_robin, 2049, 1, 0.5, OFF_DYADIC)
CASES["round_robin_stride201_n4097"] = functools.partial(round_robin, 4097, 201)
CASES["two_tiles_alternating"] = two_tiles_alternating
CASES.update({"singletons_%dx%dx%d" % s: functools.partial(singletons, s) for s in SINGLETON_SIZES})
CASES.update({f"scan_tiles_nt{nt}": functools.partial(scan_tiles, nt) for nt in SCAN_GRIDS})
CASES["scan_recursion"] = scan_recursion
CASES["with_solids"] = with_solids
CASES["one_tile_prime"] = one_tile_prime
CASES["one_tile_prime_twin"] = functools.partial(one_tile_prime, PRIME - 1)

NAMES = tuple(CASES)
PRIMES = ("one_tile_prime", "one_tile_prime_twin")                     # 152 MB each way: run once
SMALL = tuple(n for n in NAMES if n not in PRIMES)
ROUND_ROBIN = tuple(n for n in NAMES if n.startswith("round_robin"))
REBIN = ROUND_ROBIN + ("two_tiles_alternating",)                        # binning on top of binning
GOLDEN = PRIMES + tuple(n for n in NAMES if n.startswith("scan_"))     # kept as counts and digests in tests/golden/binning.npz


@functools.lru_cache(maxsize=None)
def build(name):
    """(size, parts, solid, meta) of a case; cached and read-only - callers copy `parts` before they change it."""
    size, parts, solid, meta = CASES[name]()
    parts.setflags(write=False)
    return size, parts, solid, meta


@functools.lru_cache(maxsize=None)
def expected(name):
    """model_of(build(name)), computed once and shared; read-only."""
    out = model_of(build(name))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- the CPU side
def run_cpu(cloud, kind="oracle"):
    """hash() on the oracle or the compiled reference: (raw index per upload index, counts uint32[nc], _fluid_cells)."""
    from oracle import loader as orc
    size, parts, solid, meta = cloud
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=orc.APIC, kind=kind)
    if solid is not None:
        s.set_solid_cells(solid)
    s.set_particles(parts)
    s.hash()
    after = s.particles()
    counts = s.space_hash()[1].astype(np.uint32)
    fluid = s.fluid_cells()
    s.close()
    ids = np.rint(after["cx"][:, 0]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(len(parts)))
    raw = np.empty(len(parts), dtype=np.uint64)
    raw[ids] = after["raw"]
    return raw, counts, fluid


def summary(raw, counts, fluid):
    """(int64[4]: particles, occupied cells, largest count, cells of the grid; uint8[3, 32]: SHA-256 of the three arrays' bytes)."""
    import hashlib
    arrays = (np.ascontiguousarray(raw, dtype="<u8"), np.ascontiguousarray(counts, dtype="<u4"), np.ascontiguousarray(fluid, dtype="<u8"))
    sha = np.stack([np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8) for a in arrays])
    return np.array([len(raw), len(fluid), int(counts.max(initial=0)), len(counts)], dtype=np.int64), sha
