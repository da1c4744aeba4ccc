"""Fields, right-hand sides and bars for the tile-local and the multilevel MIC(0) preconditioner (tests/multilevel_model.py against
libfluid_amd/csrc/pcg.hip).

FIELDS are those of tests/vcycle_cases.py, unchanged: one or two level-1 blocks each, a level-2 matrix of size 1 or 2. PLATES:

  plate        520 x 8 x 520 (vcycle_cases): 65 x 1 x 65 tiles, 9 x 1 x 9 = 81 level-1 blocks - more than the 64 one workgroup takes,
               so the coarse levels run as k_coarse_apply + k_coarse_top and the fused solve takes its non-embedded branch
  plate_holed  264 x 8 x 264: 33 x 1 x 33 tiles, 5 x 1 x 5 level-1 blocks whose last one along x and z holds a single row of tiles.
               Fluid in y = 0, 1, one particle per cell, at rest. Taken out:
                 - the whole level-1 block (1, 0, 1), x and z in 64 .. 127: 24 of 25 blocks hold unknowns, and from position 6 of the
                   list on a block's list position is not its grid position; 24 blocks are also more than the 8 (fp64) or 16 (fp32)
                   waves of k_coarse_all, so a wave takes several blocks
                 - the tiles (7, 0, 3) - the last tile of block (0, 0, 0) along x: tile (8, 0, 3) of the next block has no -x
                   neighbour, (6, 0, 3) no +x neighbour -, (20, 0, 5) and (12, 0, 27)
                 - a strip one cell wide, z = 200 and x in 130 .. 197: the z faces between the tile rows 24 and 25 carry 0, 4 or 16
                   couplings there (a full face of this plate carries 16: 8 cells by 2 layers)

system(name) is the level-0 system (vcycle_cases.system; plate_holed: the same stages of the oracle), model(name) the
model built from it, rhs(name) the right-hand sides: those of vcycle_cases.rhs and A_tile_constant = A v with v constant per tile
and random between tiles - its answer lives in the coarse space. The plates get random, A_smooth and A_tile_constant only.

Bars (vcycle_cases.F64_REL, F32_BARS, fp32_deviation - the one place of the rule): an fp64 result is held to 1e-10 max |model|, an
fp32 result to 8 d32 with d32 = max |model_float32 - model_float64|, never below half an fp32 ulp of the largest entry.
"""
import functools

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from oracle import loader as orc
from tests import multilevel_model as mm
from tests import stencil_cases as sc
from tests import vcycle_cases as vc
from tests import vcycle_model as vm

DT = vc.DT
FIELDS = vc.FIELDS
PLATES = ("plate", "plate_holed")
HOLED_SIZE = (264, 8, 264)
HOLED_BLOCK = (1, 0, 1)
HOLED_TILES = ((7, 0, 3), (20, 0, 5), (12, 0, 27))
HOLED_STRIP = (200, 130, 197)  # z, x0, x1 (inclusive)
PLATE_LABELS = ("random", "A_smooth", "A_tile_constant")
PRECONDS = (mm.TILED, mm.MULTILEVEL)


def plate_mask(size, block=None, tiles=(), strip=None):
    """bool[nz, ny, nx]: y = 0, 1 without a level-1 block (64 cells along x and z), single tiles and a strip one cell wide."""
    nx, ny, nz = size
    m = np.zeros((nz, ny, nx), dtype=bool)
    m[:, :2, :] = True
    if block is not None:
        m[64 * block[2]: 64 * block[2] + 64, :, 64 * block[0]: 64 * block[0] + 64] = False
    for tx, ty, tz in tiles:
        m[8 * tz: 8 * tz + 8, :, 8 * tx: 8 * tx + 8] = False
    if strip is not None:
        m[strip[0], :, strip[1]: strip[2] + 1] = False
    return m


def particles_of(mask):
    """One particle at rest at the centre of every cell of the mask."""
    z, y, x = np.nonzero(mask)
    parts = np.zeros(len(x), dtype=PARTICLE_DTYPE)
    parts["pos"] = np.stack([x, y, z], axis=1) + 0.5
    parts["old_pos"] = parts["pos"]
    return parts


def holed_mask():
    return plate_mask(HOLED_SIZE, HOLED_BLOCK, HOLED_TILES, HOLED_STRIP)


@functools.lru_cache(maxsize=None)
def build(name):
    """(size, parts, solid cells, meta) of any field here."""
    if name != "plate_holed":
        return vc.build(name)
    parts = particles_of(holed_mask())
    parts.setflags(write=False)
    return HOLED_SIZE, parts, None, dict(h=1.0, off=(0.0, 0.0, 0.0), rho=1.0)


def a_scale(name):
    return DT if name == "plate_holed" else vc.a_scale(name)


@functools.lru_cache(maxsize=None)
def system(name):
    """vcycle_cases.system; plate_holed: the same stages on the oracle (hash, P2G, gravity, build_system on the fp32-rounded grid,
    solve - 130 680 unknowns: half a second). tests/test_multilevel_model.py holds vcycle_cases.plate_system_of to it."""
    if name != "plate_holed":
        return vc.system(name)
    size, parts, _, meta = build(name)
    s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=sc.APIC, blending=1.0, density=meta["rho"])
    s.set_particles(parts)
    s.hash()
    out = dict(size=size, fluid_cells=s.fluid_cells(), counts=s.space_hash()[1].astype(np.uint32))
    s.p2g()
    s.add_gravity(DT)
    cells = s.cells()
    cells["vel"] = sc.f32(cells["vel"])
    s.set_cells(cells)
    out["type"], out["vel"] = cells["type"].copy(), cells["vel"].copy()
    s.build_system(DT)
    out["abits"], out["b"] = s.abits(), s.b()
    p, res, it = s.solve(DT)
    out["p"], out["iters"] = p.copy(), int(it)
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def model(name, mutant=None):
    w = system(name)
    return mm.Model(w["size"], w["fluid_cells"], w["abits"], a_scale(name), mutant=mutant)


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    """The V-cycle model's hierarchy of the field (vcycle_model.apply_a reads its level 0)."""
    if name != "plate_holed":
        return vc.model(name)
    w = system(name)
    ptiles, closed = vc.tiles_of(w)
    return vm.hierarchy(w["size"], w["fluid_cells"], w["abits"], w["type"], w["counts"], None, ptiles, closed, a_scale(name))


def tile_constant(name, seed=13):
    M = model(name)
    return np.random.default_rng(seed + M.coarse.n1).normal(size=M.coarse.n1)[M.coarse.tile]


@functools.lru_cache(maxsize=None)
def rhs(name, seed=7):
    """label -> right-hand side (read-only)."""
    M = model(name)
    if name in PLATES:
        out = {"random": np.random.default_rng(seed + M.n).normal(size=M.n), "A_smooth": M.apply_a(vc._smooth(system(name)))}
    else:
        out = dict(vc.rhs(name))
    out["A_tile_constant"] = M.apply_a(tile_constant(name))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- references and bars
@functools.lru_cache(maxsize=None)
def reference(name, label, precond):
    """(z, d32) of one right-hand side under one preconditioner: the fp64 model and the fp32 deviation; computed once, shared."""
    M, r = model(name), rhs(name)[label]
    z = M.apply(r, preconditioner=precond)
    d32 = vc.fp32_deviation(M.apply(r, np.float32, precond), z)
    z.setflags(write=False)
    return z, d32


def bar(name, label, precond, f64):
    z, d32 = reference(name, label, precond)
    return vc.F64_REL * float(np.abs(z).max()) if f64 else vc.F32_BARS * d32


def iterate(name, precond, k, b, f64):
    """(p_k, bar) of the model PCG on the right-hand side b after exactly k iterations."""
    M = model(name)
    p, it = M.pcg(b, max_iterations=k, preconditioner=precond)
    assert it == k, (name, precond, k, it)
    if f64:
        return p, vc.F64_REL * float(np.abs(p).max())
    p32, _ = M.pcg(b, max_iterations=k, preconditioner=precond, dtype=np.float32, stop=False)
    return p, vc.F32_BARS * vc.fp32_deviation(p32, p)


@functools.lru_cache(maxsize=None)
def model_pcg(name, precond):
    """(p, iterations) of the model PCG on the field's own b, computed once."""
    return model(name).pcg(system(name)["b"], preconditioner=precond)


@functools.lru_cache(maxsize=None)
def oracle_exact(name):
    """(factor, M^-1 probe) of the oracle's exact MIC(0) on the field's fp32-rounded grid."""
    s = sc.cpu_sim(name) if name in sc.CASES else None
    size, parts, solid, meta = build(name)
    if s is None:
        s = orc.CpuSim(size, cell_size=meta["h"], offset=meta["off"], method=sc.APIC, blending=1.0, density=meta["rho"])
        if solid is not None:
            s.set_solid_cells(solid)
        s.set_particles(parts)
    w = system(name)
    s.hash()
    s.p2g()
    cells = s.cells()
    cells["vel"], cells["type"] = w["vel"], w["type"]
    s.set_cells(cells)
    s.build_system(DT)
    assert np.array_equal(s.abits(), w["abits"]) and np.array_equal(s.fluid_cells(), w["fluid_cells"])
    out = s.precon(), s.apply_precon(sc.probe(len(w["abits"])))
    s.close()
    return out


# ---------------------------------------------------------------------------------------------------- what a field can show
def features(name):
    M = model(name)
    C = M.coarse
    f = {"unknowns": M.n, "level1": C.n1, "level2": C.n2, "blocks_in_grid": int(np.prod(C.block_dims)), "regularised": C.regularised}
    f["l1_l2_identity"] = bool(np.array_equal(C.blocks, np.arange(C.n2)))
    f["tile_safety"] = M.tile_factor(info=True)[1:]
    f["level1_safety"] = M.level1_factor(info=True)[1:]
    f["couplings_across_tile_faces"] = int(sum(w.sum() for w in C.w))
    full = max(int(w.max()) for w in C.w)
    f["full_face"] = full
    f["partial_faces"] = int(sum(((w > 0) & (w < full)).sum() for w in C.w))
    # level-1 unknowns on a face of their block whose neighbour across that face, inside the grid of tiles, holds no unknown
    n = 0
    for d in range(3):
        c = C.coords[d]
        n += int(((c % 8 == 7) & (c < C.dims[d] - 1) & (C.whole.up[d] == C.n1)).sum())
        n += int(((c % 8 == 0) & (c > 0) & (C.whole.lo[d] == C.n1)).sum())
    f["missing_across_block_face"] = n
    return f
