"""Inputs and the CPU model for the tracers (libfluid_amd/csrc/tracers.hip). No GPU here.

A tracer step is the reference's _advect_particles, _detect_collisions and PIC grid-to-particle transfer applied to points that
are no particles. Every expected value is the oracle's:
  move set      : every case of tests/move_cases.py with the tracers as the case's `pos` and `vel`; expected mc.oracle(name)
                  (n = 1, 64, 511, 513; the six tile-reach directions; obstacles; non-dyadic h and offsets in `walls`).
  transfer set  : sc.random_field() with the points of tests/sample_cases.py, the outside block included - without its three
                  non-finite rows, which cannot become tracers (lfa_tracers_add rejects them; tests/test_gpu_tracers.py checks
                  that). Expected: sc.model.
  stepped scene : sc.SIZE, sc.H, sc.OFFSET (no binary fractions), the sparse particles of sample_cases, a solid block beside the
                  first blob, and N_TRACERS tracers started from particle positions with velocities pointing at the block.
advect_collide() runs the oracle (or the compiled reference) on any tracer state. It does not say WHICH tracers a march stopped;
march_model() does: the same arithmetic in Python floats, written to count, and pinned to the oracle bit for bit by
tests/test_tracer_cases.py."""
import functools
import math

import numpy as np

from libfluid_amd.scenes import PARTICLE_DTYPE
from oracle import loader as orc
from tests import move_cases as mc
from tests import sample_cases as sc

SKIN = 0.1            # boundary_skin_width (include/fluid/simulation.h), world units
N_TRACERS = 513       # two blocks and a wave's tail
SEED = 20261020
BLOCK_LO, BLOCK_HI = (8, 0, 0), (10, 9, 9)   # the stepped scene's solid block, cells [lo, hi): beside the blob in [2, 6)^3
MOVE_NAMES = mc.NAMES


# ---------------------------------------------------------------------------------------------------- the oracle on a tracer state
def advect_collide(size, h, off, solid, pos, vel, dt, kind="oracle"):
    """{"advect", "collide"}: positions after _advect_particles and after _detect_collisions, in input order (mc.run_cpu)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    parts = np.zeros(len(pos), dtype=PARTICLE_DTYPE)
    parts["pos"] = pos
    parts["old_pos"] = pos
    parts["vel"] = vel
    parts["cx"][:, 0] = np.arange(len(pos))
    meta = dict(h=float(h), off=tuple(float(o) for o in off), dt=float(dt))
    return mc.run_cpu((tuple(size), parts, solid, meta), kind=kind)


# ---------------------------------------------------------------------------------------------------- the counting restatement
def march_model(size, mask, h, off, pos, vel, dt):
    """(end float64[n, 3], stopped bool[n]): src/simulation.cpp:240-248 and :612-683 with grid.h:140-209 in world units, one Python
    float operation per reference operation, in its order. stopped: a march met a solid cell or a wall."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    n = [int(s) for s in size]
    off = [float(o) for o in off]
    h, dt, skin = float(h), float(dt), SKIN
    lo = [off[d] + skin for d in range(3)]
    hi = [h * float(n[d]) + off[d] - skin for d in range(3)]

    def blocked(c):
        return any(c[d] < 0 or c[d] >= n[d] for d in range(3)) or bool(mask[c[0], c[1], c[2]])

    inf = math.inf
    ends, stopped = np.empty_like(pos), np.zeros(len(pos), dtype=bool)
    for i in range(len(pos)):
        frm = [float(x) for x in pos[i]]
        to = [frm[d] + float(vel[i, d]) * dt for d in range(3)]
        to = [lo[d] if to[d] < lo[d] else (hi[d] if hi[d] < to[d] else to[d]) for d in range(3)]
        for _ in range(3):
            a = [(frm[d] - off[d]) / h for d in range(3)]
            b = [(to[d] - off[d]) / h for d in range(3)]
            cur, last = [math.floor(x) for x in a], [math.floor(x) for x in b]
            diff = [b[d] - a[d] for d in range(3)]
            adv = [1 if diff[d] > 0.0 else -1 for d in range(3)]
            inv = [1.0 / abs(diff[d]) if diff[d] != 0.0 else inf for d in range(3)]
            t = []
            for d in range(3):
                gap = abs(float(cur[d] + (1 if diff[d] > 0.0 else 0)) - a[d])
                t.append(math.nan if (gap == 0.0 and inv[d] == inf) else gap * inv[d])
            hit = False
            while cur != last:
                dim, tmin = 0, 2.0
                for d in range(3):
                    if t[d] < tmin:
                        tmin, dim = t[d], d
                if not tmin <= 1.0:
                    break
                cur[dim] += adv[dim]
                if blocked(cur):
                    tt = t[dim] + skin / ((to[dim] - frm[dim]) * float(-adv[dim]))
                    if tt < 0.0:
                        tt = 0.0
                    frm = [tt * to[d] + (1.0 - tt) * frm[d] for d in range(3)]
                    to[dim] = frm[dim]
                    hit = True
                    break
                t[dim] += inv[dim]
            if not hit:
                break
            stopped[i] = True
        gp = [to[d] - off[d] for d in range(3)]
        ci = [int(gp[d] / h) for d in range(3)]
        cp = [gp[d] - float(ci[d]) * h for d in range(3)]
        skin_max = h - skin
        for d in range(3):
            if cp[d] < skin:
                q = list(ci)
                q[d] -= 1
                if ci[d] == 0 or blocked(q):
                    to[d] += skin - cp[d]
            if cp[d] > skin_max:
                q = list(ci)
                q[d] += 1
                if ci[d] + 1 >= n[d] or blocked(q):
                    to[d] += skin_max - cp[d]
        ends[i] = to
    return ends, stopped


# ---------------------------------------------------------------------------------------------------- the sets
def move_case(name):
    """(size, h, off, dt, solid, pos, vel) of a move case."""
    size, parts, solid, meta = mc.build(name)
    return size, meta["h"], meta["off"], meta["dt"], solid, parts["pos"].copy(), parts["vel"].copy()


@functools.lru_cache(maxsize=None)
def transfer_points():
    pts = sc.points()
    pts = np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1)])
    pts.setflags(write=False)
    return pts


def block_cells():
    return np.array([(x, y, z) for z in range(BLOCK_LO[2], BLOCK_HI[2]) for y in range(BLOCK_LO[1], BLOCK_HI[1])
                     for x in range(BLOCK_LO[0], BLOCK_HI[0])], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def stepped_tracers():
    """(pos, vel) float64[N_TRACERS, 3]: the first N_TRACERS particles of the first blob (cells [2, 6)^3); each aims at a point of the
    block's near face x = 8 at its own height, with a move of 0 to 7 cells in the first step: some reach the face, some do not."""
    rng = np.random.default_rng(SEED)
    pos = sc.sparse_particles()["pos"][:N_TRACERS].copy()
    off = np.array(sc.OFFSET)
    target = off + np.stack([np.full(N_TRACERS, 8.5), 1.0 + 6.0 * rng.random(N_TRACERS), 1.0 + 6.0 * rng.random(N_TRACERS)], axis=1) * sc.H
    aim = target - pos
    aim /= np.linalg.norm(aim, axis=1)[:, None]
    vel = aim * (rng.random(N_TRACERS) * 7.0 * sc.H / sc.DT)[:, None]
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def solid_mask():
    return mc.solid_mask(sc.SIZE, block_cells())


@functools.lru_cache(maxsize=None)
def stepped_cpu_model(steps=3):
    """The stepped scene on the CPU alone: the oracle's PIC time_step for the fluid, march_model and sc.model for the tracers.
    Returns (stopped in any step bool[n], stopped per step [steps], final positions)."""
    fluid = orc.CpuSim(sc.SIZE, cell_size=sc.H, offset=sc.OFFSET, gravity=sc.GRAVITY, method=orc.PIC)
    fluid.set_solid_cells(block_cells())
    fluid.set_particles(sc.sparse_particles())
    pos, vel = (a.copy() for a in stepped_tracers())
    mask = solid_mask()
    ever, per_step = np.zeros(N_TRACERS, dtype=bool), []
    for _ in range(steps):
        fluid.L.time_step(fluid.h, sc.DT, None, None)
        pos, stopped = march_model(sc.SIZE, mask, sc.H, sc.OFFSET, pos, vel, sc.DT)
        vel = sc.model(fluid.cells(), pos)[0]
        ever |= stopped
        per_step.append(int(stopped.sum()))
    fluid.close()
    return ever, per_step, pos
