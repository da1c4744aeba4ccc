"""The tile-local MIC(0) preconditioner (LFA_PRECOND_MIC0_TILED) and the multilevel one (LFA_PRECOND_MULTILEVEL: the tile-local
MIC(0) plus a level-1 / level-2 coarse correction) of libfluid_amd/csrc/pcg.hip restated in plain numpy, fp64.

A stateless function of the level-0 system - size, the unknown list (raw cell index, ascending), the A bytes (bits 0-2 the number of
non-solid neighbours ns, bits 3-5 "the +x / +y / +z neighbour is typed FLUID": the coupling b_d), a_scale - and of tau and sigma.
Vectors run over the unknowns in the reference's order; no tile-major storage, no launch layout: k_mic_apply + k_coarse_all +
k_add_coarse, k_mic_apply with the embedded coarse workgroups, the fused k_pcg_a / k_pcg_b with fast_tile_sweeps and the restricted
residual carried by linearity, and k_coarse_apply + k_coarse_top above 64 level-1 blocks are ONE operator and this is it. Written from
the reference's src/pressure_solver.cpp and the device code of pcg.hip; the rules and the kernels or functions they restate:

  tile factor   e_i = ns_i - scale sum_d [(b_d(j) pre_j)^2 + tau b_d(j) (b_d+1(j) + b_d+2(j)) pre_j^2] over the -d neighbours j that
                are unknowns; e_i < sigma ns_i: e_i = ns_i; pre_i = 1 / sqrt(e_i scale)
                                                    pressure_solver::_compute_preconditioner, k_mic_factor
                exact=False: a -d neighbour in another tile does not exist (k_mic_factor<real, false> reads no face neighbour).
                The tau term of a neighbour j INSIDE the tile is taken from j's raw A byte (`aj` in k_mic_factor): b_d+1(j) and
                b_d+2(j) count even where those couplings of j cross a tile face. The tiled factor is therefore not the MIC(0) of
                the tile's diagonal block - it is the exact recurrence with the terms of missing neighbours dropped. The model
                pins that; it does not judge it.
  tile apply    q_i = (r_i + scale sum_d b_d(j) pre_j q_j) pre_i upwards, z_i = (q_i + scale pre_i sum_d b_d(i) z_i+d) pre_i downwards
                (pressure_solver::_apply_preconditioner; k_mic_apply; the closed form of the fused kernel: the comment above
                fast_tile_sweeps), inside the tile when not exact
  level 1       one unknown per particle tile that holds an unknown; diag_I = sum_i (ns_i - 2 #couplings of i towards +d that stay
                inside I), w_d(I) = #couplings across the +d face of I (k_coarse_coeffs); A1 = scale (diag, -w)
  level-1 MIC   per 8^3 block of tiles the weighted MIC(0) of A1, block-local: a -d neighbour in another block does not exist,
                the tau term reads the neighbour's raw weights (k_coarse_factor); sweeps: coarse_block / k_coarse_apply
  level 2       one unknown per level-1 block that holds an unknown, in the order of the blocks' positions in the grid of
                blocks; A2 = P1^T A1 P1 (coarse_setup), solved densely; where A2 is not positive definite (spd_inverse fails) the
                diagonal gets 1e-8 trace / n + 1e-30 (coarse_setup): Coarse.regularised says so
  operator      z = M_tile^-1 r + P (M1^-1 P^T r) + P P1 (A2^-1 P1^T P^T r), P and P1 piecewise constant, weights 1 (CoarseFields,
                k_update_s, k_add_coarse)
  PCG           the loop of vcycle_model.pcg: signed maximum of the residual below the tolerance, tested behind the AXPYs, the
                count includes the iteration that stops (verdict_stops in pcg.h); b.b < 1e-6: p = 0 and no iteration

dtype=np.float32: vectors, factors and sweeps are fp32 (no fused multiply-add), the reductions (restriction sums, dot products) are
fp64, the inverse of A2 is rounded to fp32 and applied with fp64 sums - as on the device. It measures what fp32 arithmetic does to
the operator and is used for the fp32 bars only.

mutant= changes exactly one rule (MUTANTS); tests/test_multilevel_model.py shows that each moves z by at least 100 fp32 bars.
"""
import numpy as np

TAU, SIGMA = 0.97, 0.25  # lfa_default_params (libfluid_amd/csrc/core.hip), pressure_solver.h
TILED, MULTILEVEL, EXACT = "mic0_tiled", "multilevel", "mic0_exact"

MUTANTS = {
    "no_level1": "the level-1 term P M1^-1 P^T r is missing. Needs: a level-1 unknown.",
    "no_level2": "the level-2 term is missing. Needs: a level-2 unknown.",
    "diag_keeps_inner": "diag_I = sum ns_i, without - 2 #inner couplings. Needs: two coupled unknowns in one tile.",
    "weights_on_minus_face": "w_d(I) counts the couplings across the -d face of I. Needs: tiles whose two d faces carry different counts.",
    "l1_l2_identity": "the level-2 value of a level-1 block is looked up at the block's position in the grid of blocks instead of in "
                      "the list of blocks that hold unknowns. Needs: a block without unknowns in front of one with unknowns.",
    "tile_reads_across_faces": "the tiled factor and sweeps read their neighbours across tile faces (they behave as exact). Needs: a "
                               "coupling across a tile face.",
    "no_tau": "tau = 0 in the factors. Needs: an unknown j with b_d(j) and another coupling.",
    "no_safety": "the branch e < sigma a_ii is never taken. Needs: an unknown on which it fires.",
    "coarse_unscaled": "the level-1 MIC(0) factors and sweeps A1 without a_scale. Needs: a_scale != 1.",
    "restrict_all_cells": "the restriction sums all 512 cells of a tile, and the cells that are no unknowns hold 1 instead of 0 (the "
                          "device keeps them at exactly 0: only the mutant's right-hand side is non-zero there). Needs: a tile that "
                          "is not full.",
}


class Sweep:
    """The substitution order of one level: n unknowns, lo[d] / up[d] the index of the -d / +d neighbour (n: none; arrays carry one
    dummy entry at n that stays 0), groups: the unknowns of every hyperplane, ascending."""

    def __init__(self, coords, dims, local, grid=None):
        x = [np.asarray(c, dtype=np.int64) for c in coords]
        n = len(x[0])
        self.n = n
        if grid is None:
            grid = np.full(tuple(int(k) for k in dims[::-1]), n, dtype=np.int64)
            grid[x[2], x[1], x[0]] = np.arange(n)
        self.grid = grid
        self.lo, self.up = [], []
        for d in range(3):
            c = [x[0].copy(), x[1].copy(), x[2].copy()]
            ok = (x[d] % 8 > 0) if local else (x[d] > 0)
            c[d] = np.maximum(x[d] - 1, 0)
            self.lo.append(np.where(ok, grid[c[2], c[1], c[0]], n))
            ok = (x[d] % 8 < 7) if local else np.ones(n, dtype=bool)
            ok = ok & (x[d] < dims[d] - 1)
            c[d] = np.minimum(x[d] + 1, dims[d] - 1)
            self.up.append(np.where(ok, grid[c[2], c[1], c[0]], n))
        level = sum(c % 8 for c in x) if local else sum(x)
        order = np.argsort(level, kind="stable")
        cuts = np.flatnonzero(np.diff(level[order])) + 1
        self.groups = np.split(order, cuts) if n else []


def _factor(S, diag, w, scale, tau, sigma, dt, level1, safety=True):
    """pre (n + 1, the dummy 0), the number of unknowns on which the safety branch fired and the smallest e / a_ii before it.
    level1=False: k_mic_factor's expressions (unit couplings, scale applied at the end); True: k_coarse_factor's."""
    n = S.n
    pre = np.zeros(n + 1, dtype=dt)
    wx = [np.append(np.asarray(k, dtype=dt), dt(0)) for k in w]
    diag = np.asarray(diag, dtype=dt)
    scale, tau, sigma = dt(scale), dt(tau), dt(sigma)
    fired, smallest = 0, np.inf
    for g in S.groups:
        neg, negt = np.zeros(len(g), dtype=dt), np.zeros(len(g), dtype=dt)
        for d in range(3):
            j = S.lo[d][g]
            pj, bd, bo1, bo2 = pre[j], wx[d][j], wx[(d + 1) % 3][j], wx[(d + 2) % 3][j]
            if level1:
                ad = scale * bd
                neg = neg + ((ad * pj) * (ad * pj) + tau * ad * (scale * bo1 + scale * bo2) * pj * pj)
            else:
                ap = bd * pj
                neg = neg + ap * ap
                negt = negt + (bd * (bo1 + bo2)) * pj * pj
        if level1:
            aii = scale * diag[g]
            e = aii - neg
        else:
            aii = diag[g]
            e = aii - (neg + tau * negt) * scale
        if len(g):
            smallest = min(smallest, float((e / aii).min()))
        hit = e < sigma * aii
        if safety:
            fired += int(hit.sum())
            e = np.where(hit, aii, e)
        pre[g] = dt(1) / np.sqrt(e if level1 else e * scale)
    return pre, fired, smallest


def _substitute(S, pre, w, scale, r, dt):
    """z = (L L^T)^-1 r over the unknowns of S: both sweeps."""
    n = S.n
    scale = dt(scale)
    wx = [np.append(np.asarray(k, dtype=dt), dt(0)) for k in w]
    q, pq, z = np.zeros(n + 1, dtype=dt), np.zeros(n + 1, dtype=dt), np.zeros(n + 1, dtype=dt)
    for g in S.groups:
        t = np.zeros(len(g), dtype=dt)
        for d in range(3):
            j = S.lo[d][g]
            t = t + wx[d][j] * pq[j]
        q[g] = (r[g] + scale * t) * pre[g]
        pq[g] = pre[g] * q[g]
    for g in S.groups[::-1]:
        t = np.zeros(len(g), dtype=dt)
        for d in range(3):
            t = t + wx[d][g] * z[S.up[d][g]]
        z[g] = (q[g] + scale * pre[g] * t) * pre[g]
    return z[:n]


class Coarse:
    """Levels 1 and 2: n1, n2; tile (the level-1 unknown of every level-0 unknown); coords (tx, ty, tz) of the level-1 unknowns;
    diag, w[3] (integers); block (the level-2 unknown of every level-1 unknown) and grid_pos (that block's position in the grid of
    blocks); A2 (dense, scaled), regularised; pre1 / fired1 / smallest1 of the level-1 factor per element type."""


class Model:
    """model = Model(size, fluid_cells, abits, a_scale); model.apply(r), model.pcg(b), ..."""

    def __init__(self, size, fluid_cells, abits, a_scale, tau=TAU, sigma=SIGMA, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.size = tuple(int(k) for k in size)
        nx, ny, nz = self.size
        self.mutant, self.a_scale, self.tau, self.sigma = mutant, float(a_scale), (0.0 if mutant == "no_tau" else float(tau)), float(sigma)
        fc = np.asarray(fluid_cells, dtype=np.int64)
        ab = np.asarray(abits).astype(np.int64)
        assert len(fc) == len(ab) and (np.diff(fc) > 0).all()
        self.n = len(fc)
        self.coords = (fc % nx, (fc // nx) % ny, fc // (nx * ny))
        self.ns = ab & 7
        self.b = [(ab >> (3 + d)) & 1 for d in range(3)]
        self.whole = Sweep(self.coords, self.size, False)
        self.tiled = self.whole if mutant == "tile_reads_across_faces" else Sweep(self.coords, self.size, True, self.whole.grid)
        # the couplings of A itself: towards +d where the bit is set and the neighbour is an unknown, towards -d the neighbour's bit
        self._up = [np.where(self.whole.up[d] < self.n, self.b[d], 0) for d in range(3)]
        self._lo = [np.append(self._up[d], 0)[self.whole.lo[d]] for d in range(3)]
        self._cache = {}
        self.coarse = self._coarse()

    # ------------------------------------------------------------------------------------------------ level 0
    def apply_a(self, v):
        """A v, scaled (pressure_solver::_apply_a), fp64. tests/test_multilevel_model.py holds it to vcycle_model.apply_a."""
        vx = np.append(np.asarray(v, dtype=np.float64), 0.0)
        val = self.ns * vx[:-1]
        for d in range(3):
            val = val - self._lo[d] * vx[self.whole.lo[d]] - self._up[d] * vx[self.whole.up[d]]
        return self.a_scale * val

    def _sweep(self, exact):
        return self.whole if exact else self.tiled

    def tile_factor(self, exact=False, dtype=np.float64, info=False):
        """pre over the unknowns. info=True: (pre, unknowns on which e < sigma ns fired, smallest e / ns seen)."""
        dt = np.float32 if dtype == np.float32 else np.float64
        key = ("factor", bool(exact), dt)
        if key not in self._cache:
            self._cache[key] = _factor(self._sweep(exact), self.ns, self.b, self.a_scale, self.tau, self.sigma, dt, False,
                                       safety=self.mutant != "no_safety")
        pre, fired, smallest = self._cache[key]
        return (pre[:-1].astype(np.float64), fired, smallest) if info else pre[:-1].astype(np.float64)

    def tile_apply(self, r, exact=False, dtype=np.float64):
        dt = np.float32 if dtype == np.float32 else np.float64
        self.tile_factor(exact, dt)
        pre = self._cache[("factor", bool(exact), dt)][0]
        r = np.asarray(r, dtype=np.float64).astype(dt)
        return _substitute(self._sweep(exact), pre, self.b, self.a_scale, r, dt).astype(np.float64)

    # ------------------------------------------------------------------------------------------------ levels 1 and 2
    def _coarse(self):
        C = Coarse()
        m = self.mutant
        nx, ny, nz = self.size
        nt = ((nx + 7) // 8, (ny + 7) // 8, (nz + 7) // 8)
        x, y, z = self.coords
        tid = (x // 8) + nt[0] * ((y // 8) + nt[1] * (z // 8))
        tiles, C.tile = np.unique(tid, return_inverse=True)
        C.n1 = len(tiles)
        C.coords = (tiles % nt[0], (tiles // nt[0]) % nt[1], tiles // (nt[0] * nt[1]))
        C.dims = nt
        loc = [c % 8 for c in self.coords]
        inner = sum(np.where(loc[d] < 7, self.b[d], 0) for d in range(3))
        per_cell = self.ns if m == "diag_keeps_inner" else self.ns - 2 * inner
        C.diag = np.bincount(C.tile, weights=per_cell, minlength=C.n1).astype(np.int64)
        C.w = []
        for d in range(3):
            if m == "weights_on_minus_face":
                across = np.where(loc[d] == 0, self._lo[d], 0)
            else:
                across = np.where(loc[d] == 7, self.b[d], 0)
            C.w.append(np.bincount(C.tile, weights=across, minlength=C.n1).astype(np.int64))
        C.full = np.bincount(C.tile, minlength=C.n1)  # unknowns per tile
        C.whole = Sweep(C.coords, nt, False)
        C.local = Sweep(C.coords, nt, True, C.whole.grid)
        nb = tuple((k + 7) // 8 for k in nt)
        C.block_dims = nb
        bid = (C.coords[0] // 8) + nb[0] * ((C.coords[1] // 8) + nb[1] * (C.coords[2] // 8))
        C.blocks, C.block = np.unique(bid, return_inverse=True)  # (ascending position in the grid of blocks: coarse_setup's list)
        C.n2 = len(C.blocks)
        C.grid_pos = C.blocks[C.block]
        # A2 = P1^T A1 P1 (coarse_setup): a weight towards a tile without unknowns, or outside the grid, couples to nothing
        s = self.a_scale
        A2 = np.zeros((C.n2, C.n2))
        np.add.at(A2, (C.block, C.block), s * C.diag)
        for d in range(3):
            j = C.whole.up[d]
            on = (j < C.n1) & (C.w[d] != 0)
            k, k2 = C.block[on], C.block[j[on]]
            np.add.at(A2, (k, k2), -s * C.w[d][on])
            np.add.at(A2, (k2, k), -s * C.w[d][on])
        C.A2, C.regularised = A2, False
        try:
            np.linalg.cholesky(A2)
        except np.linalg.LinAlgError:
            C.regularised = True
            C.A2 = A2 + np.eye(C.n2) * (1e-8 * np.trace(A2) / C.n2 + 1e-30)
        return C

    def a1_dense(self):
        """A1 = scale (diag, -w) over the level-1 unknowns, dense (for the Galerkin identity)."""
        C = self.coarse
        A = np.diag(self.a_scale * C.diag.astype(np.float64))
        for d in range(3):
            j = C.whole.up[d]
            on = j < C.n1
            A[np.flatnonzero(on), j[on]] -= self.a_scale * C.w[d][on]
            A[j[on], np.flatnonzero(on)] -= self.a_scale * C.w[d][on]
        return A

    def p1_dense(self):
        C = self.coarse
        P = np.zeros((C.n1, C.n2))
        P[np.arange(C.n1), C.block] = 1.0
        return P

    def level1_factor(self, dtype=np.float64, info=False):
        dt = np.float32 if dtype == np.float32 else np.float64
        key = ("factor1", dt)
        C = self.coarse
        if key not in self._cache:
            s1 = 1.0 if self.mutant == "coarse_unscaled" else self.a_scale
            self._cache[key] = _factor(C.local, C.diag, C.w, s1, self.tau, self.sigma, dt, True, safety=self.mutant != "no_safety")
        pre, fired, smallest = self._cache[key]
        return (pre[:-1].astype(np.float64), fired, smallest) if info else pre[:-1].astype(np.float64)

    def coarse_apply(self, r, dtype=np.float64):
        """(x1, x2): M1^-1 P^T r over the level-1 unknowns and A2^-1 P1^T P^T r over the level-2 unknowns."""
        dt = np.float32 if dtype == np.float32 else np.float64
        C, m = self.coarse, self.mutant
        r = np.asarray(r, dtype=np.float64).astype(dt)
        r1 = np.bincount(C.tile, weights=r.astype(np.float64), minlength=C.n1)
        if m == "restrict_all_cells":
            r1 = r1 + (512 - C.full)
        r1 = r1.astype(dt)
        self.level1_factor(dt)
        s1 = 1.0 if m == "coarse_unscaled" else self.a_scale
        x1 = _substitute(C.local, self._cache[("factor1", dt)][0], C.w, s1, r1, dt)
        r2 = np.bincount(C.block, weights=r1.astype(np.float64), minlength=C.n2)
        if dt == np.float32:
            key = "a2inv32"
            if key not in self._cache:
                self._cache[key] = np.linalg.inv(C.A2).astype(np.float32).astype(np.float64)
            x2 = (self._cache[key] @ r2).astype(dt)
        else:
            x2 = np.linalg.solve(C.A2, r2)
        return x1, x2

    # ------------------------------------------------------------------------------------------------ the operator
    def apply(self, r, dtype=np.float64, preconditioner=MULTILEVEL):
        """z = M^-1 r over the unknowns (fp64 array whatever the arithmetic)."""
        dt = np.float32 if dtype == np.float32 else np.float64
        z = self.tile_apply(r, preconditioner == EXACT, dt).astype(dt)
        if preconditioner == MULTILEVEL:
            C, m = self.coarse, self.mutant
            x1, x2 = self.coarse_apply(r, dt)
            if m == "no_level1":
                x1 = np.zeros_like(x1)
            if m == "no_level2":
                x2 = np.zeros_like(x2)
            if m == "l1_l2_identity":
                at_pos = np.zeros(max(int(C.blocks.max()) + 1, C.n2), dtype=dt)
                at_pos[: C.n2] = x2
                top = at_pos[C.grid_pos]
            else:
                top = x2[C.block]
            xc = (x1 + top).astype(dt)  # k_update_s / k_add_coarse: coarse_x[i1] + coarse_x2[l1_l2[i1 >> 9]]
            z = (z + xc[C.tile]).astype(dt)
        return z.astype(np.float64)

    def _dot(self, a, b, by_tile):
        prod = a.astype(np.float64) * b.astype(np.float64)
        if by_tile:
            return float(np.bincount(self.coarse.tile, weights=prod, minlength=self.coarse.n1).sum())
        return float(prod.sum())

    def pcg(self, b, max_iterations=200, preconditioner=MULTILEVEL, tolerance=1e-6, dtype=np.float64, stop=True, dots_by_tile=False):
        """(p, iterations). stop=False: exactly max_iterations iterations, whatever the residual. dots_by_tile: the dot products
        are summed tile by tile and then over the tiles (another order of the same sum)."""
        dt = np.float32 if dtype == np.float32 else np.float64
        b64 = np.asarray(b, dtype=np.float64)
        p = np.zeros(self.n, dtype=dt)
        if float(b64 @ b64) < 1e-6:  # src/pressure_solver.cpp:33-35
            return p.astype(np.float64), 0
        r = b64.astype(dt)
        z = self.apply(r, dt, preconditioner).astype(dt)
        s = z.copy()
        sigma = self._dot(z, r, dots_by_tile)
        it = 0
        while it < max_iterations:
            q = self.apply_a(s).astype(dt) if dt == np.float64 else self._apply_a32(s)
            alpha = dt(sigma / self._dot(q, s, dots_by_tile))
            p = (p + alpha * s).astype(dt)
            r = (r + (-alpha) * q).astype(dt)
            it += 1
            if stop and r.max() < tolerance:
                break
            z = self.apply(r, dt, preconditioner).astype(dt)
            sigma_new = self._dot(z, r, dots_by_tile)
            s = (z + dt(sigma_new / sigma) * s).astype(dt)
            sigma = sigma_new
        return p.astype(np.float64), it

    def _apply_a32(self, v):
        """k_spmv's expression in fp32: ns v, minus the three lower and the three upper neighbours, times scale."""
        f = np.float32
        vx = np.append(v.astype(f), f(0))
        val = self.ns.astype(f) * vx[:-1]
        for d in range(3):
            val = val - self._lo[d].astype(f) * vx[self.whole.lo[d]]
        for d in range(3):
            val = val - self._up[d].astype(f) * vx[self.whole.up[d]]
        return (f(self.a_scale) * val).astype(f)
