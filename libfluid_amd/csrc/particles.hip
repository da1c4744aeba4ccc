// libfluid_amd/csrc/particles.hip -- the per-step particle stages either side of the hot path:
// advection, collision against solid cells / domain walls, position correction, and the device-resident
// simulation::time_step built from them.
//
// Reference: simulation::_advect_particles src/simulation.cpp:226-249; _detect_collisions :612-683 with
// grid::march_cells include/fluid/data_structures/grid.h:140-209; _correct_positions :562-610; time_step :43-125.
// Positions live on the device as (cell, fraction-in-cell); the marches run in fp64 grid units (cell + fraction), which is
// the reference's (position - grid_offset) / cell_size.
#include <math.h>

#include <algorithm>
#include <utility>

#include "common.h"
#include "pcg.h"

namespace {

__device__ inline bool solid_or_outside(const GridDims &g, const uint8_t *solid, int x, int y, int z) {
	if (!in_grid(g, x, y, z)) return true;
	return solid[blocked_index(g, x, y, z)] != 0;
}

/// _detect_collisions for one particle, in grid units (skin = boundary_skin_width / cell_size): up to three bounces of
/// the segment from -> to (DDA over cells, first solid/outside cell stops it `skin` short of the face and removes the
/// normal component), then the push-out from walls / solid neighbours closer than `skin`. Result in `to`.
__device__ inline void collide(const GridDims &g, const uint8_t *solid, double from[3], double to[3], double skin) {
	for (int bounce = 0; bounce < 3; ++bounce) {
		bool hit = false;
		double diff[3], inv[3], t[3];
		int cur[3], last[3], adv[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			cur[d] = (int)floor(from[d]);
			last[d] = (int)floor(to[d]);
			diff[d] = to[d] - from[d];
			adv[d] = diff[d] > 0.0 ? 1 : -1;
			inv[d] = 1.0 / fabs(diff[d]);
			t[d] = fabs((double)(cur[d] + (diff[d] > 0.0 ? 1 : 0)) - from[d]) * inv[d];
		}
		for (int guard = 0; guard < 4096 && (cur[0] != last[0] || cur[1] != last[1] || cur[2] != last[2]); ++guard) {
			int dim = 0;
			double tmin = 2.0;
			if (t[0] < tmin) { tmin = t[0]; dim = 0; }
			if (t[1] < tmin) { tmin = t[1]; dim = 1; }
			if (t[2] < tmin) { tmin = t[2]; dim = 2; }
			if (!(tmin <= 1.0)) break;  // grid.h:196-199
			// static indexing (no scratch): update the chosen axis
			const int a0 = dim == 0, a1 = dim == 1, a2 = dim == 2;
			cur[0] += a0 ? adv[0] : 0; cur[1] += a1 ? adv[1] : 0; cur[2] += a2 ? adv[2] : 0;
			if (solid_or_outside(g, solid, cur[0], cur[1], cur[2])) {
				const double td = a0 ? t[0] : (a1 ? t[1] : t[2]);
				const double od = a0 ? diff[0] : (a1 ? diff[1] : diff[2]);
				const int ad = a0 ? adv[0] : (a1 ? adv[1] : adv[2]);
				double tt = td + skin / (od * (double)(-ad));
				if (tt < 0.0) tt = 0.0;
#pragma unroll
				for (int d = 0; d < 3; ++d) from[d] = tt * to[d] + (1.0 - tt) * from[d];
				if (a0) to[0] = from[0];
				if (a1) to[1] = from[1];
				if (a2) to[2] = from[2];
				hit = true;
				break;
			}
			t[0] += a0 ? inv[0] : 0.0; t[1] += a1 ? inv[1] : 0.0; t[2] += a2 ? inv[2] : 0.0;
		}
		if (!hit) break;
	}
	int ci[3];
	double cp[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		ci[d] = (int)to[d];
		cp[d] = to[d] - (double)ci[d];
	}
	const double skin_max = 1.0 - skin;
	const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		if (cp[d] < skin) {
			if (ci[d] == 0 || solid_or_outside(g, solid, ci[0] - (d == 0), ci[1] - (d == 1), ci[2] - (d == 2))) to[d] += skin - cp[d];
		}
		if (cp[d] > skin_max) {
			if (ci[d] + 1 >= n[d] || solid_or_outside(g, solid, ci[0] + (d == 0), ci[1] + (d == 1), ci[2] + (d == 2)))
				to[d] += skin_max - cp[d];
		}
	}
}

/// What is left of `collide` when no solid cell is within reach: nothing stops the segment, and the skin push-out (:654-681)
/// only ever fires at the domain walls.
__device__ inline void collide_walls_only(const GridDims &g, double to[3], double skin) {
	const int n[3] = {g.nx, g.ny, g.nz};
	const double skin_max = 1.0 - skin;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		const int ci = (int)to[d];
		const double cp = to[d] - (double)ci;
		double x = to[d];
		if (cp < skin && ci == 0) x += skin - cp;
		if (cp > skin_max && ci + 1 >= n[d]) x += skin_max - cp;
		to[d] = x;
	}
}

__device__ inline void cell_of_key(const GridDims &g, uint32_t key, int c[3]) {
	int tile = (int)(key >> 9), l = (int)(key & 511), tx, ty, tz;
	tile_coords(g, tile, tx, ty, tz);
	c[0] = tx * 8 + (l & 7); c[1] = ty * 8 + ((l >> 3) & 7); c[2] = tz * 8 + (l >> 6);
}
/// grid-unit position -> (clamped cell, fraction), the same rule as the upload path (core.hip: cell_and_fraction).
__device__ inline void split_position(double p, int n, int &cell, float &t) {
	double m = p < 0.0 ? 0.0 : p;
	int c = m >= (double)n ? n - 1 : (int)m;
	double td = p - (double)c;
	float tf = (float)td;
	if (!(tf > 0.0f)) tf = 0.0f;
	if (td < 1.0 && tf >= 1.0f) tf = 0.99999994f;
	if (tf > 1.0f) tf = 1.0f;
	cell = c;
	t = tf;
}

#ifndef CORR_PARTS
#define CORR_PARTS 2                       // workgroups per tile of the LDS-tiled position correction (split in z; 4: 5.6 instead of 5.0 ms alone, and no better beside the pressure solve)
#endif
#define CORR_THREADS 512                   // 8 waves per workgroup, 2 workgroups per CU (LDS)
#define CORR_THREADS_BIG 1024              // the second pass over crowded parts: 16 waves, one workgroup per CU
#ifndef CORR_STAGE_DEPTH
#define CORR_STAGE_DEPTH 4                  // staged records per thread in flight (k_correct_fine)
#endif
#define CORR_BIG_SLICES 4                  // workgroups that share the own particles of one crowded part

struct MoveParams {
	double dt_over_h;   // dt / cell_size
	double skin;        // boundary_skin_width / cell_size
	double corr;        // dt * correction_stiffness * re / cell_size   (re = cell_size / sqrt 2)
	double inv_re2;     // cell_size^2 / re^2 = 2
	float *c_home;      // non-null: C lives in its home array, [9][c_home_stride] indexed by the particle id (lfa_sim::c_home)
	size_t c_home_stride;
	int collide;        // 1: the collision handling that follows the move in the reference runs inside the kernel (the default); 0: the
	                    // caller runs it later (lfa_collide), after a host callback that sits between the two in simulation::time_step
};

/// _advect_particles (x += v dt, clamp to [skin, n - skin]) fused with _detect_collisions (from = the old position).
/// tile_solid[t] = tile t holds a solid cell (or padding of a ragged grid, which counts as one)
__global__ void __launch_bounds__(256) k_tile_has_solid(const uint8_t *solid, int nt, uint8_t *tile_solid) {
	for (int t = blockIdx.x; t < nt; t += gridDim.x) {
		const uint8_t *c = solid + (size_t)t * LFA_TILE_CELLS;
		const int any = __syncthreads_or((c[threadIdx.x] | c[threadIdx.x + 256]) != 0);
		if (threadIdx.x == 0) tile_solid[t] = (uint8_t)(any ? 1 : 0);
	}
}
/// tile_clear[t] = no solid cell within one tile of tile t: a particle that starts in t and moves less than 7 cells per axis
/// neither meets one nor ends in a cell with a solid face neighbour, so its collision handling reduces to the domain walls
/// (which the clamp of the advection already enforces). (Less than 8 cells would do for the march alone; the skin push-out
/// looks one cell further.)
__global__ void k_tile_clear(GridDims g, const uint8_t *tile_solid, uint8_t *tile_clear) {
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= g.nt) return;
	int tx, ty, tz;
	tile_coords(g, t, tx, ty, tz);
	int any = 0;
	for (int dz = -1; dz <= 1; ++dz)
		for (int dy = -1; dy <= 1; ++dy)
			for (int dx = -1; dx <= 1; ++dx) {
				const int x = tx + dx, y = ty + dy, z = tz + dz;
				if ((unsigned)x < (unsigned)g.ntx && (unsigned)y < (unsigned)g.nty && (unsigned)z < (unsigned)g.ntz)
					any |= tile_solid[x + g.ntx * (y + g.nty * z)];
			}
	tile_clear[t] = (uint8_t)(any ? 0 : 1);
}

/// One particle of the advection between its loads and its stores. The kernels run three phases - load, move, store - over all
/// of a thread's particles, so that every load is in flight before the first is consumed and none is issued behind a store:
/// stores count in vmcnt on this hardware, and a wait for a load issued after them waits for their acknowledgement too.
struct AdvectSlot {
	uint32_t key;    // in: the old key (0xFFFFFFFF: no particle); out: the new one
	float t[3];      // in: the old fractions; out: the new ones
	float v[3];      // in: the velocity; out (a coerced particle): the source's
	uint32_t clear;  // tile_clear of the old tile
	uint32_t src;    // COERCE: 1 + the coercing source of the old cell, 0 = none
};
/// Load phase, first round trip: what does not depend on the key. Unconditional: the caller clamps an index >= n to a valid one
/// and marks the slot invalid afterwards; the values of an invalid slot are never used.
__device__ inline void advect_load(size_t i, const ParticleSoA &p, AdvectSlot &a) {
	const PosRec me = pos_load(p.pos, i);
	a.key = me.key;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		a.t[d] = me.t[d];
		a.v[d] = p.v[d][i];
	}
}
/// Load phase, second round trip: the bytes the key names (an invalid key reads entry 0 and ignores it).
template <bool COERCE>
__device__ inline void advect_load_by_key(const uint8_t *coerce_map, const uint8_t *tile_clear, AdvectSlot &a) {
	const uint32_t k = a.key != 0xFFFFFFFFu ? a.key : 0u;
	a.clear = tile_clear[k >> 9];
	a.src = COERCE ? (uint32_t)coerce_map[k] : 0u;
}
/// Move phase: registers in, registers out; the only memory it touches is the solid mask of the general collide() march (and
/// the source's velocity of a coerced particle), read-only. Returns the new key (0xFFFFFFFF for an invalid slot).
/// COERCE: the velocity coercion of the fluid sources first (src/simulation.cpp:227-238): a particle inside a cell of an active
/// coercing source takes the source's velocity and C = 0 (the cell is the particle's current one: the reference hashes at the
/// start of the step, :49).
template <bool COERCE>
__device__ inline uint32_t advect_move(AdvectSlot &a, const GridDims &g, const uint8_t *solid, const MoveParams &mp, const float *src_vel) {
	const uint32_t key = a.key;
	if (key == 0xFFFFFFFFu) return key;  // outside this rank's slab (dropped at the next binning)
	int c[3];
	cell_of_key(g, key, c);
	const int nn[3] = {g.nx, g.ny, g.nz};
	if (COERCE && a.src) {
#pragma unroll
		for (int d = 0; d < 3; ++d) a.v[d] = src_vel[3 * (a.src - 1) + d];
	}
	double from[3], to[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		from[d] = (double)c[d] + (double)a.t[d];
		double x = from[d] + (double)a.v[d] * mp.dt_over_h;
		const double lo = mp.skin, hi = (double)nn[d] - mp.skin;
		to[d] = x < lo ? lo : (hi < x ? hi : x);
	}
	// No solid cell within a tile of the start and a move of less than 7 cells per axis: the march of _detect_collisions meets
	// nothing, and of its skin push-out only the domain walls remain - where the clamp above has already left the particle at
	// least `skin` inside (to[d] in [skin, n - skin] => cp >= skin in cell 0, cp <= 1 - skin in cell n - 1). 7, not 8: the
	// push-out looks at the face neighbours of the END cell. A move of less than 8 cells ends in the neighbouring tile at the
	// farthest, but possibly in its far cell layer (7.95 -> 15.93), whose neighbour (cell 16) lies two tiles from the start, where
	// tile_clear says nothing; below 7 cells the end cell is at most 7 + 7 = 14 (or 8 - 7 = 1) and its neighbours are covered.
	// The general path costs a dependent byte load per crossed cell and per near face; most tiles of a scene are nowhere near a
	// solid. Those loads wait for nothing but themselves: no store of any slot has been issued yet.
	const bool open_water = (a.clear & 1) && fabs(to[0] - from[0]) < 7.0 && fabs(to[1] - from[1]) < 7.0 &&
	                        fabs(to[2] - from[2]) < 7.0;
	if (!open_water && mp.collide) collide(g, solid, from, to, mp.skin);
	int nc[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) split_position(to[d], nn[d], nc[d], a.t[d]);
	a.key = blocked_index(g, nc[0], nc[1], nc[2]);
	return a.key;
}
/// Store phase: the position record of a valid slot; of a coerced one the source's velocity and C = 0 as well (rare: its id load
/// is the one load that follows a store).
template <bool COERCE>
__device__ inline void advect_store(size_t i, const ParticleSoA &p, const MoveParams &mp, const AdvectSlot &a) {
	if (a.key == 0xFFFFFFFFu) return;
	pos_store(p.pos, i, a.key, a.t[0], a.t[1], a.t[2]);
	if (COERCE && a.src) {
#pragma unroll
		for (int d = 0; d < 3; ++d) p.v[d][i] = a.v[d];
		if (mp.c_home) {
			const size_t j = p.id[i];
#pragma unroll
			for (int k = 0; k < 9; ++k) mp.c_home[k * mp.c_home_stride + j] = 0.0f;
		} else {
#pragma unroll
			for (int k = 0; k < 9; ++k) p.c[k][i] = 0.0f;
		}
	}
}

template <bool COERCE>
__global__ void __launch_bounds__(256)
k_advect_collide(size_t n, ParticleSoA p, GridDims g, const uint8_t *solid, MoveParams mp, const uint8_t *coerce_map,
                 const float *src_vel, const uint8_t *tile_clear) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	AdvectSlot a;
	advect_load(i, p, a);
	advect_load_by_key<COERCE>(coerce_map, tile_clear, a);
	advect_move<COERCE>(a, g, solid, mp, src_vel);
	advect_store<COERCE>(i, p, mp, a);
}

/// The same with pass 1 of the binning that follows it in lfa_time_step (core.hip: k_tile_count) done on the way: the new keys are
/// in registers, so a wave ranks its AC_CHUNKS x 64 particles inside their new tiles right here (one atomic per distinct tile) and
/// the binning neither reads the keys again nor waits for that pass's returning atomics (0.24 ms at C4).
/// A lane's AC_CHUNKS particles are disjoint indices that no other thread touches, so all of their loads may - and do - come
/// before the first of their stores: two round trips (the keys, fractions and velocities; then the bytes the keys name), the
/// moves, the ranking, and the stores (key, fractions, rank) last.
#define AC_CHUNKS 8  // particles per lane (one after the other: 4: 0.80 ms, 8: 0.74, 16: 0.73 at C4; the plain advection 0.58 + k_tile_count 0.24)
template <bool COERCE>
__global__ void __launch_bounds__(256)
k_advect_collide_count(size_t n, ParticleSoA p, GridDims g, const uint8_t *solid, MoveParams mp, const uint8_t *coerce_map,
                       const float *src_vel, const uint8_t *tile_clear, uint32_t *tile_count, uint32_t *rank) {
	const int lane = threadIdx.x & 63;
	const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const size_t i0 = wave * (64 * AC_CHUNKS) + lane;
	AdvectSlot a[AC_CHUNKS];
	uint32_t tile[AC_CHUNKS], my_rank[AC_CHUNKS];
#pragma unroll
	for (int c = 0; c < AC_CHUNKS; ++c) {
		const size_t i = i0 + 64 * c;
		advect_load(i < n ? i : n - 1, p, a[c]);
	}
#pragma unroll
	for (int c = 0; c < AC_CHUNKS; ++c) {
		if (i0 + 64 * c >= n) a[c].key = 0xFFFFFFFFu;
		advect_load_by_key<COERCE>(coerce_map, tile_clear, a[c]);
	}
#pragma unroll
	for (int c = 0; c < AC_CHUNKS; ++c) {
		const uint32_t k = advect_move<COERCE>(a[c], g, solid, mp, src_vel);
		tile[c] = k != 0xFFFFFFFFu ? k >> 9 : 0xFFFFFFFFu;
	}
	lfa_wave_tile_ranks(tile, tile_count, my_rank);
#pragma unroll
	for (int c = 0; c < AC_CHUNKS; ++c) {
		const size_t i = i0 + 64 * c;
		advect_store<COERCE>(i, p, mp, a[c]);
		if (tile[c] != 0xFFFFFFFFu) rank[i] = my_rank[c];
	}
}

__device__ inline float hash_unit(uint32_t a, uint32_t b, uint32_t k) {
	uint32_t x = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ k * 0xC2B2AE3Du;
	x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
	return (float)(x >> 8) * (2.0f / 16777216.0f) - 1.0f;
}

// ------------------------------------------------------------------------------------------------ position correction
// _correct_positions (src/simulation.cpp:562-610): pairwise springs between particles closer than re = cell / sqrt 2, all from
// the OLD positions, fused with the _detect_collisions that follows it.
// The pair tests are VALU bound and cannot get cheaper per pair, so the lever is the number of candidates. History (C4, a
// moving dam, ms of the tiled kernel): round 1 walked the 27 CELLS around a particle - 216 candidates for 12 partners - 10.5;
// packed fp32 pair math 9.2; per-particle pruning of cells by box distance 62 (divergent loop control costs more than the pairs
// it saves); FINE cells of 0.72 cells, the halo block re-sorted in LDS per workgroup, 81 candidates: 5.8; the force evaluated
// branch-free for every candidate (below): 5.0. This version: fine cells of 8/11 = 0.7273 cells (still >= re = 0.7071),
// ALIGNED with the 8-cell tiles - 11 per axis - so the per-tile index is sorted by fine cell once, by the index kernel (1.02 ms
// instead of 1.17 for the cell index), and a workgroup's block of 13 x 13 x 8 fine cells is put together from contiguous runs
// of its 27 source tiles without atomics or a second pass: per fine row one cell of the x-1 tile, the eleven cells of the own x
// tile (one run), one cell of the x+1 tile, in that order = sorted by fine cell. The kernel itself stayed at 5.0 ms (PMC: 2.3e9
// VALU wave-instructions, 70 % of them the pair walk, 47 of 64 lanes active on average - the lanes of a wave are particles of ~21
// different fine cells whose runs have different lengths; staging 18 %, the per-particle epilogue 11 %).
// Along x the fine cells are HALF as wide, 22 per tile of 8/22 = 0.3636 cells, and a particle walks the five around its own,
// [hx - 2, hx + 2] = 1.82 cells (2 x 0.3636 = 0.7273 >= re, the same margin) instead of three whole ones = 2.18 cells: still nine
// contiguous runs per particle, a sixth fewer candidates. y and z keep the whole fine cells - the runs stay as long as they are.
// A block row is then 26 half cells - two of the x-1 tile, the own 22, two of the x+1 tile - which is the same particles as
// before (two half cells are one fine cell exactly). Measured at C4: 2.10e9 -> 1.90e9 VALU wave-instructions, 4.57 -> 4.22 ms;
// the index kernel, with twice the bins, 0.50 -> 0.54 ms (docs/experiments.md, "half-width fine cells along x").
#define FT 11                                // fine cells per tile axis, y and z
#define FTX (2 * FT)                         // fine (half) cells per tile along x
#define FT3 (FTX * FT * FT)
#define FT_STRIDE (FT3 + 1)                  // per tile: first record of every fine cell + the end
#define FT_INV 1.375f                        // 11 / 8 (exact)
#define FTX_INV 2.75f                        // 22 / 8 (exact)
#define FT_PL ((FT + CORR_PARTS - 1) / CORR_PARTS)  // own fine layers (z) of a part (the last part takes what is left)
#define FB 13                                // block, y and z: the own 11 fine cells + one on each side
#define FBX (FTX + 4)                        // block, x: the own 22 half cells + two on each side
#define FBZ (FT_PL + 2)
#define FB_N (FBX * FB * FBZ)
#define FB_ROWS (FB * FBZ)
#define FINE_CAP 5632                       // staged particles (13 x 13 x 8 whole fine cells hold 4160 at 8 per cell)
#define FINE_CAP_BIG 12288                   // the second pass over flagged parts: 144 KB of positions, one workgroup per CU
// (own particles the u16 list of k_correct_fine holds: 3 072, in the second pass 4 096; more are found through the row offsets)
#define FIDX_THREADS 512   // (256: 0.75 ms at C4, 512: 0.58; FIDX_STAGE and FIDX_CNT are multiples of it)
#define FIDX_CNT (((FT3 + 1 + FIDX_THREADS - 1) / FIDX_THREADS) * FIDX_THREADS)  // index kernel: >= FT3 + 1, a multiple of FIDX_THREADS
#define FIDX_STAGE 4608                      // records staged in LDS per tile by the index kernel (72 KB)

__device__ inline int fine_coord(int l, float t) {
	const int f = (int)(((float)l + t) * FT_INV);
	return f < FT - 1 ? f : FT - 1;  // (t == 1 in the last cell: the max face belongs to the last fine cell)
}
__device__ inline int fine_coord_x(int l, float t) {
	const int f = (int)(((float)l + t) * FTX_INV);
	return f < FTX - 1 ? f : FTX - 1;
}
/// A record of the fine index: the in-cell fractions (exact) + the particle index, and the cell inside the tile in the two top
/// bits of the fractions (a fraction is in [0, 1]: sign and top exponent bit are clear): lx whole (3 bits); of ly, lz the lowest
/// bit - a fine row overlaps two cells per axis at most, floor(8 f / 11) and the next one.
__device__ inline float4 fine_record(int lx, int ly, int lz, float t0, float t1, float t2, uint32_t index) {
	const uint32_t b0 = (__float_as_uint(t0) & 0x3FFFFFFFu) | ((uint32_t)(lx & 3) << 30);
	const uint32_t b1 = (__float_as_uint(t1) & 0x3FFFFFFFu) | ((uint32_t)(lx >> 2) << 31) | ((uint32_t)(ly & 1) << 30);
	const uint32_t b2 = (__float_as_uint(t2) & 0x3FFFFFFFu) | ((uint32_t)(lz & 1) << 31);
	return make_float4(__uint_as_float(b0), __uint_as_float(b1), __uint_as_float(b2), __uint_as_float(index));
}
/// (y0, z0: the first cell the fine row overlaps, floor(8 f / 11))
__device__ inline void fine_decode_at(const float4 &r, int y0, int z0, float t[3], int l[3]) {
	const uint32_t b0 = __float_as_uint(r.x), b1 = __float_as_uint(r.y), b2 = __float_as_uint(r.z);
	t[0] = __uint_as_float(b0 & 0x3FFFFFFFu); t[1] = __uint_as_float(b1 & 0x3FFFFFFFu); t[2] = __uint_as_float(b2 & 0x3FFFFFFFu);
	l[0] = (int)(b0 >> 30) | ((int)(b1 >> 31) << 2);
	l[1] = y0 + ((y0 ^ (int)(b1 >> 30)) & 1);
	l[2] = z0 + ((z0 ^ (int)(b2 >> 31)) & 1);
}
__device__ inline void fine_decode(const float4 &r, int fy, int fz, float t[3], int l[3]) {
	fine_decode_at(r, (8 * fy) / FT, (8 * fz) / FT, t, l);
}

/// Per particle tile: its particles grouped by fine cell - fine_start[tile][f] = first record of fine cell f (absolute), records
/// (fine_record) in spos. (What the reference's _space_hash is to its 27-cell walk, include/fluid/simulation.h:193-197.)
__global__ void __launch_bounds__(FIDX_THREADS, 4)  // (128 VGPRs: two workgroups per CU, what the LDS allows)
k_build_fine_index(const int *ptiles, int n_ptiles, const PosRec *pos, const uint32_t *tile_start, const uint32_t *tile_count, uint32_t *fine_start, float4 *spos, uint32_t *key_copy) {
	// Counters and cursors are relative to the tile's first record. A tile that fits the staging area has at most FIDX_STAGE < 2^16
	// records: its counters are 16 bits wide, two per word (an atomic add on the word bumps one half; a cursor ends at the next
	// cell's start, so the low half never carries into the high one) - the 2 663 of them take the room the 1 332 whole-cell words
	// took, and the kernel stays at two workgroups per CU. A larger tile does not stage, so its counters - whole words, any
	// count - live in the staging area.
	__shared__ uint32_t cnt[FIDX_CNT / 2];
	__shared__ uint32_t wsum[FIDX_THREADS / 64];
	__shared__ float4 stage[FIDX_STAGE];
	static_assert(FIDX_CNT % (2 * FIDX_THREADS) == 0 && FIDX_STAGE % FIDX_THREADS == 0 && FIDX_STAGE < 65536 && FIDX_CNT <= 4 * FIDX_STAGE,
	              "index kernel sizing");
	constexpr int PER = FIDX_CNT / FIDX_THREADS;
	uint32_t *cnt_big = (uint32_t *)stage;
	auto fine_of = [&](uint32_t i, int l[3], float t[3]) -> int {
		const PosRec me = pos_load(pos, i);
		const uint32_t k = me.key;
		l[0] = (int)(k & 7); l[1] = (int)((k >> 3) & 7); l[2] = (int)((k >> 6) & 7);
		t[0] = me.t[0]; t[1] = me.t[1]; t[2] = me.t[2];
		return fine_coord_x(l[0], t[0]) + FTX * (fine_coord(l[1], t[1]) + FT * fine_coord(l[2], t[2]));
	};
	constexpr int RPT = FIDX_STAGE / FIDX_THREADS;  // particles per thread of a tile that fits the staging area: kept in registers
	for (int slot = blockIdx.x; slot < n_ptiles; slot += gridDim.x) {
		const int tile = ptiles[slot];
		// ghost tiles (slab decomposition) keep their particles behind the live ones: the range end comes from the count
		const uint32_t b = tile_start[tile], e = b + tile_count[tile];
		const bool staged = e - b <= FIDX_STAGE;  // (uniform)
		if (staged) {
#pragma unroll
			for (int k = 0; k < PER / 2; ++k) cnt[threadIdx.x + FIDX_THREADS * k] = 0;
		} else {
#pragma unroll
			for (int k = 0; k < PER; ++k) cnt_big[threadIdx.x + FIDX_THREADS * k] = 0;
		}
		__syncthreads();
		// pass 1: histogram. A tile that fits keeps what it has read - (fine cell << 9 | cell in the tile) and the fractions -
		// in registers for pass 2 (reading key and t a second time was a third of the kernel's HBM traffic)
		uint32_t rf[RPT];
		float r0[RPT], r1[RPT], r2[RPT];
		if (staged) {
			// all of the thread's loads first, unconditionally (a slot past the end reads the tile's last record and drops it): a
			// load inside `if (i < e)` is branched around and waited for on its own, RPT round trips where one will do
			const uint32_t last = e > b ? e - 1 : 0u;
#pragma unroll
			for (int r = 0; r < RPT; ++r) {
				const uint32_t i = min(b + threadIdx.x + FIDX_THREADS * r, last);
				const PosRec me = pos_load(pos, i);
				rf[r] = me.key;
				r0[r] = me.t[0]; r1[r] = me.t[1]; r2[r] = me.t[2];
			}
#pragma unroll
			for (int r = 0; r < RPT; ++r) {
				if (b + threadIdx.x + FIDX_THREADS * r < e) {
					const int l[3] = {(int)(rf[r] & 7), (int)((rf[r] >> 3) & 7), (int)((rf[r] >> 6) & 7)};
					const int f = fine_coord_x(l[0], r0[r]) + FTX * (fine_coord(l[1], r1[r]) + FT * fine_coord(l[2], r2[r]));
					rf[r] = ((uint32_t)f << 9) | (uint32_t)(l[0] | (l[1] << 3) | (l[2] << 6));
					atomicAdd(&cnt[f >> 1], 1u << (16 * (f & 1)));
				} else {
					rf[r] = 0xFFFFFFFFu;
				}
			}
		} else {
			for (uint32_t i = b + threadIdx.x; i < e; i += FIDX_THREADS) {
				int l[3];
				float t[3];
				atomicAdd(&cnt_big[fine_of(i, l, t)], 1u);
			}
		}
		__syncthreads();
		// exclusive scan: thread t owns entries PER t .. PER t + PER - 1
		uint32_t c[PER], incl = 0;
#pragma unroll
		for (int k = 0; k < PER; ++k) {
			c[k] = staged ? (cnt[(PER / 2) * threadIdx.x + k / 2] >> (16 * (k & 1))) & 0xFFFFu : cnt_big[PER * threadIdx.x + k];
			incl += c[k];
		}
		const uint32_t sum = incl;
		const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			uint32_t t = __shfl_up(incl, o, 64);
			if (lane >= o) incl += t;
		}
		if (lane == 63) wsum[wid] = incl;
		__syncthreads();
		uint32_t ex = incl - sum;
		for (int w = 0; w < wid; ++w) ex += wsum[w];
		__syncthreads();
#pragma unroll
		for (int k = 0; k < PER; ++k) {
			const int f = PER * threadIdx.x + k;
			// cursor
			if (!staged) cnt_big[f] = ex;
			else if (k & 1) cnt[f >> 1] = (ex - c[k - (k & 1)]) | (ex << 16);
			if (!staged && f <= FT3) fine_start[(size_t)tile * FT_STRIDE + f] = b + ex;  // (a staged tile: after pass 2)
			ex += c[k];
		}
		__syncthreads();
		// pass 2: the records are put in place in LDS and written out as one contiguous run (scattered 16-B stores straight to
		// HBM cost 1.6x); a tile with more particles than the staging area holds reads them again and writes them directly
		if (staged) {
#pragma unroll
			for (int r = 0; r < RPT; ++r)
				if (rf[r] != 0xFFFFFFFFu) {
					const uint32_t f = rf[r] >> 9;
					const uint32_t at = (atomicAdd(&cnt[f >> 1], 1u << (16 * (f & 1))) >> (16 * (f & 1))) & 0xFFFFu;
					stage[at] = fine_record((int)(rf[r] & 7), (int)((rf[r] >> 3) & 7), (int)((rf[r] >> 6) & 7), r0[r], r1[r], r2[r],
					                        b + threadIdx.x + FIDX_THREADS * r);
				}
			// `key_copy`: the keys of before the correction, for its fallback pass and lfa_correct_collide_undo - written here, from
			// registers and together with the other stores (a store between the loads of pass 1 held them up: vmcnt is one
			// in-order counter), instead of by a 2 x 4 Np byte copy of their own
			if (key_copy) {
#pragma unroll
				for (int r = 0; r < RPT; ++r)
					if (rf[r] != 0xFFFFFFFFu) key_copy[b + threadIdx.x + FIDX_THREADS * r] = ((uint32_t)tile << 9) | (rf[r] & 511u);
			}
			__syncthreads();
			// the cells' first records: pass 2 has left the cursor of cell f - 1 at the start of cell f - consecutive threads write
			// consecutive entries (from the scan, a thread's PER entries apiece, the stores were PER words apart)
			for (int f = threadIdx.x; f <= FT3; f += FIDX_THREADS)
				fine_start[(size_t)tile * FT_STRIDE + f] = b + (f ? (cnt[(f - 1) >> 1] >> (16 * ((f - 1) & 1))) & 0xFFFFu : 0u);
			for (uint32_t k = threadIdx.x; k < e - b; k += FIDX_THREADS) spos[b + k] = stage[k];
		} else {
			for (uint32_t i = b + threadIdx.x; i < e; i += FIDX_THREADS) {
				int l[3];
				float t[3];
				const uint32_t at = atomicAdd(&cnt_big[fine_of(i, l, t)], 1u);
				spos[b + at] = fine_record(l[0], l[1], l[2], t[0], t[1], t[2], i);
				if (key_copy) key_copy[i] = pos[i].key;
			}
		}
		__syncthreads();
	}
}

/// Where block fine cell (gx, gy, gz) - own-tile fine coordinates, -2 .. FTX + 1 in x, -1 .. FT in y and z - lives: the source tile
/// (-1: none) and its fine coordinates there.
__device__ inline int fine_source(const GridDims &g, const uint32_t *tile_count, int tx, int ty, int tz, int gx, int gy, int gz, int &fx,
                                  int &fy, int &fz) {
	const int dx = gx < 0 ? -1 : (gx >= FTX ? 1 : 0), dy = gy < 0 ? -1 : (gy >= FT ? 1 : 0), dz = gz < 0 ? -1 : (gz >= FT ? 1 : 0);
	fx = gx - FTX * dx; fy = gy - FT * dy; fz = gz - FT * dz;
	const int x = tx + dx, y = ty + dy, z = tz + dz;
	if ((unsigned)x >= (unsigned)g.ntx || (unsigned)y >= (unsigned)g.nty || (unsigned)z >= (unsigned)g.ntz) return -1;
	const int tile = x + g.ntx * (y + g.nty * z);
	return tile_count[tile] ? tile : -1;  // (tile_flag marks the DILATED set: only tiles with particles have an index)
}

/// One record of the fallback pass below.
__device__ inline void correct_collide_record(size_t rk, const ParticleSoA &p, PosRec *out, const GridDims &g, const uint8_t *solid, const uint32_t *tile_count, const uint32_t *fine_start,
                                              const float4 *spos, const MoveParams &mp, const uint32_t *only_flagged, const int *tile_pslot,
                                              int p_off, const uint32_t *key_before) {
	const float4 me = spos[rk];
	const size_t i = __float_as_uint(me.w);
	const uint32_t key_i = key_before ? key_before[i] : p.pos[i].key;
	if (key_i == 0xFFFFFFFFu) return;
	const int tile = (int)(key_i >> 9);
	const int l[3] = {(int)(key_i & 7), (int)((key_i >> 3) & 7), (int)((key_i >> 6) & 7)};
	const float t[3] = {__uint_as_float(__float_as_uint(me.x) & 0x3FFFFFFFu), __uint_as_float(__float_as_uint(me.y) & 0x3FFFFFFFu),
	                    __uint_as_float(__float_as_uint(me.z) & 0x3FFFFFFFu)};
	const int f[3] = {fine_coord_x(l[0], t[0]), fine_coord(l[1], t[1]), fine_coord(l[2], t[2])};
	if (only_flagged) {
		const int work = CORR_PARTS * (tile_pslot[tile] - p_off) + f[2] / FT_PL;
		if (!((only_flagged[1 + (work >> 5)] >> (work & 31)) & 1u)) return;
	}
	int tx, ty, tz;
	tile_coords(g, tile, tx, ty, tz);
	const int nn[3] = {g.nx, g.ny, g.nz};
	const float inv_re2 = (float)mp.inv_re2;
	double spring[3] = {0.0, 0.0, 0.0};
	for (int dz = -1; dz <= 1; ++dz)
		for (int dy = -1; dy <= 1; ++dy)
			for (int dx = -2; dx <= 2; ++dx) {  // (the five half cells of the tiled kernel's x-run, one at a time)
				int sf[3];
				const int src = fine_source(g, tile_count, tx, ty, tz, f[0] + dx, f[1] + dy, f[2] + dz, sf[0], sf[1], sf[2]);
				if (src < 0) continue;
				const uint32_t *fs = fine_start + (size_t)src * FT_STRIDE + (sf[0] + FTX * (sf[1] + FT * sf[2]));
				const uint32_t kb = fs[0], ke = fs[1];
				int stx, sty, stz;
				tile_coords(g, src, stx, sty, stz);
				for (uint32_t k = kb; k < ke; ++k) {
					const float4 rec = spos[k];  // the neighbours' OLD positions (the outputs go back in place)
					if (__float_as_uint(rec.w) == (uint32_t)i) continue;
					float nt[3];
					int nl[3];
					fine_decode(rec, sf[1], sf[2], nt, nl);
					const float ddx = ((float)(8 * (tx - stx) + l[0] - nl[0]) + t[0]) - nt[0];
					const float ddy = ((float)(8 * (ty - sty) + l[1] - nl[1]) + t[1]) - nt[1];
					const float ddz = ((float)(8 * (tz - stz) + l[2] - nl[2]) + t[2]) - nt[2];
					const float d2 = ddx * ddx + ddy * ddy + ddz * ddz;  // grid units^2
					if (d2 < 1e-12f) {
						// coincident pair: the reference adds a random unit-box vector (:584-587, std::random_device)
						const uint32_t j = __float_as_uint(rec.w);
						spring[0] += hash_unit((uint32_t)i, j, 0); spring[1] += hash_unit((uint32_t)i, j, 1);
						spring[2] += hash_unit((uint32_t)i, j, 2);
					} else {
						const float kl = 1.0f - d2 * inv_re2;
						if (kl > 0.0f) {
							const float fr = kl * kl * kl * rsqrtf(d2);
							spring[0] += (double)(fr * ddx); spring[1] += (double)(fr * ddy); spring[2] += (double)(fr * ddz);
						}
					}
				}
			}
	const int c[3] = {8 * tx + l[0], 8 * ty + l[1], 8 * tz + l[2]};
	double from[3], to[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		from[d] = (double)c[d] + (double)t[d];
		double x = from[d] + spring[d] * mp.corr;
		to[d] = x < 0.0 ? 0.0 : ((double)nn[d] < x ? (double)nn[d] : x);  // clamp to [offset, grid max] (:604-609)
	}
	if (mp.collide) collide(g, solid, from, to, mp.skin);
	int nc[3];
	float ntt[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) split_position(to[d], nn[d], nc[d], ntt[d]);
	pos_store(out, i, blocked_index(g, nc[0], nc[1], nc[2]), ntt[0], ntt[1], ntt[2]);
}

/// _correct_positions + _detect_collisions for the particles of the flagged half tiles (those the LDS-tiled kernel could not
/// hold) - or, without a flag bitmap, of all: a thread per particle gathers its 27 fine cells from the index in global memory.
/// `n` = live particles = records of the owned tiles (ghost tiles' records lie behind them).
__global__ void __launch_bounds__(256)
k_correct_collide(size_t n, ParticleSoA p, PosRec *out, GridDims g,
                   const uint8_t *solid, const uint32_t *tile_count, const uint32_t *fine_start, const float4 *spos, MoveParams mp,
                   const uint32_t *only_flagged, const int *tile_pslot, int p_off, const uint32_t *key_before) {
	// A thread per RECORD of the index: everything about the particle as it was BEFORE the correction - the tiled kernel has
	// already rewritten, in place, key and fractions of the particles it moved, and which part a particle belongs to depends on
	// its old fraction - comes from the record (fractions, index) and the copy of the old keys.
	if (only_flagged && only_flagged[0] == 0) return;  // (word 0 counts the flagged parts: none, as a rule - the grid is bounded, so that
	                                                     // costs a few thousand workgroups, not n / 256)
	for (size_t rk = (size_t)blockIdx.x * blockDim.x + threadIdx.x; rk < n; rk += (size_t)gridDim.x * blockDim.x)
		correct_collide_record(rk, p, out, g, solid, tile_count, fine_start, spos, mp, only_flagged, tile_pslot,
		                       p_off, key_before);
}

/// LDS-tiled _correct_positions + _detect_collisions on the fine index. One workgroup per (particle tile, z part): part 0 moves the
/// particles of FT_PL fine layers (the last part of what is left); the block staged in LDS is those layers + one fine cell all around
/// (along x: two half cells).
/// CAP: staged particles. <FINE_CAP, false> is the pass over every part (two workgroups per CU); <FINE_CAP_BIG, true> takes the parts
/// the first pass has flagged in `only` (word 0: how many; a crowded neighbourhood late in a run) with the whole LDS of a CU to
/// itself, and flags what does not fit even that for the global-gather kernel.
#ifdef CORR_PROFILE
// (variant builds only: where a work item's time goes - wall-clock ticks of thread 0 summed over the work items of every launch)
__device__ unsigned long long g_corr_prof[8];
#define CORR_STAMP(k)                                                                   \
	do {                                                                                \
		if (!ONLY && threadIdx.x == 0) {                                                \
			const unsigned long long now_ = wall_clock64();                             \
			atomicAdd(&g_corr_prof[k], now_ - stamp_);                                  \
			stamp_ = now_;                                                              \
		}                                                                               \
	} while (0)
#else
#define CORR_STAMP(k) do { } while (0)
#endif
// (Budget, both instantiations: <= 128 VGPRs - the 4 waves per SIMD asked for below -, no scratch, static LDS <= 81 920 B for the
// first pass (two workgroups per CU) and <= 163 840 B for the second. The compiler spills silently beyond 128:
// tests/test_kernel_budgets.py reads the figures from the compiler's metadata.)
template <int CAP, bool ONLY>
__global__ void __launch_bounds__(ONLY ? CORR_THREADS_BIG : CORR_THREADS, 4)
k_correct_fine(const int *ptiles, int n_ptiles, PosRec *out, GridDims g,
                const uint8_t *solid, const uint32_t *tile_count, const uint32_t *fine_start, const float4 *spos, MoveParams mp,
                uint32_t *overflow_tiles, const uint8_t *tile_clear, const uint32_t *only) {
	constexpr int T = ONLY ? CORR_THREADS_BIG : CORR_THREADS;  // threads of the workgroup
	constexpr int CNT0 = ((FB_N + 1 + 2 * T - 1) / (2 * T)) * (2 * T);  // >= FB_N + 1, a multiple of 2 T: the cells take CNT / 2 T rounds
	constexpr int CNT = ONLY && CNT0 < 4096 ? 4096 : CNT0;  // own particles listed (the second pass has the room for 4 096)
	__shared__ float px[CAP], py[CAP], pz[CAP];
	__shared__ uint16_t own[CNT];              // the own list: staged slots of the part's own particles, in fine-cell order
	__shared__ uint32_t foff2[(FB_N + 2) / 2]; // first staged slot of every block fine cell + the end, two per word
	const uint16_t *foff = (const uint16_t *)foff2;
	// Per fine row of the block, everything the staging derives from the row alone: four words read as one 128-bit load,
	// [0..2] source record of staged slot s in the row's three runs (x-1 tile, own x tile, x+1 tile) is base[seg] + s
	// [3]    first slot of the own x run | first slot of the x+1 run << 16
	// and one packed word (the half cells doubled count and offset arrays: the descriptors gave the LDS back),
	// bits 0-2, 3-5  y0, z0: first cell of the fine row (fine_decode)     bits 6-10, 11-15  8 (dy + 1), 8 (dz + 1): the source
	// tile's offset in cells     bits 16-31  own list: a slot s of the own x run is entry (signed) + s; ROW_NOT_OWN: not listed
	__shared__ __attribute__((aligned(16))) uint32_t rowd[FB_ROWS * 4];
	__shared__ uint32_t rowe[FB_ROWS];
	constexpr int ROW_NOT_OWN = -32768;  // (a listed base is within -CAP .. CNT: 16 bits, signed)
	__shared__ uint32_t ownoff[FT * FT_PL + 1];
	__shared__ int srct[27];                   // the source tiles around the own one
	__shared__ uint32_t wsum[T / 64];
	static_assert(CNT > FB_N && CNT % (2 * T) == 0 && FBX % 2 == 0 && CAP < 32768 && CNT < 32768, "own list and cell rounds sizing");
	const int nn[3] = {g.nx, g.ny, g.nz};
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	if (ONLY && only[0] == 0) return;  // (as a rule)
	// (second pass: CORR_BIG_SLICES workgroups per crowded part, each stages the block and moves every CORR_BIG_SLICES-th round of
	// its own particles - the pair work of such a part is several times a normal one's, and there are fewer of them than CUs)
	constexpr int SLICES = ONLY ? CORR_BIG_SLICES : 1;
	for (int item = blockIdx.x; item < SLICES * CORR_PARTS * n_ptiles; item += gridDim.x) {
		int work = item / SLICES;
		const int slice = item % SLICES;
		// (first pass: workgroups are handed to the eight XCDs in turn, and the parts of a tile write interleaved halves of the same
		// lines of the outputs and stage two fine layers in common - so they are items 8 apart, on one XCD and one L2: of every
		// 8 CORR_PARTS items the first eight are part 0 of eight tiles, the next eight their part 1. The tiles left over at the end
		// keep item = work. The grid is a multiple of 8 or the whole of the items. Measured at C4: 4.19 -> 3.91 ms, the bytes
		// written to HBM halved; four consecutive tiles with both parts per XCD instead: 3.96. docs/experiments.md, "cheaper block
		// set-up".)
		if (!ONLY && (item / (8 * CORR_PARTS)) * 8 + 8 <= n_ptiles)
			work = CORR_PARTS * ((item / (8 * CORR_PARTS)) * 8 + item % 8) + (item % (8 * CORR_PARTS)) / 8;
		if (ONLY && !((only[1 + (work >> 5)] >> (work & 31)) & 1u)) continue;  // (uniform)
		const int tile = ptiles[work / CORR_PARTS], part = work % CORR_PARTS;
		int tx, ty, tz;
		tile_coords(g, tile, tx, ty, tz);
		const int own_lo = part * FT_PL, own_n = (own_lo + FT_PL <= FT ? FT_PL : FT - own_lo);
		const int gz0 = own_lo - 1;  // own-tile fine layer of block layer 0
		const int nzb = own_n + 2;   // block layers
		const int nrows = FB * nzb, nown_rows = FT * (nzb - 2);
		const bool open_water = (tile_clear[tile] & 1) != 0;  // no solid cell within a tile of this one
		// every cell c of the tile has c - 7 >= 1 and c + 7 <= n - 2 on all three axes, and collisions are on in open water (uniform)
		const bool lean = open_water && mp.collide && tx >= 1 && ty >= 1 && tz >= 1 && 8 * tx + 16 <= g.nx && 8 * ty + 16 <= g.ny &&
		                  8 * tz + 16 <= g.nz;
		__syncthreads();
#ifdef CORR_PROFILE
		unsigned long long stamp_ = wall_clock64();
		if (!ONLY && threadIdx.x == 0) atomicAdd(&g_corr_prof[7], 1ull);
#endif
		// ---- the 27 source tiles (-1: outside the grid or without particles), then the block's fine cells: where their records
		// are, how many
		// (the thread index behind an empty asm: what the first few threads derive from it - the source tiles, the row descriptors -
		// is a handful of instructions per work item; hoisted out of the work-item loop it would occupy registers across the
		// pair walk)
		uint32_t tid = threadIdx.x;
		asm volatile("" : "+v"(tid));
		if (tid < 27) {
			int fx, fy, fz;
			srct[tid] = fine_source(g, tile_count, tx, ty, tz, FTX * ((int)tid % 3 - 1), FT * (((int)tid / 3) % 3 - 1), FT * ((int)tid / 9 - 1), fx,
			                        fy, fz);
		}
		__syncthreads();
		// A source tile's index IS a prefix sum (fine_start), and a block row is three contiguous runs of it - two half cells of the
		// x-1 tile, the own x tile's 22, two of the x+1 tile: the first staged slot of a block cell is fine_start[its source cell]
		// minus the run's base (first source record - first slot, what the row descriptor holds anyway). Only the rows' three run
		// lengths are scanned, by the rows' threads; nothing is counted per cell. (Before: a count per cell, scanned six per thread -
		// 356 static VALU per work item.)
		// (a thread takes two neighbouring half cells, bx even and bx + 1: they lie in the same source tile - the block's x halo is
		// two half cells, the own run 22 - next to each other in its index: one look-up, two loads. They are issued here, together
		// with the rows' loads, and wait in registers for the bases)
		constexpr int ROUNDS = CNT / (2 * T), KEPT = ROUNDS - 1 < 2 ? ROUNDS - 1 : 2;
		uint32_t fs0[ROUNDS], fs1[ROUNDS];
		int fbase[ROUNDS];  // the cell's run in rowd; -1: a cell behind the last row
#pragma unroll
		for (int k = 0; k < ROUNDS; ++k) {
			// (all but the first KEPT rounds' cell coordinates are worked out per work item, not kept in registers across the loop: see `tid`)
			const int p = (int)(k >= KEPT ? tid : threadIdx.x) + T * k;
			fs0[k] = 0; fs1[k] = 0; fbase[k] = -1;
			if (p < (FBX / 2) * nrows) {
				const int bx = 2 * (p % (FBX / 2)), row = p / (FBX / 2), by = row % FB, bz = row / FB;
				const int gx = bx - 2, gy = by - 1, gz = gz0 + bz;
				const int dx = gx < 0 ? 0 : (gx >= FTX ? 2 : 1), dy = gy < 0 ? 0 : (gy >= FT ? 2 : 1), dz = gz < 0 ? 0 : (gz >= FT ? 2 : 1);
				const int src = srct[dx + 3 * dy + 9 * dz];
				fbase[k] = row * 4 + dx;
				if (src >= 0) {  // (a tile without particles: an empty run, whose base is minus its first slot)
					const uint32_t fid = (uint32_t)((gx - FTX * (dx - 1)) + FTX * ((gy - FT * (dy - 1)) + FT * (gz - FT * (dz - 1))));
					const uint32_t *fs = fine_start + ((uint32_t)src * FT_STRIDE + fid);  // (nt * FT_STRIDE < 2^32 up to 1.6 M tiles)
					fs0[k] = fs[0]; fs1[k] = fs[1];
				}
			}
		}
		// ---- the rows: thread r has row r's three runs - first source record, length - and, for an own row (by = 1 .. FT,
		// bz = 1 .. nzb - 2), the length of its middle run = its own particles. Two scans in one go over the first two waves: the
		// rows' first slots and the own rows' first list entries (own rows come in list order).
		static_assert(FB_ROWS <= 128 && T >= 256, "the rows are the first two waves; wsum holds two sums of each scan");
		uint32_t run_at[3] = {0, 0, 0}, run_n[3] = {0, 0, 0}, row_incl = 0, own_incl = 0, row_n = 0, own_len = 0;
		int own_row = -1;  // which own row this thread's row is
		uint32_t rowe_lo = 0;
		if (tid < 128u) {  // (whole waves: the shuffles need every lane)
			const int r = (int)tid, by = r % FB, bz = r / FB;
			const int gy = by - 1, gz = gz0 + bz;
			const int dy = gy < 0 ? -1 : (gy >= FT ? 1 : 0), dz = gz < 0 ? -1 : (gz >= FT ? 1 : 0);
			const int fy = gy - FT * dy, fz = gz - FT * dz;
			if (r < nrows) {
				const uint32_t frow = (uint32_t)(FTX * (fy + FT * fz));
#pragma unroll
				for (int seg = 0; seg < 3; ++seg) {
					const int src = srct[seg + 3 * (dy + 1) + 9 * (dz + 1)];
					if (src >= 0) {
						const uint32_t *fs = fine_start + ((uint32_t)src * FT_STRIDE + frow + (seg == 0 ? FTX - 2 : 0));
						run_at[seg] = fs[0];
						run_n[seg] = fs[seg == 1 ? FTX : 2] - run_at[seg];  // (frow + FTX <= FT3: the entry behind the tile's last cell)
					}
				}
				row_n = run_n[0] + run_n[1] + run_n[2];
				if (by >= 1 && by <= FT && bz >= 1 && bz <= nzb - 2) {
					own_row = (by - 1) + FT * (bz - 1);
					own_len = run_n[1];
				}
				rowe_lo = (uint32_t)((8 * fy) / FT) | ((uint32_t)((8 * fz) / FT) << 3) | ((uint32_t)(8 * (dy + 1)) << 6) | ((uint32_t)(8 * (dz + 1)) << 11);
			}
			row_incl = row_n; own_incl = own_len;
#pragma unroll
			for (int o = 1; o < 64; o <<= 1) {
				const uint32_t t = __shfl_up(row_incl, o, 64), u = __shfl_up(own_incl, o, 64);
				if (lane >= o) { row_incl += t; own_incl += u; }
			}
			if (lane == 63) { wsum[wid] = row_incl; wsum[2 + wid] = own_incl; }
		}
		__syncthreads();
		// (32-bit sums of disjoint record runs: no cell, however crowded, wraps them)
		const uint32_t total = wsum[0] + wsum[1], own_total = wsum[2] + wsum[3];
		if (total > (uint32_t)CAP) {  // uniform
			if (threadIdx.x == 0 && slice == 0) {
				atomicOr(&overflow_tiles[1 + (work >> 5)], 1u << (work & 31));
				atomicAdd(&overflow_tiles[0], 1u);
			}
			continue;
		}
		// (a crowded part with more own particles than the list holds finds them through the row offsets instead: uniform)
		const bool listed = own_total <= (uint32_t)CNT;
		// ---- the row descriptors, and the own rows' first list entries
		if (tid < (unsigned)nrows) {
			const uint32_t d0 = (wid ? wsum[0] : 0u) + row_incl - row_n, d1 = d0 + run_n[0], d2 = d1 + run_n[1];
			*(uint4 *)(rowd + tid * 4) = make_uint4(run_at[0] - d0, run_at[1] - d1, run_at[2] - d2, d1 | (d2 << 16));
			uint32_t ob = (uint32_t)ROW_NOT_OWN;
			if (own_row >= 0) {
				const uint32_t own_first = (wid ? wsum[2] : 0u) + own_incl - own_len;  // list entry of the row's first own particle
				ownoff[own_row] = own_first;
				if (listed) ob = own_first - d1;
			}
			rowe[tid] = rowe_lo | (ob << 16);
		}
		if (tid == 0) ownoff[nown_rows] = own_total;
		__syncthreads();
		// ---- first staged slot of every block fine cell; the cells behind the last row, and the entry behind the last cell: `total`
#pragma unroll
		for (int k = 0; k < ROUNDS; ++k) {
			const int p = (int)(k >= KEPT ? tid : threadIdx.x) + T * k;
			if (p < (FB_N + 2) / 2) {
				const uint32_t base = fbase[k] >= 0 ? rowd[fbase[k]] : 0u - total;
				foff2[p] = ((fs0[k] - base) & 0xFFFFu) | ((fs1[k] - base) << 16);
			}
		}
		__syncthreads();
		CORR_STAMP(0);  // counts, scans, own offsets
		// ---- stage the rows: their three runs - two half cells of the x-1 tile, the own x tile's 22, two of the x+1 tile - follow
		// each other in the block (positions relative to the own tile's origin, in cells)
		// Flat: a thread per staged SLOT - every thread's record load is issued at once, CORR_STAGE_DEPTH per thread in flight.
		// (Round 5 and before: a wave per fine row, one row after the other - 13 dependent HBM round trips per wave and work
		// item. Measured, round 6: C4 4.91 -> 4.84 ms, the late C3 sheet 2.07 -> 1.89; 2, 4 or 8 records in flight make no
		// difference - the kernel is bound by its instruction count, not by this latency.)
		// A slot's row: the 64 slots of a wave are consecutive, so the rows of its first and last slot come from ballots over
		// the rows' first slots (lane l holds those of rows l and l + 64; they are monotone: a population count is a row), and
		// a lane searches between the two only - no step inside a long row, one or two in a dense block. Rows can be empty,
		// several in a row: the search takes the last row that starts at or before the slot, which is the one that holds it.
		{
			static_assert(FB_ROWS <= 128, "two row starts per lane");
			const int rl = (int)(tid & 63u);
			const uint32_t rs_lo = rl < nrows ? (uint32_t)foff[rl * FBX] : 0xFFFFFFFFu;
			const uint32_t rs_hi = rl + 64 < nrows ? (uint32_t)foff[(rl + 64) * FBX] : 0xFFFFFFFFu;
			auto row_of = [&](uint32_t s) -> int {  // (every lane of the wave calls it, s uniform)
				return (int)__popcll(__ballot(rs_lo <= s)) + (int)__popcll(__ballot(rs_hi <= s)) - 1;
			};
			auto locate = [&](uint32_t slot, int r_first, int r_last, uint32_t &src, int &rs) {
				int r = r_first;
				const int span = r_last - r_first;  // (uniform)
				for (int step = span ? 1 << (31 - __builtin_clz(span)) : 0; step; step >>= 1) {
					const int c = r + step;
					if (c <= r_last && (uint32_t)foff[c * FBX] <= slot) r = c;
				}
				const uint4 d = *(const uint4 *)(rowd + r * 4);
				const int seg = slot < (d.w & 0xFFFFu) ? 0 : (slot < (d.w >> 16) ? 1 : 2);
				src = (seg == 0 ? d.x : (seg == 1 ? d.y : d.z)) + slot;
				rs = r | (seg << 8);
			};
			auto put = [&](uint32_t slot, const float4 &rec, int rs) {
				const int r = rs & 255, seg = rs >> 8;
				const uint32_t d = rowe[r];
				const int ob = (int)d >> 16;
				float t[3];
				int l[3];
				fine_decode_at(rec, (int)(d & 7u), (int)((d >> 3) & 7u), t, l);
				px[slot] = (float)(8 * (seg - 1) + l[0]) + t[0];
				py[slot] = (float)((int)((d >> 6) & 31u) - 8 + l[1]) + t[1];
				pz[slot] = (float)((int)((d >> 11) & 31u) - 8 + l[2]) + t[2];
				if (seg == 1 && ob != ROW_NOT_OWN) own[ob + (int)slot] = (uint16_t)slot;  // the own list: slot order = fine-cell order
			};
			// CORR_STAGE_DEPTH records per thread in flight (a dense item stages ~3 600 = 7 per thread)
			const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
			for (uint32_t w0 = wave0; w0 < total; w0 += CORR_STAGE_DEPTH * T) {  // (uniform per wave: the ballots need every lane)
				uint32_t src[CORR_STAGE_DEPTH];
				int rs[CORR_STAGE_DEPTH];  // row | seg << 8
				float4 rec[CORR_STAGE_DEPTH];
#pragma unroll
				for (int u = 0; u < CORR_STAGE_DEPTH; ++u) {
					const uint32_t wu = w0 + u * T, slot = wu + lane;
					src[u] = 0; rs[u] = 0;
					if (wu < total) {
						const uint32_t last = wu + 63 < total ? wu + 63 : total - 1;
						const int r_first = row_of(wu), r_last = row_of(last);
						if (slot < total) locate(slot, r_first, r_last, src[u], rs[u]);
					}
				}
#pragma unroll
				for (int u = 0; u < CORR_STAGE_DEPTH; ++u) rec[u] = spos[src[u]];  // (src 0 for a slot beyond the end: any valid record)
#pragma unroll
				for (int u = 0; u < CORR_STAGE_DEPTH; ++u) {
					const uint32_t slot = w0 + u * T + lane;
					if (slot < total) put(slot, rec[u], rs[u]);
				}
			}
		}
		__syncthreads();
		CORR_STAMP(1);  // staging
#ifdef CORR_PROFILE
		if (!ONLY && threadIdx.x == 0) { atomicAdd(&g_corr_prof[5], (unsigned long long)total); atomicAdd(&g_corr_prof[6], (unsigned long long)own_total); }
#endif
		for (uint32_t w = threadIdx.x + T * slice; w < own_total; w += T * SLICES) {
			uint32_t me;
			if (listed) {
				me = own[w];
			} else {  // the own row that holds the w-th own particle: last r with ownoff[r] <= w
				int lo = 0, hi = nown_rows - 1;
				while (lo < hi) {
					const int mid = (lo + hi + 1) >> 1;
					if (ownoff[mid] <= w) lo = mid;
					else hi = mid - 1;
				}
				me = (uint32_t)foff[((1 + lo % FT) + FB * (1 + lo / FT)) * FBX + 2] + (w - ownoff[lo]);
			}
#ifdef CORR_PROFILE
			const unsigned long long w0_ = wall_clock64();
#endif
			const float mx = px[me], my = py[me], mz = pz[me];
			// block coordinates of its fine cell (the same arithmetic the index was built with: mx = (float)lx + t exactly)
			int fx = (int)(mx * FTX_INV), fy = (int)(my * FT_INV), fz = (int)(mz * FT_INV);
			fx = fx < FTX - 1 ? fx : FTX - 1; fy = fy < FT - 1 ? fy : FT - 1; fz = fz < FT - 1 ? fz : FT - 1;
			const int bx = fx + 2, by = fy + 1, bz = fz - gz0;
			float sx = 0.f, sy = 0.f, sz = 0.f;
			typedef float f2 __attribute__((ext_vector_type(2)));
			f2 s2x = 0.f, s2y = 0.f, s2z = 0.f;
			const float inv_re2 = (float)mp.inv_re2;
			uint32_t j = 0xFFFFFFFFu;  // (the coincidence hash needs the particle's index: loaded by the rare branch only)
			const uint32_t myrow = by + FB * bz;
			const uint32_t grec = rowd[myrow * 4 + 1] + me;
			auto pair2 = [&](uint32_t q, f2 qx, f2 qy, f2 qz) {
				const f2 dx = mx - qx, dy = my - qy, dz = mz - qz;
				const f2 d2 = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
				const f2 kl = __builtin_elementwise_fma(-d2, (f2)inv_re2, (f2)1.0f);
				if (kl.x > 0.0f || kl.y > 0.0f) {
#pragma unroll
					for (int k = 0; k < 2; ++k) {
						const float d2k = k ? d2.y : d2.x, klk = k ? kl.y : kl.x;
						if (!(klk > 0.0f)) continue;
						if (d2k < 1e-12f) {
							// coincident (or the particle itself): the reference adds a random unit-box vector (:584-587)
							if (q + k != me) {
								if (j == 0xFFFFFFFFu) j = __float_as_uint(spos[grec].w);
								sx += hash_unit(j, q + k, 0); sy += hash_unit(j, q + k, 1); sz += hash_unit(j, q + k, 2);
							}
						} else {
							const float f = klk * klk * klk * rsqrtf(d2k);
							sx += f * (k ? dx.y : dx.x); sy += f * (k ? dy.y : dy.x); sz += f * (k ? dz.y : dz.x);
						}
					}
				}
			};
			// The nine x-runs of five half cells around the particle (always inside the block); `p2` takes two candidates at a time
			// (a far-away dummy pads an odd tail: it contributes exactly 0).
			auto walk = [&](auto &&p2, auto &&p2_centre) {
				for (int dz = -1; dz <= 1; ++dz)
					for (int dy = -1; dy <= 1; ++dy) {
						const int rowf = FBX * ((by + dy) + FB * (bz + dz)) + bx;
						const uint32_t b = foff[rowf - 2], e = foff[rowf + 3];
						auto run = [&](auto &&pp) {
							uint32_t q = b;
							for (; q + 4 <= e; q += 4) {
								const float x0 = px[q], x1 = px[q + 1], x2 = px[q + 2], x3 = px[q + 3];
								const float y0 = py[q], y1 = py[q + 1], y2 = py[q + 2], y3 = py[q + 3];
								const float z0 = pz[q], z1 = pz[q + 1], z2 = pz[q + 2], z3 = pz[q + 3];
								pp(q, f2{x0, x1}, f2{y0, y1}, f2{z0, z1});
								pp(q + 2, f2{x2, x3}, f2{y2, y3}, f2{z2, z3});
							}
							if (q + 2 <= e) {
								pp(q, f2{px[q], px[q + 1]}, f2{py[q], py[q + 1]}, f2{pz[q], pz[q + 1]});
								q += 2;
							}
							if (q < e) pp(q, f2{px[q], 1e6f}, f2{py[q], 1e6f}, f2{pz[q], 1e6f});
						};
						if (dy == 0 && dz == 0) run(p2_centre);  // (uniform) the run that holds the particle itself
						else run(p2);
					}
			};
			// Fast walk, no branch per candidate: the force is evaluated for every candidate with the kernel clamped at 0 - the same
			// sums, since fma(0, d, s) == s. The self pair (d = 0 exactly) contributes 0 through d^2 + 1e-30. What this cannot do
			// is the reference's random push for COINCIDENT pairs (d^2 < 1e-12, :584-587): a lane that has met one - a d^2 below
			// the threshold in the eight other runs (running minimum), or a second one in its own run (count) - redoes its
			// particle with the branching walk. (With ~0.72-cell fine cells one candidate in seven is a partner and a wave tests
			// 128 per step: a "nobody has a partner" branch around the force is almost never skipped - measured: 5.77 -> 5.00 ms.)
			float d2_min = 1.0f;
			uint32_t n_tiny = 0;
			auto fast = [&](f2 qx, f2 qy, f2 qz) -> f2 {
				const f2 dx = mx - qx, dy = my - qy, dz = mz - qz;
				const f2 d2 = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, __builtin_elementwise_fma(dx, dx, (f2)1e-30f)));
				f2 kl;
				kl.x = __builtin_amdgcn_fmed3f(__builtin_fmaf(-d2.x, inv_re2, 1.0f), 0.0f, 1.0f);
				kl.y = __builtin_amdgcn_fmed3f(__builtin_fmaf(-d2.y, inv_re2, 1.0f), 0.0f, 1.0f);
				f2 f = kl * kl * kl;
				f.x *= __builtin_amdgcn_rsqf(d2.x);  // d^2 >= 1e-30: a normal number, the bare v_rsq_f32 (what rsqrtf compiles to
				f.y *= __builtin_amdgcn_rsqf(d2.y);  // behind the d^2 >= 1e-12 test of the branching walk)
				s2x = __builtin_elementwise_fma(f, dx, s2x);
				s2y = __builtin_elementwise_fma(f, dy, s2y);
				s2z = __builtin_elementwise_fma(f, dz, s2z);
				return d2;
			};
			walk([&](uint32_t, f2 qx, f2 qy, f2 qz) {
					     const f2 d2 = fast(qx, qy, qz);
					     d2_min = fminf(d2_min, fminf(d2.x, d2.y));
				     },
				     [&](uint32_t, f2 qx, f2 qy, f2 qz) {
					     const f2 d2 = fast(qx, qy, qz);
					     n_tiny += (d2.x < 1e-12f ? 1u : 0u) + (d2.y < 1e-12f ? 1u : 0u);
				     });
			if (d2_min < 1e-12f || n_tiny != 1u) {  // rare
				s2x = 0.f; s2y = 0.f; s2z = 0.f;
				walk(pair2, pair2);
			}
			sx += s2x.x + s2x.y;
			sy += s2y.x + s2y.y;
			sz += s2z.x + s2z.y;
#ifdef CORR_PROFILE
			if (!ONLY && threadIdx.x == 0) atomicAdd(&g_corr_prof[4], wall_clock64() - w0_);
#endif
			// the particle's exact cell and fractions (the staged copy is tile-relative fp32) and its index
			float tme[3];
			int lme[3];
			const float4 rec = spos[grec];
			const uint32_t yz = rowe[myrow];
			fine_decode_at(rec, (int)(yz & 7u), (int)((yz >> 3) & 7u), tme, lme);
			const uint32_t jj = __float_as_uint(rec.w);
			const int c[3] = {8 * tx + lme[0], 8 * ty + lme[1], 8 * tz + lme[2]};
			const double spring[3] = {(double)sx, (double)sy, (double)sz};
			double from[3], to[3];
#pragma unroll
			for (int d = 0; d < 3; ++d) {
				from[d] = (double)c[d] + (double)tme[d];
				to[d] = from[d] + spring[d] * mp.corr;
			}
			// (a correction moves a particle by a fraction of a cell: in open water there is nothing to march against, only the
			// domain walls push back - and a particle of an interior tile that moves less than 7 cells stays inside [1, n - 1):
			// neither the clamp to the box nor the walls' push-out can fire)
			if (!(lean && fabs(to[0] - from[0]) < 7.0 && fabs(to[1] - from[1]) < 7.0 && fabs(to[2] - from[2]) < 7.0)) {
#pragma unroll
				for (int d = 0; d < 3; ++d) to[d] = to[d] < 0.0 ? 0.0 : ((double)nn[d] < to[d] ? (double)nn[d] : to[d]);
				if (mp.collide) {
					if (!open_water || fabs(to[0] - from[0]) >= 7.0 || fabs(to[1] - from[1]) >= 7.0 || fabs(to[2] - from[2]) >= 7.0)
						collide(g, solid, from, to, mp.skin);
					else
						collide_walls_only(g, to, mp.skin);
				}
			}
			int nc[3];
			float nt[3];
#pragma unroll
			for (int d = 0; d < 3; ++d) split_position(to[d], nn[d], nc[d], nt[d]);
			pos_store(out, jj, blocked_index(g, nc[0], nc[1], nc[2]), nt[0], nt[1], nt[2]);
		}
#ifdef CORR_PROFILE
		CORR_STAMP(2);  // thread 0's own particles
		__syncthreads();
		CORR_STAMP(3);  // waiting for the workgroup's slowest thread
#endif
	}
}

}  // namespace
#ifdef CORR_PROFILE
extern "C" int lfa_debug_corr_prof(uint64_t out[8], int reset) {
	unsigned long long h[8] = {0};
	if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_corr_prof), sizeof h) != hipSuccess) return -1;
	for (int i = 0; i < 8; ++i) out[i] = h[i];
	if (reset) {
		unsigned long long z[8] = {0};
		if (hipMemcpyToSymbol(HIP_SYMBOL(g_corr_prof), z, sizeof z) != hipSuccess) return -1;
	}
	return 0;
}
#endif

static MoveParams move_params(const lfa_sim *s, double dt) {
	MoveParams mp;
	const double h = s->prm.cell_size, re = h / sqrt(2.0);
	mp.dt_over_h = dt / h;
	mp.skin = s->prm.boundary_skin_width / h;
	mp.corr = dt * s->prm.correction_stiffness * re / h;
	mp.inv_re2 = h * h / (re * re);
	mp.collide = 1;
	mp.c_home = s->c_home_valid ? s->c_home : nullptr;
	mp.c_home_stride = s->c_home_cap;
	return mp;
}


// ===================================================================================================== fluid sources
namespace {
__global__ void k_mark_coerce(const uint32_t *cell, const uint32_t *src1, size_t n, uint8_t *map) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) map[cell[i]] = (uint8_t)src1[i];
}
/// seed_cell's `for (; num < target; ++num)` (src/simulation.cpp:144): particles an entry has to create, given the count of
/// the last binning and what earlier entries of the same cell have already topped it up to.
__global__ void k_source_need(const uint32_t *cell, const uint32_t *lo, const uint32_t *target, size_t n, const uint32_t *cell_count,
                              const uint32_t *tile_flag, uint32_t *need) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t b = cell[i];
	// first entry of the cell: the binning's count; later entries: the target the previous entry left in the hash (:150)
	const uint32_t have = lo[i] != 0xFFFFFFFFu ? lo[i] : (tile_flag[b >> 9] ? cell_count[b] : 0u);
	need[i] = target[i] > have ? target[i] - have : 0u;
}
/// Slabs, pcg32 draws: the own entries' needs into their slots of the (zeroed) vector over the job-wide entry list, as floats
/// for the all-reduce - a need is at most 4096, so they are exact - and the reduced vector back to integers.
__global__ void k_source_need_scatter(const uint32_t *need, const uint32_t *gidx, size_t n, float *all) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) all[gidx[i]] = (float)need[i];
}
__global__ void k_source_need_gather(const float *all, size_t n, uint32_t *need) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) need[i] = (uint32_t)all[i];
}
__device__ inline uint64_t mix64(uint64_t x) {
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
	x ^= x >> 27; x *= 0x94D049BB133111EBull;
	x ^= x >> 31;
	return x;
}
/// One workgroup-strided thread per seeding entry: position = cell + U[0,1)^3 (seed_cell :141-147), velocity = the source's.
__global__ void k_source_seed(const uint32_t *cell, const uint32_t *src_of, const uint32_t *need, const uint32_t *off, size_t n,
                              const float *src_vel, ParticleSoA p, size_t base, uint64_t seed, uint64_t id_base) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t cnt = need[i], b = cell[i];
	const float *vel = src_vel + 3 * src_of[i];
	for (uint32_t j = 0; j < cnt; ++j) {
		const size_t d = base + off[i] + j;
		float tt[3];
#pragma unroll
		for (int a = 0; a < 3; ++a) {
			// the generator is keyed on the particle's own slot d (unique over every entry of a call, so two entries that top up
			// the same cell never create coincident particles, and no (cell, j) window can alias a neighbouring cell's)
			// (a slab rank keys on the particle's id in the whole job, id_base + its index among this call's new particles)
			const uint64_t r = mix64(seed + ((id_base + (uint64_t)(d - base)) * 3ull + (uint64_t)a + 1ull) * 0x9E3779B97F4A7C15ull + ((uint64_t)b << 40));
			float t = (float)(r >> 40) * (1.0f / 16777216.0f);  // 24 random bits: [0, 1)
			tt[a] = t;
			p.v[a][d] = vel[a];
		}
		pos_store(p.pos, d, b, tt[0], tt[1], tt[2]);
		particle_zero_c_set_id(p, d, (uint32_t)(id_base + (uint64_t)(d - base)));
	}
}
}  // namespace

extern "C" int lfa_clear_sources(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	s->sources.clear();
	s->sources_valid = false;
	return LFA_OK;
}

extern "C" int lfa_add_source(lfa_sim *s, const int32_t *xyz, uint64_t k, const double velocity[3], uint64_t root, int active,
                              int coerce_velocity) {
	if (!s || (!xyz && k) || !velocity) return LFA_E_INVALID;
	if (s->sources.size() >= 254) return lfa_fail(s, LFA_E_UNSUPPORTED, "more than 254 fluid sources");
	if (root > 16) return lfa_fail(s, LFA_E_INVALID, "target_density_cubic_root %llu: more than 4096 particles per cell", (unsigned long long)root);
	for (uint64_t i = 0; i < k; ++i)
		if (!in_grid(s->g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]))
			return lfa_fail(s, LFA_E_INVALID, "source cell (%d, %d, %d) outside the grid", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
	lfa_sim::SourceHost h;
	h.xyz.assign(xyz, xyz + 3 * k);
	for (int d = 0; d < 3; ++d) h.vel[d] = velocity[d];
	h.root = root;
	h.active = active != 0;
	h.coerce = coerce_velocity != 0;
	s->sources.push_back(std::move(h));
	s->sources_valid = false;
	return LFA_OK;
}

/// Flattens the source list for the kernels. Seeding entries keep the reference's sequential semantics: seed_cell ends with
/// `_space_hash(cell).count = target` UNCONDITIONALLY (src/simulation.cpp:150), so the first entry of a cell tops it up from the
/// count of the binning, and every later entry of the same cell from the previous entry's target (a static difference; an
/// entry whose target does not exceed it creates nothing and is dropped). Coercion: the last active coercing source of a cell wins.
int lfa_sources_sync(lfa_sim *s) {
	if (s->sources_valid) return LFA_OK;
	if (s->sources == s->sources_built && (s->sources.empty() || s->src_vel)) {  // the host re-sent the same list
		s->sources_valid = true;
		return LFA_OK;
	}
	LFA_HIP(s, hipSetDevice(s->device));
	// slabs: every rank is handed the whole list (like the solid cells) and seeds the cells of its own tile layers; the coercion
	// map covers the whole grid (a particle's cell is always an owned one)
	const int own_zlo = s->dist ? s->slab_lo * 8 : 0, own_zhi = s->dist ? s->slab_hi * 8 : s->g.nz;
	std::vector<uint32_t> cell, lo, target, of, ccell, csrc;
	// slabs: global index of the own entries; cell, source, global index and mode of the candidates (lfa_sim::SourceSlab)
	std::vector<uint32_t> own_g, k_cell, k_of, k_g, k_mode;
	uint32_t n_global = 0;
	std::vector<float> vel;
	{
		std::vector<std::pair<uint32_t, uint32_t>> seen;  // (cell, target of its latest entry), kept sorted by cell
		std::vector<std::pair<uint32_t, uint32_t>> coerce;  // (cell, source + 1), last one wins
		for (size_t si = 0; si < s->sources.size(); ++si) {
			const auto &h = s->sources[si];
			for (int d = 0; d < 3; ++d) vel.push_back((float)h.vel[d]);
			if (!h.active) continue;
			const uint32_t tgt = (uint32_t)(h.root * h.root * h.root);
			for (size_t i = 0; i + 2 < h.xyz.size(); i += 3) {
				const uint32_t b = blocked_index(s->g, h.xyz[i], h.xyz[i + 1], h.xyz[i + 2]);
				if (h.coerce) coerce.push_back(std::make_pair(b, (uint32_t)si + 1));
				// (the rule runs over every rank's cells: a cell has one owner, so the own entries are the ones a walk over the own
				// cells alone gives, and every rank numbers the entries of the whole job alike)
				const int z = h.xyz[i + 2];
				const bool own = z >= own_zlo && z < own_zhi;
				auto it = std::lower_bound(seen.begin(), seen.end(), std::make_pair(b, 0u),
				                           [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &c) { return a.first < c.first; });
				uint32_t from = 0xFFFFFFFFu;
				if (it != seen.end() && it->first == b) {
					from = it->second;
					it->second = tgt;
					if (tgt <= from) continue;
				} else {
					seen.insert(it, std::make_pair(b, tgt));
				}
				const uint32_t gi = n_global++;
				if (own) {
					cell.push_back(b); lo.push_back(from); target.push_back(tgt); of.push_back((uint32_t)si);
					own_g.push_back(gi);
				}
				if (s->dist && z >= own_zlo - 1 && z <= own_zhi) {
					const int below = z > 0 ? z - 1 : 0, above = z + 1 < s->g.nz ? z + 1 : s->g.nz - 1;
					k_cell.push_back(b); k_of.push_back((uint32_t)si); k_g.push_back(gi);
					k_mode.push_back(own && below >= own_zlo && above < own_zhi ? 0u : 1u);
				}
			}
		}
		std::stable_sort(coerce.begin(), coerce.end(), [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &c) { return a.first < c.first; });
		for (size_t i = 0; i < coerce.size(); ++i)
			if (i + 1 == coerce.size() || coerce[i + 1].first != coerce[i].first) { ccell.push_back(coerce[i].first); csrc.push_back(coerce[i].second); }
	}
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	const size_t n = cell.size(), need = std::max(n, ccell.size());
	if (need > s->src_cap) {
		// the old arrays are dropped first and the handle never keeps a dangling pointer: a failing hipMalloc leaves nulls and a
		// capacity of 0 behind (lfa_destroy frees what is non-null, the next sync allocates again)
		uint32_t **arr[] = {&s->src_cell, &s->src_lo, &s->src_target, &s->src_of, &s->src_need};
		s->src_cap = 0;
		for (uint32_t **q : arr) {
			if (*q) (void)hipFree(*q);
			*q = nullptr;
		}
		const size_t cap = need + need / 2 + 64;
		LFA_HIP(s, hipMalloc(&s->src_cell, cap * 4));
		LFA_HIP(s, hipMalloc(&s->src_lo, cap * 4));
		LFA_HIP(s, hipMalloc(&s->src_target, cap * 4));
		LFA_HIP(s, hipMalloc(&s->src_of, cap * 4));
		LFA_HIP(s, hipMalloc(&s->src_need, 2 * (cap + 1) * 4));  // counts | their exclusive scan
		s->src_cap = cap;
	}
	if (s->src_vel) LFA_HIP(s, hipFree(s->src_vel));
	s->src_vel = nullptr;
	LFA_HIP(s, hipMalloc(&s->src_vel, (vel.size() + 3) * 4));
	if (!vel.empty()) LFA_HIP(s, hipMemcpy(s->src_vel, vel.data(), vel.size() * 4, hipMemcpyHostToDevice));
	// coercion map first (it borrows the entry arrays), then the seeding entries
	const bool had_coerce = s->any_coerce;
	s->any_coerce = !ccell.empty();
	if (s->any_coerce || had_coerce) {
		if (!s->coerce_map) LFA_HIP(s, hipMalloc(&s->coerce_map, s->ncp));
		LFA_HIP(s, hipMemsetAsync(s->coerce_map, 0, s->ncp, s->stream));
		if (s->any_coerce) {
			LFA_HIP(s, hipMemcpyAsync(s->src_cell, ccell.data(), ccell.size() * 4, hipMemcpyHostToDevice, s->stream));
			LFA_HIP(s, hipMemcpyAsync(s->src_of, csrc.data(), csrc.size() * 4, hipMemcpyHostToDevice, s->stream));
			hipLaunchKernelGGL(k_mark_coerce, dim3((unsigned)((ccell.size() + 255) / 256)), dim3(256), 0, s->stream,
			                   (const uint32_t *)s->src_cell, (const uint32_t *)s->src_of, ccell.size(), s->coerce_map);
			LFA_LAUNCH_CHECK(s);
		}
		LFA_HIP(s, hipStreamSynchronize(s->stream));
	}
	if (n) {
		LFA_HIP(s, hipMemcpy(s->src_cell, cell.data(), n * 4, hipMemcpyHostToDevice));
		LFA_HIP(s, hipMemcpy(s->src_lo, lo.data(), n * 4, hipMemcpyHostToDevice));
		LFA_HIP(s, hipMemcpy(s->src_target, target.data(), n * 4, hipMemcpyHostToDevice));
		LFA_HIP(s, hipMemcpy(s->src_of, of.data(), n * 4, hipMemcpyHostToDevice));
	}
	s->n_src_entries = n;
	if (s->src_slab.words) LFA_HIP(s, hipFree(s->src_slab.words));
	s->src_slab = lfa_sim::SourceSlab();
	if (s->dist && n_global) {
		lfa_sim::SourceSlab &q = s->src_slab;
		const size_t nk = k_cell.size(), ng = n_global;
		LFA_HIP(s, hipMalloc(&q.words, (n + 6 * nk + 3 * ng + 2) * 4));
		uint32_t *w = q.words;
		auto take = [&](size_t m) { uint32_t *at = w; w += m; return at; };
		q.own_gidx = take(n); q.cell = take(nk); q.of = take(nk); q.gidx = take(nk); q.mode = take(nk);
		q.need_f = (float *)take(ng); q.need = take(ng); q.first = take(ng + 1); q.keep = take(nk); q.keep_off = take(nk + 1);
		if (n) LFA_HIP(s, hipMemcpy(q.own_gidx, own_g.data(), n * 4, hipMemcpyHostToDevice));
		if (nk) {
			LFA_HIP(s, hipMemcpy(q.cell, k_cell.data(), nk * 4, hipMemcpyHostToDevice));
			LFA_HIP(s, hipMemcpy(q.of, k_of.data(), nk * 4, hipMemcpyHostToDevice));
			LFA_HIP(s, hipMemcpy(q.gidx, k_g.data(), nk * 4, hipMemcpyHostToDevice));
			LFA_HIP(s, hipMemcpy(q.mode, k_mode.data(), nk * 4, hipMemcpyHostToDevice));
		}
		q.n_cand = nk;
		q.n_global = ng;
	}
	s->sources_built = s->sources;
	s->sources_valid = true;
	return LFA_OK;
}

/// The own entries' needs (k_source_need) into src_need.
static int source_needs(lfa_sim *s) {
	const size_t n = s->n_src_entries;
	hipLaunchKernelGGL(k_source_need, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t *)s->src_cell,
	                   (const uint32_t *)s->src_lo, (const uint32_t *)s->src_target, n, (const uint32_t *)s->cell_count,
	                   (const uint32_t *)s->tile_flag, s->src_need);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

/// Room for `count` new records behind the `base` live ones (a deferred binning is completed first: the new particles bring their
/// own v / C), C = 0 in the home array for the ids [id_lo, id_lo + id_n) - the array sized for the ids below id_end -, and, when the
/// caller wants the positions, its buffer checked against `count` and the device's made ready. Nothing of the handle's state moves.
static int source_room(lfa_sim *s, size_t base, size_t count, uint64_t id_lo, size_t id_n, size_t id_end, const double *positions,
                       uint64_t positions_capacity, const char *keeps) {
	if (base + count >= ((size_t)1 << 32)) return lfa_fail(s, LFA_E_INVALID, "more than 2^32 particles");
	if (positions && positions_capacity < count)
		return lfa_fail(s, LFA_E_INVALID, "lfa_update_sources_rng: room for %llu positions but %s%zu particles",
		                (unsigned long long)positions_capacity, keeps, count);
	if (positions) LFA_TRY(lfa_ensure_io(s, count * 24));
	LFA_TRY(lfa_particles_materialize(s));
	LFA_TRY(lfa_particles_reserve(s, base, base + count));  // keeps the live records
	if (s->c_home_valid) {
		LFA_TRY(lfa_c_home_ensure(s, id_end));
		for (int k = 0; k < 9 && id_n; ++k)
			LFA_HIP(s, hipMemsetAsync(s->c_home + (size_t)k * s->c_home_cap + id_lo, 0, id_n * 4, s->stream));
	}
	return LFA_OK;
}

/// The `kept` new records are written behind `base`: counts, flags and the re-binning (the reference re-hashes after seeding,
/// src/simulation.cpp:64). A call that drew from the pcg32 (rng_state) then - and only after a successful re-binning - moves the
/// state on by the draws of the whole job's total_all particles and records lfa_source_last.
static int source_finish(lfa_sim *s, size_t base, size_t kept, uint64_t total_all, uint64_t id_base, uint64_t *n_seeded,
                         uint64_t *rng_state, const double *positions) {
	s->np_live = base + kept;
	s->np = s->np_live;
	s->vmax2_valid = false;  // the new particles carry their source's velocity
	if (n_seeded) *n_seeded = kept;
	const int rc = lfa_hash_particles(s);
	if (rc >= 0 && rng_state) {
		if (positions) LFA_HIP(s, hipStreamSynchronize(s->stream));
		*rng_state = lfa_pcg32_advance(*rng_state, 6ull * total_all);
		s->source_last[0] = total_all;
		s->source_last[1] = kept;
		s->source_last[2] = id_base;
	}
	return rc;
}

/// lfa_update_sources_rng with LFA_SEED_COLLECTIVE on a slab decomposition (the checks of update_sources are done, the entry lists
/// are current). ONE transport call - the all-reduce of the needs over the job-wide entry list -, none when no source lists an
/// active entry; the re-binning that ends the call has its own.
static int update_sources_collective(lfa_sim *s, uint64_t *n_seeded, uint64_t *rng_state, int flags, double *positions,
                                     uint64_t positions_capacity) {
	const lfa_sim::SourceSlab &q = s->src_slab;
	const size_t n = s->n_src_entries, ng = q.n_global;
	const uint64_t id_base = s->next_global_id, state = *rng_state;
	const int ltr = (flags & LFA_SEED_DRAW_LTR) ? 1 : 0;
	if (!ng) return LFA_OK;  // no entry anywhere: nothing to create, no draw, no message
	LFA_HIP(s, hipMemsetAsync(q.need_f, 0, ng * 4, s->stream));
	if (n) {
		LFA_TRY(source_needs(s));
		hipLaunchKernelGGL(k_source_need_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
		                   (const uint32_t *)s->src_need, (const uint32_t *)q.own_gidx, n, q.need_f);
		LFA_LAUNCH_CHECK(s);
	}
	LFA_TRY(s->dist->allreduce_buf(s, q.need_f, ng, LFA_RED_F32, false));
	hipLaunchKernelGGL(k_source_need_gather, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s->stream, (const float *)q.need_f, ng,
	                   q.need);
	LFA_LAUNCH_CHECK(s);
	size_t total_all = 0;
	LFA_TRY(lfa_scan_total(s, q.need, q.first, ng, q.first + ng, LFA_PIN_SOURCE_TOTAL_ALL, &total_all));
	// ---- what the job-wide count decides: every rank decides alike
	if (!total_all) return LFA_OK;  // every source cell of the job is full: no draw, the binning stands
	if (id_base + total_all >= ((uint64_t)1 << 32)) return lfa_fail(s, LFA_E_INVALID, "more than 2^32 particles");
	// ---- from here a failure is this rank's alone: its peers must not wait for it in the re-binning
	size_t kept = 0;
	const size_t base = s->np_live;
	auto seed = [&]() -> int {
		LFA_TRY(lfa_source_count(s, total_all, state, ltr, &kept));
		// (C = 0 for every new id of the job: the ids a rank keeps are no contiguous range)
		LFA_TRY(source_room(s, base, kept, id_base, total_all, (size_t)(id_base + total_all), positions, positions_capacity, "this rank keeps "));
		LFA_TRY(lfa_source_write(s, base, kept, total_all, id_base, state, ltr, positions ? (double *)s->io_buf : (double *)nullptr));
		if (positions && kept) LFA_HIP(s, hipMemcpyAsync(positions, s->io_buf, kept * 24, hipMemcpyDeviceToHost, s->stream));
		return LFA_OK;
	};
	const int rc_seed = seed();
	if (rc_seed < 0) {
		s->dist->give_up();
		return rc_seed;
	}
	s->next_global_id = id_base + total_all;
	return source_finish(s, base, kept, total_all, id_base, n_seeded, rng_state, positions);
}

/// lfa_update_sources. rng_state == nullptr: positions from the counter-based generator (k_source_seed); else the reference's
/// draws from the pcg32 in *rng_state (seed.hip: k_source_write; slabs: update_sources_collective), advanced on success.
static int update_sources(lfa_sim *s, uint64_t *n_seeded, uint64_t *rng_state, int flags, double *positions, uint64_t positions_capacity) {
	if (n_seeded) *n_seeded = 0;
	if (rng_state) {
		if (flags & ~(LFA_SEED_DRAW_LTR | LFA_SEED_COLLECTIVE))
			return lfa_fail(s, LFA_E_INVALID, "lfa_update_sources_rng: flags LFA_SEED_DRAW_LTR, LFA_SEED_COLLECTIVE or none");
		if (s->dist && !(flags & LFA_SEED_COLLECTIVE))
			return lfa_fail(s, LFA_E_UNSUPPORTED, "fluid sources that draw from the pcg32 on a slab decomposition: pass LFA_SEED_COLLECTIVE, "
			                                      "and make the same call with the same generator state on every rank");
		if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size before seeding");
	}
	if (!s->binned) return lfa_fail(s, LFA_E_INVALID, "lfa_update_sources: call lfa_hash_particles first");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	LFA_TRY(lfa_sources_sync(s));
	if (rng_state && s->dist) return update_sources_collective(s, n_seeded, rng_state, flags, positions, positions_capacity);
	const size_t n = s->n_src_entries;
	if (!n && !s->dist) return LFA_OK;
	size_t total = 0;
	uint32_t *off = s->src_need ? s->src_need + s->src_cap + 1 : nullptr;
	if (n) {
		LFA_TRY(source_needs(s));
		// exclusive scan into the second half of the scratch; the total is read back (the host has to size the particle arrays)
		LFA_TRY(lfa_scan_total(s, s->src_need, off, n, off + n, LFA_PIN_SOURCE_TOTAL, &total));
	}
	// slabs: what every rank creates, gathered (one sum all-reduce of a vector with one slot per rank) - the ids of the new
	// particles continue the job-wide numbering in rank order, and either every rank re-bins or none does
	uint64_t id_base = s->np_live, total_all = total;
	if (s->dist) {
		const int nr = s->dist->nranks, me = s->dist->rank;
		double hv[LFA_DR_MAX_RANKS] = {0};
		hv[me] = (double)total;
		double *dv = s->dist_red + LFA_DR_SOURCE_TOTALS;
		LFA_HIP(s, hipMemcpyAsync(dv, hv, (size_t)nr * 8, hipMemcpyHostToDevice, s->stream));
		LFA_TRY(s->dist->allreduce_buf(s, dv, (size_t)nr, LFA_RED_F64, false));
		LFA_HIP(s, hipMemcpyAsync(hv, dv, (size_t)nr * 8, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipStreamSynchronize(s->stream));
		id_base = s->next_global_id;
		total_all = 0;
		for (int r = 0; r < nr; ++r) {
			if (r < me) id_base += (uint64_t)hv[r];
			total_all += (uint64_t)hv[r];
		}
		if (s->next_global_id + total_all >= ((uint64_t)1 << 32)) return lfa_fail(s, LFA_E_INVALID, "more than 2^32 particles");
		s->next_global_id += total_all;
	}
	if (!total_all) return LFA_OK;  // every source cell is full: the binning stands
	const size_t base = s->np_live;
	// the new particles get the ids id_base .. id_base + total - 1 (single domain: = base)
	LFA_TRY(source_room(s, base, total, id_base, total, s->dist ? (size_t)s->next_global_id : base + total, positions, positions_capacity, ""));
	if (rng_state) {
		LFA_TRY(lfa_source_write(s, base, total, total, id_base, *rng_state, (flags & LFA_SEED_DRAW_LTR) ? 1 : 0,
		                         positions ? (double *)s->io_buf : (double *)nullptr));
		if (positions) LFA_HIP(s, hipMemcpyAsync(positions, s->io_buf, total * 24, hipMemcpyDeviceToHost, s->stream));
	} else {
		++s->source_epoch;
		if (total) {
			hipLaunchKernelGGL(k_source_seed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t *)s->src_cell,
			                   (const uint32_t *)s->src_of, (const uint32_t *)s->src_need, (const uint32_t *)off, n, (const float *)s->src_vel,
			                   s->pb[s->cur], base, 0x5EED50ull + s->source_epoch * 0x632BE59BD9B4E019ull, id_base);
			LFA_LAUNCH_CHECK(s);
		}
	}
	return source_finish(s, base, total, total_all, id_base, n_seeded, rng_state, positions);
}

extern "C" int lfa_update_sources(lfa_sim *s, uint64_t *n_seeded) {
	if (!s) return LFA_E_INVALID;
	if (s->src_rng_on) return update_sources(s, n_seeded, &s->src_rng_state, s->src_rng_flags, nullptr, 0);
	return update_sources(s, n_seeded, nullptr, 0, nullptr, 0);
}

extern "C" int lfa_update_sources_rng(lfa_sim *s, uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions,
                                      uint64_t positions_capacity) {
	if (!s) return LFA_E_INVALID;
	if (!rng_state) return lfa_fail(s, LFA_E_INVALID, "lfa_update_sources_rng: rng_state is NULL");
	return update_sources(s, n_seeded, rng_state, flags, positions, positions_capacity);
}

extern "C" int lfa_set_source_rng(lfa_sim *s, int on, uint64_t rng_state, int flags) {
	if (!s) return LFA_E_INVALID;
	if (on && (flags & ~(LFA_SEED_DRAW_LTR | LFA_SEED_COLLECTIVE)))
		return lfa_fail(s, LFA_E_INVALID, "lfa_set_source_rng: flags LFA_SEED_DRAW_LTR, LFA_SEED_COLLECTIVE or none");
	if (on && s->dist && !(flags & LFA_SEED_COLLECTIVE))
		return lfa_fail(s, LFA_E_UNSUPPORTED, "fluid sources that draw from the pcg32 on a slab decomposition: pass LFA_SEED_COLLECTIVE "
		                                      "(every rank then switches the mode on with the same state)");
	s->src_rng_on = on != 0;
	s->src_rng_state = on ? rng_state : 0;
	s->src_rng_flags = on ? flags : 0;
	return LFA_OK;
}

extern "C" int lfa_source_last(const lfa_sim *s, uint64_t out[3]) {
	if (!s || !out) return LFA_E_INVALID;
	for (int k = 0; k < 3; ++k) out[k] = s->source_last[k];
	return LFA_OK;
}

extern "C" int lfa_get_source_rng(const lfa_sim *s, int *on, uint64_t *rng_state) {
	if (!s) return LFA_E_INVALID;
	if (on) *on = s->src_rng_on ? 1 : 0;
	if (rng_state) *rng_state = s->src_rng_state;
	return LFA_OK;
}

/// Which tiles are nowhere near a solid cell / a domain wall (k_tile_clear): recomputed when the solid mask has changed.
static int refresh_tile_clear(lfa_sim *s) {
	if (s->clear_epoch == s->solid_epoch && s->tile_clear) return LFA_OK;
	if (!s->tile_clear) LFA_HIP(s, hipMalloc(&s->tile_clear, (size_t)s->g.nt * 2));
	uint8_t *tile_solid = s->tile_clear + s->g.nt;
	hipLaunchKernelGGL(k_tile_has_solid, dim3(s->g.nt < 16384 ? s->g.nt : 16384), dim3(256), 0, s->stream, (const uint8_t *)s->solid,
	                   s->g.nt, tile_solid);
	hipLaunchKernelGGL(k_tile_clear, dim3((s->g.nt + 255) / 256), dim3(256), 0, s->stream, s->g, (const uint8_t *)tile_solid,
	                   s->tile_clear);
	LFA_LAUNCH_CHECK(s);
	s->clear_epoch = s->solid_epoch;
	return LFA_OK;
}

/// `with_count`: lfa_time_step's variant - the binning that follows finds tile_count / rank done (lfa_sim::counts_fresh).
/// `split`: _advect_particles alone - the positions of before are kept (save_old_positions) for the lfa_collide that follows.
static int save_old_positions(lfa_sim *s, size_t n);
static int advect_collide(lfa_sim *s, double dt, bool with_count, bool split = false) {
	if (!s) return LFA_E_INVALID;
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	LFA_TRY(lfa_particles_materialize(s));  // reads v
	const size_t n = s->binned ? s->np_live : s->np;
	MoveParams mp = move_params(s, dt);
	s->move_pending = false;
	if (split) {  // (slabs: the particles migrate once they have their final positions, in lfa_collide)
		LFA_TRY(save_old_positions(s, n));
		mp.collide = 0;
	}
	LFA_TRY(lfa_sources_sync(s));
	LFA_TRY(refresh_tile_clear(s));
	s->counts_fresh = false;
	if (n) {
		if (s->any_coerce) s->vmax2_valid = false;  // velocities are overwritten inside the coercing sources' cells
		const uint8_t *cm = s->any_coerce ? (const uint8_t *)s->coerce_map : (const uint8_t *)nullptr;
		const float *sv = s->any_coerce ? (const float *)s->src_vel : (const float *)nullptr;
		if (with_count && !s->dist) {
			LFA_HIP(s, hipMemsetAsync(s->tile_count, 0, (size_t)(s->g.nt + 1) * 4, s->stream));
			const dim3 grid((unsigned)((n + 256 * AC_CHUNKS - 1) / (256 * AC_CHUNKS)));
			if (s->any_coerce)
				hipLaunchKernelGGL(k_advect_collide_count<true>, grid, dim3(256), 0, s->stream, n, s->pb[s->cur], s->g, s->solid,
				                   mp, cm, sv, (const uint8_t *)s->tile_clear, s->tile_count, s->rank);
			else
				hipLaunchKernelGGL(k_advect_collide_count<false>, grid, dim3(256), 0, s->stream, n, s->pb[s->cur], s->g, s->solid,
				                   mp, cm, sv, (const uint8_t *)s->tile_clear, s->tile_count, s->rank);
			s->counts_fresh = true;
		} else {
			const dim3 grid((unsigned)((n + 255) / 256));
			if (s->any_coerce)
				hipLaunchKernelGGL(k_advect_collide<true>, grid, dim3(256), 0, s->stream, n, s->pb[s->cur], s->g, s->solid, mp,
				                   cm, sv, (const uint8_t *)s->tile_clear);
			else
				hipLaunchKernelGGL(k_advect_collide<false>, grid, dim3(256), 0, s->stream, n, s->pb[s->cur], s->g, s->solid, mp,
				                   cm, sv, (const uint8_t *)s->tile_clear);
		}
		LFA_LAUNCH_CHECK(s);
	}
	if (!split) LFA_TRY(lfa_dist_migrate(s));
	s->unknown_count_valid = false;
	s->move_pending = split;
	return LFA_OK;
}
extern "C" int lfa_advect_collide(lfa_sim *s, double dt) { return advect_collide(s, dt, false); }
extern "C" int lfa_advect(lfa_sim *s, double dt) { return advect_collide(s, dt, false, true); }

namespace {
/// _detect_collisions as its own pass (lfa_collide): from = the position saved before the move, to = the current one.
__global__ void __launch_bounds__(256)
k_collide_only(size_t n, ParticleSoA p, const PosRec *old, GridDims g,
               const uint8_t *solid, double skin) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const PosRec me = pos_load(p.pos, i);
	const uint32_t key = me.key;
	if (key == 0xFFFFFFFFu) return;
	const PosRec was = old ? pos_load(old, i) : me;
	const int nn[3] = {g.nx, g.ny, g.nz};
	int c[3], oc[3];
	cell_of_key(g, key, c);
	double from[3], to[3];
	cell_of_key(g, was.key, oc);
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		to[d] = (double)c[d] + (double)me.t[d];
		from[d] = (double)oc[d] + (double)was.t[d];
	}
	collide(g, solid, from, to, skin);
	int nc[3];
	float nt[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) split_position(to[d], nn[d], nc[d], nt[d]);
	pos_store(p.pos, i, blocked_index(g, nc[0], nc[1], nc[2]), nt[0], nt[1], nt[2]);
}
}  // namespace

/// The position records of before a split move go to the other buffer's pos array (free between a binning and the G2P, and
/// after the materialisation at the start of a step), where lfa_collide and a download in between (old_position) find them.
static int save_old_positions(lfa_sim *s, size_t n) {
	if (!n) return LFA_OK;
	ParticleSoA &cur = s->pb[s->cur], &oth = s->pb[s->cur ^ 1];
	LFA_HIP(s, hipMemcpyAsync(oth.pos, cur.pos, n * sizeof(PosRec), hipMemcpyDeviceToDevice, s->stream));
	return LFA_OK;
}

extern "C" int lfa_collide(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	const size_t n = s->binned ? s->np_live : s->np;
	const bool pending = s->move_pending;
	s->move_pending = false;
	if (!n) return lfa_dist_migrate(s);  // (slabs: every rank takes part in the hand-over, also one without particles)
	LFA_TRY(refresh_tile_clear(s));
	ParticleSoA &cur = s->pb[s->cur], &oth = s->pb[s->cur ^ 1];
	// nothing pending (an upload in between has replaced the particles): from = to, i.e. the skin push-out alone
	hipLaunchKernelGGL(k_collide_only, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, n, cur,
	                   pending ? (const PosRec *)oth.pos : (const PosRec *)nullptr, s->g,
	                   (const uint8_t *)s->solid, move_params(s, 0.0).skin);
	LFA_LAUNCH_CHECK(s);
	s->unknown_count_valid = false;
	// slabs: the move that lfa_advect / lfa_correct left pending is complete now - particles that crossed a slab face change rank
	return lfa_dist_migrate(s);
}

/// The correction's scratch for the cell-ordered positions: four consecutive v / c arrays that are free between the binning and
/// the G2P - the other buffer's v.. ; with a deferred binning, where the other buffer still holds the v (and for APIC the C)
/// that the P2G / G2P read: this buffer's own v.. (APIC: the G2P is yet to fill them) or the other buffer's c[0..3] (PIC /
/// FLIP: its C has moved here already)
static float4 *correction_scratch(lfa_sim *s) {
	ParticleSoA &cur = s->pb[s->cur], &oth = s->pb[s->cur ^ 1];
	return (float4 *)(!s->vc_pending ? oth.v[0] : (s->vc_with_c ? cur.v[0] : oth.c[0]));
}

/// First half of lfa_correct_collide: per-cell particle lists + cell-ordered positions (reads the (key, t) of the current binning).
static int correct_build_index(lfa_sim *s, bool exchange = true) {
	const size_t n = s->np_live;
	if (!n && !s->dist) return LFA_OK;
	if (!s->fine_start) {
		const size_t bytes = (size_t)s->g.nt * FT_STRIDE * 4;
		hipError_t e = hipMalloc(&s->fine_start, bytes);
		if (e != hipSuccess) return lfa_fail(s, LFA_E_OOM, "hipMalloc of the fine-cell index (%zu bytes) failed", bytes);
	}
	// neighbours within one cell across the slab faces: ghost copies of the adjacent tile layers' particles
	if (s->dist && exchange) LFA_TRY(lfa_dist_exchange_ghost_particles(s));
	LFA_TRY(refresh_tile_clear(s));
	const int n_index = s->dist ? s->n_ptiles_all : s->n_ptiles;
	const int grid = n_index < 16384 ? (n_index > 0 ? n_index : 1) : 16384;
	ParticleSoA &cur = s->pb[s->cur];
	if (n) LFA_TRY(lfa_ev_record(s, LFA_EV_CORR_BEGIN));
	hipLaunchKernelGGL(k_build_fine_index, dim3(grid), dim3(FIDX_THREADS), 0, s->stream, s->dist ? s->ptiles_all : s->ptiles, n_index,
	                   (const PosRec *)cur.pos, s->tile_start, s->tile_count, s->fine_start, correction_scratch(s), s->bkey);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

/// Second half: the pairwise correction + collision; writes (key, t) in place.
static int correct_apply(lfa_sim *s, double dt, bool migrate = true, bool with_collide = true) {
	const size_t n = s->np_live;
	MoveParams mpc = move_params(s, dt);
	mpc.collide = with_collide ? 1 : 0;
	ParticleSoA &cur = s->pb[s->cur];
	float4 *spos = correction_scratch(s);
	if (n) {
		// LDS-tiled pass; half tiles whose neighbourhood exceeds the LDS capacity are flagged and redone, first by the same kernel
		// with the whole LDS of a CU (round 4: late in a run a few hundred crowded half tiles cost the global-gather kernel more
		// than the other 31 000 cost the tiled one), then - what exceeds even that - by the global-gather kernel
		const size_t ovf_words = ((size_t)CORR_PARTS * s->n_ptiles + 31) / 32 + 2;  // word 0: how many are flagged
		const size_t ovf_stride = ((size_t)CORR_PARTS * s->g.nt + 31) / 32 + 2;     // second bitmap: what the big pass has flagged
		if (!s->corr_ovf) {  // 2 x 2 bits per tile of the grid; its own array: the pressure solve may be running beside this
			hipError_t e = hipMalloc(&s->corr_ovf, 2 * ovf_stride * 4);
			if (e != hipSuccess) return lfa_fail(s, LFA_E_OOM, "hipMalloc of the correction's overflow bitmaps failed");
		}
		uint32_t *ovf = s->corr_ovf, *ovf2 = s->corr_ovf + ovf_stride;
		s->corr_parts_tiles = s->n_ptiles;
		LFA_HIP(s, hipMemsetAsync(ovf, 0, ovf_words * 4, s->stream));
		LFA_HIP(s, hipMemsetAsync(ovf2, 0, ovf_words * 4, s->stream));
		{
			const int work = CORR_PARTS * s->n_ptiles, g2 = work < 65536 ? (work > 0 ? work : 1) : 65536;
			// every neighbour position comes from the records of the index built above (the OLD positions), so the new ones are
			// written in place; the fallback pass below takes its particles' old state from the records and the copy of the keys
			// the index kernel has left in bkey
			LFA_TRY(lfa_ev_record(s, LFA_EV_CORR_INDEXED));
			hipLaunchKernelGGL((k_correct_fine<FINE_CAP, false>), dim3(g2), dim3(CORR_THREADS), 0, s->stream, s->ptiles, s->n_ptiles, cur.pos,
			                   s->g, s->solid, s->tile_count, s->fine_start, (const float4 *)spos, mpc, ovf,
			                   (const uint8_t *)s->tile_clear, (const uint32_t *)nullptr);
			LFA_LAUNCH_CHECK(s);
			LFA_TRY(lfa_ev_record(s, LFA_EV_CORR_TILED));
			// (a workgroup per CU and a few more: they return at once unless something is flagged)
			hipLaunchKernelGGL((k_correct_fine<FINE_CAP_BIG, true>), dim3(std::min(CORR_BIG_SLICES * g2, 2048)), dim3(CORR_THREADS_BIG), 0, s->stream, s->ptiles,
			                   s->n_ptiles, cur.pos, s->g, s->solid, s->tile_count, s->fine_start,
			                   (const float4 *)spos, mpc, ovf2, (const uint8_t *)s->tile_clear, (const uint32_t *)ovf);
			LFA_LAUNCH_CHECK(s);
		}
		const uint32_t *fallback = ovf2;
		hipLaunchKernelGGL(k_correct_collide, dim3((unsigned)std::min<size_t>((n + 255) / 256, 16384)), dim3(256), 0, s->stream, n, cur, cur.pos,
		                   s->g, s->solid, s->tile_count, s->fine_start, (const float4 *)spos, mpc,
		                   fallback, (const int *)s->tile_pslot, s->p_off, (const uint32_t *)s->bkey);
		LFA_LAUNCH_CHECK(s);
	}
	if (migrate) LFA_TRY(lfa_dist_migrate(s));
	s->unknown_count_valid = false;
	return LFA_OK;
}

extern "C" int lfa_correct_collide(lfa_sim *s, double dt) {
	if (!s) return LFA_E_INVALID;
	if (!s->binned) return lfa_fail(s, LFA_E_INVALID, "lfa_correct_collide: call lfa_hash_particles first");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	if (!s->np_live && !s->dist) return LFA_OK;
	LFA_TRY(correct_build_index(s));
	return correct_apply(s, dt);
}

/// _correct_positions alone (src/simulation.cpp:562-610): the collision handling that follows it in time_step (:115) is left to
/// lfa_collide, so that a host's post_correction_callback sits exactly where the reference has it (:111-117).
extern "C" int lfa_correct(lfa_sim *s, double dt) {
	if (!s) return LFA_E_INVALID;
	if (!s->binned) return lfa_fail(s, LFA_E_INVALID, "lfa_correct: call lfa_hash_particles first");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	s->move_pending = false;
	if (!s->np_live && !s->dist) return LFA_OK;
	LFA_TRY(correct_build_index(s));  // (slabs: with the ghost exchange - every rank takes part)
	// the positions of before: the records go to the other buffer, whole
	LFA_TRY(save_old_positions(s, s->np_live));
	LFA_TRY(correct_apply(s, dt, false, false));  // (no migration yet: lfa_collide hands the particles over)
	s->move_pending = true;
	return LFA_OK;
}

int lfa_corr_join(lfa_sim *s) {
	if (!s->corr_in_flight) return LFA_OK;
	s->corr_in_flight = false;
	LFA_HIP(s, hipStreamWaitEvent(s->stream, s->ev_cjoin, 0));
	return LFA_OK;
}

/// `slab_exchanged`: lfa_time_step on a slab decomposition has already exchanged the ghost particles on the main stream and
/// migrates after the join - no communication happens on the correction's stream.
static int correct_begin(lfa_sim *s, double dt, bool slab_exchanged) {
	if (!s) return LFA_E_INVALID;
	if (!s->binned) return lfa_fail(s, LFA_E_INVALID, "lfa_correct_collide_begin: call lfa_hash_particles first");
	if (s->dist && !slab_exchanged)
		return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_correct_collide_begin: slab decompositions exchange particles inside the correction (use lfa_correct_collide or lfa_time_step)");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	s->corr_begun = false;
	if (!s->np_live && !s->dist) return LFA_OK;  // nothing to correct: _end and _undo are no-ops
	LFA_HIP(s, hipEventRecord(s->ev_cfork, s->stream));
	LFA_HIP(s, hipStreamWaitEvent(s->stream3, s->ev_cfork, 0));
	hipStream_t main_stream = s->stream;
	s->stream = s->stream3;
	int rc = correct_build_index(s, false);
	if (rc == LFA_OK) rc = correct_apply(s, dt, false);
	s->stream = main_stream;
	const hipError_t e1 = s->timing ? hipEventRecord(s->ev[LFA_EV_STEP_CORRECT], s->stream3) : hipSuccess;
	// the join event is recorded whatever happened: the main stream waits for it before it touches particles again
	const hipError_t e2 = hipEventRecord(s->ev_cjoin, s->stream3);
	s->corr_in_flight = true;
	s->corr_begun = true;
	s->corr_undo_valid = rc == LFA_OK && !s->dist;
	if (rc < 0) return rc;
	LFA_HIP(s, e1);
	LFA_HIP(s, e2);
	return LFA_OK;
}
extern "C" int lfa_correct_collide_begin(lfa_sim *s, double dt) { return correct_begin(s, dt, false); }

extern "C" int lfa_correct_collide_end(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	LFA_HIP(s, hipSetDevice(s->device));
	return lfa_corr_join(s);
}

namespace {
/// (key, t) of before the correction: the keys from their copy, the fractions from the cell-ordered records (record k
/// belongs to particle spos[k].w) - both are inputs the correction does not write.
__global__ void __launch_bounds__(256)
k_correct_undo(size_t n, const float4 *spos, const uint32_t *old_key, PosRec *pos) {
	const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	const float4 rec = spos[k];
	const uint32_t i = __float_as_uint(rec.w);
	// (the records of the fine index keep cell bits in the two top bits of the fractions: fine_record)
	pos[i].t[0] = __uint_as_float(__float_as_uint(rec.x) & 0x3FFFFFFFu);
	pos[i].t[1] = __uint_as_float(__float_as_uint(rec.y) & 0x3FFFFFFFu);
	pos[i].t[2] = __uint_as_float(__float_as_uint(rec.z) & 0x3FFFFFFFu);
	pos[k].key = old_key[k];
}
}  // namespace

extern "C" int lfa_correct_collide_undo(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	// What decides is whether the correction's inputs are still there (corr_undo_valid), not whether it is still running: entry
	// points that only read (lfa_cfl, lfa_upload_cells of a grid-editing callback, lfa_get_correction_stats, the mesher) join it
	// without invalidating anything, and a begin that found no particles started nothing.
	if (!s->corr_begun) return LFA_OK;
	if (!s->corr_undo_valid)
		return lfa_fail(s, LFA_E_INVALID, "lfa_correct_collide_undo: positions, binning or solid cells have changed since lfa_correct_collide_begin");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));  // joins if still in flight; the restore below is the change that invalidates a second undo
	s->corr_begun = false;
	const size_t n = s->np_live;
	if (!n) return LFA_OK;
	ParticleSoA &cur = s->pb[s->cur];
	hipLaunchKernelGGL(k_correct_undo, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, n, (const float4 *)correction_scratch(s),
	                   (const uint32_t *)s->bkey, cur.pos);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

/// Device-resident simulation::time_step(dt) (src/simulation.cpp:43-125) without fluid sources and host callbacks:
/// advect+collide, hash, P2G, gravity, pressure solve, pressure gradient, correct+collide, extrapolate, hash, G2P.
int lfa_g2p_stale(lfa_sim *s);  // grid_ops.hip
extern "C" int lfa_time_step(lfa_sim *s, double dt, double *residual, uint64_t *iterations) {
	if (!s) return LFA_E_INVALID;
	if (s->src_rng_on && s->dist && !(s->src_rng_flags & LFA_SEED_COLLECTIVE))  // (before anything moves: lfa_update_sources would refuse in the middle of the step)
		return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_time_step: fluid sources that draw from the pcg32 (lfa_set_source_rng) on a slab decomposition");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_commit(s));
	LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_START));
	LFA_TRY(advect_collide(s, dt, true));
	LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_ADVECT));
	{
		const bool counted = s->counts_fresh;
		s->counts_fresh = false;
		LFA_TRY(lfa_hash_particles_impl(s, counted));
	}
	if (!s->sources.empty()) LFA_TRY(lfa_update_sources(s, nullptr));  // _update_sources + hash_particles (:63-64)
	LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_BIN));
	// The correction reads and writes particle positions only, the pressure solve / gradient / extrapolation grid arrays only:
	// the two run side by side (the solve is a chain of short launch- and HBM-bound kernels, the correction one long VALU-bound
	// one); the correction's stream has the lower priority. (Starting its cell index already beside the P2G - it only reads the
	// binned (key, t) - changed nothing at C4.) Slabs exchange ghost particles and migrate around the correction, on the main
	// stream: they do the exchange before the fork and the migration after the join (the decision must be the same on every
	// rank - a rank without particles included -, or the ranks would issue their collectives in different orders).
	const bool overlap = s->overlap_correction && (s->dist || s->np_live);
	LFA_TRY(lfa_p2g_run(s, true, dt));
	LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_P2G));
	if (overlap) {
		if (s->dist) LFA_TRY(lfa_dist_exchange_ghost_particles(s));
		LFA_TRY(correct_begin(s, dt, true));
	}
	double res = 0.0;
	uint64_t it = 0;
	int rc = LFA_OK;
	auto grid_stages = [&]() -> int {
		rc = lfa_pcg_solve(s, dt, &res, &it);
		if (rc < 0) return rc;
		LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_SOLVE));
		LFA_TRY(lfa_apply_pressure(s, dt));
		LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_APPLY));
		if (!overlap) {
			LFA_TRY(lfa_correct_collide(s, dt));
			LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_CORRECT));
		}
		LFA_TRY(lfa_extrapolate(s));  // the valid set is the one of the P2G-time hash, like the reference (:119)
		return lfa_ev_record(s, LFA_EV_STEP_EXTRAP);
	};
	const int rc_grid = grid_stages();
	// joined whatever happened in between: nothing that follows on the main stream may race with the correction
	if (overlap) LFA_TRY(lfa_corr_join(s));
	if (rc_grid < 0) return rc_grid;
	if (overlap && s->dist) LFA_TRY(lfa_dist_migrate(s, true));
	LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_JOIN));
	// The G2P gathers per tile. The particles keep the order of the P2G-time binning and the few whose corrected position left
	// their tile take the global-gather path (lfa_g2p_stale); like after lfa_advect_collide the order is stale afterwards and
	// the next step re-bins. Slabs: the same - particles that went to a neighbour rank carry an invalid key (skipped), the ones
	// that arrived sit behind the binned ones and join the leaver list. (Round 2 re-binned here: +18 % on a one-rank slab run.)
	LFA_TRY(lfa_g2p_stale(s));
	if (s->timing) {
		LFA_TRY(lfa_ev_record(s, LFA_EV_STEP_G2P));
		LFA_HIP(s, hipEventSynchronize(s->ev[LFA_EV_STEP_G2P]));
		double *m = s->ms_next;
		static const lfa_span spans[] = {
			{LFA_STEP_TIMER_ADVECT_COLLIDE, LFA_EV_STEP_START, LFA_EV_STEP_ADVECT},
			{LFA_STEP_TIMER_BIN, LFA_EV_STEP_ADVECT, LFA_EV_STEP_BIN},
			{LFA_STEP_TIMER_P2G, LFA_EV_STEP_BIN, LFA_EV_STEP_P2G},
			{LFA_STEP_TIMER_P2G_SCATTER_KERNEL, LFA_EV_SCATTER_BEGIN, LFA_EV_SCATTER_END},
			{LFA_STEP_TIMER_BUILD_SYSTEM, LFA_EV_STEP_P2G, LFA_EV_STEP_SOLVE},
			{LFA_STEP_TIMER_APPLY_PRESSURE, LFA_EV_STEP_SOLVE, LFA_EV_STEP_APPLY},
			{LFA_STEP_TIMER_G2P, LFA_EV_STEP_JOIN, LFA_EV_STEP_G2P},
			{LFA_STEP_TIMER_TIME_STEP, LFA_EV_STEP_START, LFA_EV_STEP_G2P},
		};
		LFA_TRY(lfa_fill_spans(s, spans, m));
		m[LFA_STEP_TIMER_PCG_LOOP] = 0.0;
		if (it || s->n_ptiles) {  // a solve ran: the split is at the end of the system build, recorded inside it
			static const lfa_span split[] = {{LFA_STEP_TIMER_BUILD_SYSTEM, LFA_EV_STEP_P2G, LFA_EV_SYSTEM_BUILT},
			                                 {LFA_STEP_TIMER_PCG_LOOP, LFA_EV_SYSTEM_BUILT, LFA_EV_STEP_SOLVE}};
			LFA_TRY(lfa_fill_spans(s, split, m));
		}
		m[LFA_STEP_TIMER_CORRECT_CELL_INDEX] = m[LFA_STEP_TIMER_CORRECT_TILED_KERNEL] = m[LFA_STEP_TIMER_CORRECT_COLLIDE] = 0.0;
		if (s->np_live) {
			static const lfa_span corr[] = {{LFA_STEP_TIMER_CORRECT_CELL_INDEX, LFA_EV_CORR_BEGIN, LFA_EV_CORR_INDEXED},
			                                {LFA_STEP_TIMER_CORRECT_TILED_KERNEL, LFA_EV_CORR_INDEXED, LFA_EV_CORR_TILED}};
			LFA_TRY(lfa_fill_spans(s, corr, m));
		}
		// overlapped: the correction's own span on its stream (its kernels share the device with the solve's), and the
		// extrapolation follows the pressure gradient; back to back: the correction sits between the two
		if (!overlap || s->np_live) {
			const lfa_span whole[] = {{LFA_STEP_TIMER_CORRECT_COLLIDE, overlap ? LFA_EV_CORR_BEGIN : LFA_EV_STEP_APPLY, LFA_EV_STEP_CORRECT}};
			LFA_TRY(lfa_fill_spans(s, whole, m));
		}
		const lfa_span extrap[] = {{LFA_STEP_TIMER_EXTRAPOLATE, overlap ? LFA_EV_STEP_APPLY : LFA_EV_STEP_CORRECT, LFA_EV_STEP_EXTRAP}};
		LFA_TRY(lfa_fill_spans(s, extrap, m));
		m[LFA_STEP_TIMER_PCG_ITERATIONS] = (double)it;
		m[LFA_STEP_TIMER_PCG_ITERATION_MEAN] = it ? m[LFA_STEP_TIMER_PCG_LOOP] / (double)it : 0.0;
		m[LFA_STEP_TIMER_OVERLAPPED] = overlap ? 1.0 : 0.0;
	}
	if (residual) *residual = res;
	if (iterations) *iterations = it;
	return rc;
}

extern "C" int lfa_get_correction_stats(lfa_sim *s, uint64_t stats[2]) {
	if (!s || !stats) return LFA_E_INVALID;
	stats[0] = stats[1] = 0;
	uint64_t ex[3];
	LFA_TRY(lfa_get_correction_stats_ex(s, ex));
	stats[0] = ex[0];
	stats[1] = ex[1];
	return LFA_OK;
}

extern "C" int lfa_get_correction_stats_ex(lfa_sim *s, uint64_t stats[3]) {
	if (!s || !stats) return LFA_E_INVALID;
	stats[0] = stats[1] = stats[2] = 0;
	if (!s->corr_ovf) return LFA_OK;
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_corr_join(s));
	const size_t ovf_stride = ((size_t)CORR_PARTS * s->g.nt + 31) / 32 + 2;
	uint32_t first = 0, second = 0;
	LFA_HIP(s, hipMemcpyAsync(&first, s->corr_ovf, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipMemcpyAsync(&second, s->corr_ovf + ovf_stride, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	stats[0] = second;
	stats[1] = (uint64_t)CORR_PARTS * (uint64_t)s->corr_parts_tiles;
	stats[2] = first;
	return LFA_OK;
}

extern "C" int lfa_set_step_overlap(lfa_sim *s, int on) {
	if (!s) return LFA_E_INVALID;
	s->overlap_correction = on != 0;
	return LFA_OK;
}

extern "C" int lfa_get_step_timings(lfa_sim *s, double ms[LFA_NUM_STEP_TIMERS]) {
	if (!s || !ms) return LFA_E_INVALID;
	for (int k = 0; k < LFA_NUM_STEP_TIMERS; ++k) ms[k] = s->ms_next[k];
	return LFA_OK;
}
