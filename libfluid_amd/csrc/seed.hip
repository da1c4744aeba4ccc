// libfluid_amd/csrc/seed.hip -- simulation::seed_box / seed_sphere on the device, the reference's particles bit for bit.
//
// The reference's seed_func (include/fluid/simulation.h:80-115) walks the candidate sub-cells one by one - z, y, x over the cell
// range (x fastest), then sx, sy, sz over density^3 sub-cells (sz fastest) - and draws three doubles from its pcg32 for EVERY
// candidate, accepted or not (:98-102). libstdc++'s uniform_real_distribution<double> takes two 32-bit draws per double, so
// candidate i always starts at draw 6 i. pcg32 is a 64-bit linear congruential generator: its state after k draws is an affine
// map of the state before, and the map of 2^j draws is the map of 2^(j-1) draws applied twice, so a thread reaches its
// candidate's state in one multiply-add per set bit of 6 i (table c_jump). From there it repeats the host loop's fp64 arithmetic
// operation by operation (the file is compiled without contraction, like the rest of the library).
//
// Two passes over the candidates, one lane each: k_seed_count evaluates the predicate and leaves the number of accepted
// candidates per wave; their exclusive scan places every wave's particles; k_seed_write evaluates the candidate again (nothing
// is staged between the passes but that one word per wave) and writes key, fractions, velocity, C = 0 and the id straight into
// the resident particle arrays, in candidate order - the order of the reference's particle list.
//
// Slabs (LFA_SEED_COLLECTIVE): a candidate's draws depend on its number alone, so every rank evaluates every candidate and keeps
// the accepted ones whose key lies in its own tile layers - no message. The count pass leaves a second word per wave (accepted AND
// owned), the write pass places a particle by the owned offset and numbers it by the accepted one: the id is the particle's index
// in the single-domain list, the same on whichever rank it lands. A single domain owns every layer and runs the same kernels.
#include "common.h"

#include <cmath>

// ---------------------------------------------------------------------------------------------------- pcg32 jump-ahead
#define PCG_MULT 6364136223846793005ull
#define PCG_INC 1442695040888963407ull

/// mult[j], plus[j]: the state after 2^j draws is mult[j] * state + plus[j] (mult[j] = A^(2^j), plus[j] = c * sum of A^i, i < 2^j).
struct SeedJump {
	uint64_t mult[64], plus[64];
};
static constexpr SeedJump make_seed_jump() {
	SeedJump t{};
	uint64_t m = PCG_MULT, p = PCG_INC;
	for (int j = 0; j < 64; ++j) {
		t.mult[j] = m;
		t.plus[j] = p;
		p = (m + 1ull) * p;
		m = m * m;
	}
	return t;
}
static constexpr SeedJump h_jump = make_seed_jump();
__constant__ SeedJump c_jump = make_seed_jump();

static uint64_t pcg_advance(uint64_t state, uint64_t k) {
	for (int j = 0; k; ++j, k >>= 1)
		if (k & 1ull) state = state * h_jump.mult[j] + h_jump.plus[j];
	return state;
}
__device__ inline uint32_t pcg_next(uint64_t &state) {
	const uint64_t old = state;
	state = old * PCG_MULT + PCG_INC;
	const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27), rot = (uint32_t)(old >> 59);
	return (xs >> rot) | (xs << ((32u - rot) & 31u));
}
/// std::uniform_real_distribution<double>(0, sub)(pcg32) as libstdc++ evaluates it: generate_canonical<double, 53> sums two draws,
/// the first one the low word, divides by 2^64 and steps back below 1 if the sum rounded up to it.
__device__ inline double seed_uniform(uint64_t &state, double sub) {
	const uint32_t r1 = pcg_next(state), r2 = pcg_next(state);
	const double sum = (double)r1 + (double)r2 * 4294967296.0;
	double ret = sum / 18446744073709551616.0;
	if (ret >= 1.0) ret = 0x1.fffffffffffffp-1;  // nextafter(1, 0)
	return ret * (sub - 0.0) + 0.0;
}

// ---------------------------------------------------------------------------------------------------- candidates
struct SeedShape {
	double off[3], h, sub;  // grid_offset, cell_size, cell_size / density
	double lo[3], hi[3];    // box: start, start + size; sphere: lo = centre
	double r2;              // sphere: radius * radius
	uint64_t n_cand, state;
	uint32_t s[3], ex, ey;  // first cell of the range, its extent in x and y (cells)
	uint32_t density, d3;
	int nbits;              // significant bits of 6 * (n_cand - 1)
	int sphere, ltr;
	int nz, slab_lo, slab_hi;  // cells in z; the tile layers [slab_lo, slab_hi) this rank keeps (single domain: all of them)
};

/// Candidate i of the loop nest: its position (the host loop's fp64 arithmetic) and whether the predicate accepts it.
__device__ inline bool seed_candidate(const SeedShape &q, uint64_t i, double (&pos)[3]) {
	const uint32_t cell = (uint32_t)(i / q.d3), sub = (uint32_t)(i - (uint64_t)cell * q.d3);
	const uint32_t xy = q.ex * q.ey, cz = cell / xy, rem = cell - cz * xy, cy = rem / q.ex, cx = rem - cy * q.ex;
	const uint32_t dd = q.density * q.density, sx = sub / dd, srem = sub - sx * dd, sy = srem / q.density, sz = srem - sy * q.density;
	uint64_t st = q.state;
	const uint64_t dist = 6ull * i;
	for (int j = 0; j < q.nbits; ++j)
		if ((dist >> j) & 1ull) st = st * c_jump.mult[j] + c_jump.plus[j];
	// `vec3d(dist(random), dist(random), dist(random))`: g++ evaluates right to left, so z gets the first draw
	double a, b, c;
	if (q.ltr) {
		a = seed_uniform(st, q.sub); b = seed_uniform(st, q.sub); c = seed_uniform(st, q.sub);
	} else {
		c = seed_uniform(st, q.sub); b = seed_uniform(st, q.sub); a = seed_uniform(st, q.sub);
	}
	// grid_offset + cell * cell_size + sub_index * sub + (a, b, c), left to right per component
	pos[0] = ((q.off[0] + (double)(q.s[0] + cx) * q.h) + (double)sx * q.sub) + a;
	pos[1] = ((q.off[1] + (double)(q.s[1] + cy) * q.h) + (double)sy * q.sub) + b;
	pos[2] = ((q.off[2] + (double)(q.s[2] + cz) * q.h) + (double)sz * q.sub) + c;
	if (q.sphere) {
		const double dx = pos[0] - q.lo[0], dy = pos[1] - q.lo[1], dz = pos[2] - q.lo[2];
		double r = dx * dx;
		r += dy * dy;
		r += dz * dz;
		return r < q.r2;
	}
	return pos[0] > q.lo[0] && pos[1] > q.lo[1] && pos[2] > q.lo[2] && pos[0] < q.hi[0] && pos[1] < q.hi[1] && pos[2] < q.hi[2];
}

/// Whether this rank keeps a particle at z: the tile layer of its clamped cell - of its KEY, not of the candidate's loop cell
/// (a draw may round up into the next cell) - is one of the rank's own. cz, tz: cell_and_fraction of z, as the key takes them.
__device__ inline bool seed_owned(const SeedShape &q, double z, int &cz, float &tz) {
	cell_and_fraction(z, q.off[2], q.h, q.nz, cz, tz);
	return (cz >> 3) >= q.slab_lo && (cz >> 3) < q.slab_hi;
}

/// Pass 1: per wave (wave w holds the candidates [64 w, 64 w + 64)) the accepted candidates and those of them this rank keeps.
__global__ void __launch_bounds__(256) k_seed_count(SeedShape q, uint32_t *wave_accepted, uint32_t *wave_owned) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	double pos[3];
	int cz;
	float tz;
	const bool in = i < q.n_cand && seed_candidate(q, i, pos);
	const bool own = in && seed_owned(q, pos[2], cz, tz);
	const unsigned long long m = __ballot(in), mo = __ballot(own);
	if ((threadIdx.x & 63) == 0 && (i >> 6) < ((q.n_cand + 63) >> 6)) {
		wave_accepted[i >> 6] = (uint32_t)__popcll(m);
		wave_owned[i >> 6] = (uint32_t)__popcll(mo);
	}
}

/// Pass 2: the kept candidates become the particles [base, base + total) in candidate order; the id of a particle is id_base + its
/// index among ALL accepted candidates (single domain: every accepted candidate is kept and id_base = base, so id = slot).
__global__ void __launch_bounds__(256) k_seed_write(SeedShape q, const uint32_t *accepted_off, const uint32_t *owned_off, ParticleSoA p,
                                                    size_t base, size_t total, uint64_t id_base, GridDims g, float vx, float vy, float vz,
                                                    double *positions) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	double pos[3];
	int c[3];
	float t[3];
	const bool in = i < q.n_cand && seed_candidate(q, i, pos);
	const bool own = in && seed_owned(q, pos[2], c[2], t[2]);
	const unsigned long long m = __ballot(in), mo = __ballot(own);
	if (!own) return;  // (a wave that keeps nothing ends here)
	const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
	const size_t j = (size_t)owned_off[i >> 6] + (size_t)__popcll(mo & below);
	if (j >= total) return;  // (cannot happen: both passes evaluate the same candidates; keeps a write inside the arrays regardless)
	const size_t d = base + j;
	cell_and_fraction(pos[0], q.off[0], q.h, g.nx, c[0], t[0]);
	cell_and_fraction(pos[1], q.off[1], q.h, g.ny, c[1], t[1]);
	p.key[d] = blocked_index(g, c[0], c[1], c[2]);
#pragma unroll
	for (int k = 0; k < 3; ++k) p.t[k][d] = t[k];
	p.v[0][d] = vx; p.v[1][d] = vy; p.v[2][d] = vz;
#pragma unroll
	for (int k = 0; k < 9; ++k) p.c[k][d] = 0.0f;
	p.id[d] = (uint32_t)(id_base + (uint64_t)accepted_off[i >> 6] + (uint64_t)__popcll(m & below));
	if (positions) {
		positions[3 * j] = pos[0]; positions[3 * j + 1] = pos[1]; positions[3 * j + 2] = pos[2];
	}
}

/// Slabs, records with holes (particles handed to a neighbour since the last binning carry an invalid key): the resident
/// records move to their place among the resident ones (slot = exclusive scan of the valid flags), whole, in storage order.
__global__ void __launch_bounds__(256) k_seed_valid_flags(const uint32_t *key, size_t n, uint32_t *valid) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) valid[i] = key[i] != 0xFFFFFFFFu ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_seed_close_holes(size_t n, ParticleSoA src, ParticleSoA dst, const uint32_t *slot, size_t n_dst) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n || src.key[i] == 0xFFFFFFFFu) return;
	const size_t d = slot[i];
	if (d >= n_dst) return;  // (cannot happen: the caller has compared the scan's total with the resident count)
	dst.key[d] = src.key[i];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		dst.t[k][d] = src.t[k][i];
		dst.v[k][d] = src.v[k][i];
	}
#pragma unroll
	for (int k = 0; k < 9; ++k) dst.c[k][d] = src.c[k][i];
	dst.id[d] = src.id[i];
}

// ---------------------------------------------------------------------------------------------------- fluid sources
/// simulation::seed_cell (src/simulation.cpp:136-151) for the flattened entries of lfa_update_sources, with the reference's draws:
/// new particle k of the call, counted over all entries in order, starts at draw 6 k, and off[i] - the exclusive scan of the
/// entries' needs - is the number of the entry's first particle. One thread per entry: one jump to 6 off[i], then the entry's
/// need[i] particles drawn one after the other, as the host loop draws them. position = (grid_offset + cell * cell_size) + draws
/// in fp64; key and fractions are what an upload of that position stores (cell_and_fraction), not the source cell: a sum that
/// rounds up to the cell's far face lands in the next cell.
__global__ void __launch_bounds__(256) k_source_seed_rng(const uint32_t *cell, const uint32_t *src_of, const uint32_t *need,
                                                         const uint32_t *off, size_t n, const float *src_vel, ParticleSoA p, size_t base,
                                                         size_t total, uint64_t id_base, GridDims g, IngestParams ip, uint64_t state,
                                                         int nbits, int ltr, double *positions) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t cnt = need[i], first = off[i], b = cell[i];
	if (!cnt) return;
	uint64_t st = state;
	const uint64_t dist = 6ull * first;
	for (int j = 0; j < nbits; ++j)
		if ((dist >> j) & 1ull) st = st * c_jump.mult[j] + c_jump.plus[j];
	int tx, ty, tz;
	tile_coords(g, (int)(b >> 9), tx, ty, tz);
	const int l = (int)(b & 511), cc[3] = {tx * 8 + (l & 7), ty * 8 + ((l >> 3) & 7), tz * 8 + (l >> 6)}, nn[3] = {g.nx, g.ny, g.nz};
	double corner[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) corner[k] = ip.off[k] + (double)cc[k] * ip.h;
	const float *vel = src_vel + 3 * src_of[i];
	const float v0 = vel[0], v1 = vel[1], v2 = vel[2];
	for (uint32_t j = 0; j < cnt; ++j) {
		const size_t r = (size_t)first + j;
		if (r >= total) return;  // (cannot happen: total is the scan's sum; keeps a write inside the arrays regardless)
		// `vec3d(dist(random), dist(random), dist(random))` (:145): g++ evaluates right to left, so z gets the first draw
		double u[3];
		if (ltr) {
			u[0] = seed_uniform(st, ip.h); u[1] = seed_uniform(st, ip.h); u[2] = seed_uniform(st, ip.h);
		} else {
			u[2] = seed_uniform(st, ip.h); u[1] = seed_uniform(st, ip.h); u[0] = seed_uniform(st, ip.h);
		}
		const size_t d = base + r;
		int c[3];
		float t[3];
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const double x = corner[k] + u[k];
			cell_and_fraction(x, ip.off[k], ip.h, nn[k], c[k], t[k]);
			p.t[k][d] = t[k];
			if (positions) positions[3 * r + k] = x;
		}
		p.key[d] = blocked_index(g, c[0], c[1], c[2]);
		p.v[0][d] = v0; p.v[1][d] = v1; p.v[2][d] = v2;
#pragma unroll
		for (int k = 0; k < 9; ++k) p.c[k][d] = 0.0f;
		p.id[d] = (uint32_t)(id_base + (uint64_t)r);
	}
}

int lfa_source_seed_rng(lfa_sim *s, const uint32_t *off, size_t base, size_t total, uint64_t id_base, uint64_t state, int ltr,
                        double *positions_dev, uint64_t *state_after) {
	const size_t n = s->n_src_entries;
	*state_after = pcg_advance(state, 6ull * total);
	if (!n || !total) return LFA_OK;
	IngestParams ip;
	for (int k = 0; k < 3; ++k) ip.off[k] = s->prm.grid_offset[k];
	ip.h = s->prm.cell_size;
	const int nbits = 64 - __builtin_clzll(6ull * total | 1ull);
	hipLaunchKernelGGL(k_source_seed_rng, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t *)s->src_cell,
	                   (const uint32_t *)s->src_of, (const uint32_t *)s->src_need, off, n, (const float *)s->src_vel, s->pb[s->cur], base,
	                   total, id_base, s->g, ip, state, nbits, ltr, positions_dev);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

uint64_t lfa_pcg32_advance(uint64_t state, uint64_t draws) { return pcg_advance(state, draws); }

// ---- slabs (LFA_SEED_COLLECTIVE). The draw number of an entry's first particle is its offset among the new particles of ALL
// ranks in source order: lfa_update_sources has summed the ranks' needs into one vector over the job-wide entry list (one
// all-reduce) and scanned it. A particle belongs to the rank whose tile layers hold its KEY, as in the collective lfa_seed_box;
// only a particle of a cell next to a slab face can have its key beyond the face, so the count pass draws those entries (z alone:
// the two coordinates it skips are one jump of four draws) and takes the need of every other entry as it stands. The write pass
// draws like k_source_seed_rng and places the kept particles by the scan of the kept counts, numbered by their draw number.
struct SourceSlabArgs {
	const uint32_t *cell, *of, *gidx, *mode;  // the candidate entries (lfa_sim::SourceSlab)
	const uint32_t *need, *first;             // per job-wide entry
	size_t n_cand;
	GridDims g;
	IngestParams ip;
	uint64_t state;
	int nbits, ltr;
	int slab_lo, slab_hi;  // own tile layers
};

__device__ inline uint64_t source_jump(const SourceSlabArgs &a, uint32_t first) {
	uint64_t st = a.state;
	const uint64_t dist = 6ull * first;
	for (int j = 0; j < a.nbits; ++j)
		if ((dist >> j) & 1ull) st = st * c_jump.mult[j] + c_jump.plus[j];
	return st;
}
__device__ inline void source_cell_coords(const GridDims &g, uint32_t b, int (&cc)[3]) {
	int tx, ty, tz;
	tile_coords(g, (int)(b >> 9), tx, ty, tz);
	const int l = (int)(b & 511);
	cc[0] = tx * 8 + (l & 7); cc[1] = ty * 8 + ((l >> 3) & 7); cc[2] = tz * 8 + (l >> 6);
}
__device__ inline bool source_owned(const SourceSlabArgs &a, double z, int &cz, float &tz) {
	cell_and_fraction(z, a.ip.off[2], a.ip.h, a.g.nz, cz, tz);
	return (cz >> 3) >= a.slab_lo && (cz >> 3) < a.slab_hi;
}

/// Count pass, one thread per candidate entry: keep[c] = its particles whose key lies in the own tile layers.
__global__ void __launch_bounds__(256) k_source_slab_count(SourceSlabArgs a, uint32_t *keep) {
	const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= a.n_cand) return;
	const uint32_t gi = a.gidx[c], cnt = a.need[gi];
	if (!cnt || !a.mode[c]) {  // (mode 0: an own cell with own cells, or the grid's end, below and above it)
		keep[c] = cnt;
		return;
	}
	uint64_t st = source_jump(a, a.first[gi]);
	int cc[3], cz;
	float tz;
	source_cell_coords(a.g, a.cell[c], cc);
	const double corner = a.ip.off[2] + (double)cc[2] * a.ip.h;
	uint32_t k = 0;
	for (uint32_t j = 0; j < cnt; ++j) {
		// z is the first of the three doubles (default) or the last (LFA_SEED_DRAW_LTR); four draws are x and y
		if (a.ltr) st = st * c_jump.mult[2] + c_jump.plus[2];
		const double z = corner + seed_uniform(st, a.ip.h);
		if (!a.ltr) st = st * c_jump.mult[2] + c_jump.plus[2];
		k += source_owned(a, z, cz, tz) ? 1u : 0u;
	}
	keep[c] = k;
}

/// Write pass: the kept particles of candidate c become the records base + keep_off[c] .. in draw order; id = id_base + draw number.
__global__ void __launch_bounds__(256) k_source_slab_write(SourceSlabArgs a, const uint32_t *keep, const uint32_t *keep_off,
                                                           const float *src_vel, ParticleSoA p, size_t base, size_t kept,
                                                           size_t total_all, uint64_t id_base, double *positions) {
	const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= a.n_cand || !keep[c]) return;
	const uint32_t gi = a.gidx[c], cnt = a.need[gi], first = a.first[gi];
	uint64_t st = source_jump(a, first);
	int cc[3];
	source_cell_coords(a.g, a.cell[c], cc);
	const int nn[3] = {a.g.nx, a.g.ny, a.g.nz};
	double corner[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) corner[k] = a.ip.off[k] + (double)cc[k] * a.ip.h;
	const float *vel = src_vel + 3 * a.of[c];
	const float v0 = vel[0], v1 = vel[1], v2 = vel[2];
	size_t w = keep_off[c];
	for (uint32_t j = 0; j < cnt; ++j) {
		double u[3];
		if (a.ltr) {
			u[0] = seed_uniform(st, a.ip.h); u[1] = seed_uniform(st, a.ip.h); u[2] = seed_uniform(st, a.ip.h);
		} else {
			u[2] = seed_uniform(st, a.ip.h); u[1] = seed_uniform(st, a.ip.h); u[0] = seed_uniform(st, a.ip.h);
		}
		double x[3];
#pragma unroll
		for (int k = 0; k < 3; ++k) x[k] = corner[k] + u[k];
		int ci[3];
		float t[3];
		if (!source_owned(a, x[2], ci[2], t[2])) continue;
		// (cannot happen: both passes draw the same numbers; keeps a write inside the arrays regardless)
		if (w >= kept || (size_t)first + j >= total_all) return;
		const size_t d = base + w;
		cell_and_fraction(x[0], a.ip.off[0], a.ip.h, nn[0], ci[0], t[0]);
		cell_and_fraction(x[1], a.ip.off[1], a.ip.h, nn[1], ci[1], t[1]);
		p.key[d] = blocked_index(a.g, ci[0], ci[1], ci[2]);
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			p.t[k][d] = t[k];
			if (positions) positions[3 * w + k] = x[k];
		}
		p.v[0][d] = v0; p.v[1][d] = v1; p.v[2][d] = v2;
#pragma unroll
		for (int k = 0; k < 9; ++k) p.c[k][d] = 0.0f;
		p.id[d] = (uint32_t)(id_base + (uint64_t)first + (uint64_t)j);
		++w;
	}
}

static SourceSlabArgs source_slab_args(lfa_sim *s, size_t total_all, uint64_t state, int ltr) {
	const lfa_sim::SourceSlab &q = s->src_slab;
	SourceSlabArgs a;
	a.cell = q.cell; a.of = q.of; a.gidx = q.gidx; a.mode = q.mode;
	a.need = q.need; a.first = q.first;
	a.n_cand = q.n_cand;
	a.g = s->g;
	for (int k = 0; k < 3; ++k) a.ip.off[k] = s->prm.grid_offset[k];
	a.ip.h = s->prm.cell_size;
	a.state = state;
	a.nbits = 64 - __builtin_clzll(6ull * total_all | 1ull);
	a.ltr = ltr;
	a.slab_lo = s->slab_lo;
	a.slab_hi = s->slab_hi;
	return a;
}

int lfa_source_slab_count(lfa_sim *s, size_t total_all, uint64_t state, int ltr, size_t *kept) {
	const lfa_sim::SourceSlab &q = s->src_slab;
	*kept = 0;
	if (!q.n_cand) return LFA_OK;
	hipLaunchKernelGGL(k_source_slab_count, dim3((unsigned)((q.n_cand + 255) / 256)), dim3(256), 0, s->stream,
	                   source_slab_args(s, total_all, state, ltr), q.keep);
	LFA_LAUNCH_CHECK(s);
	LFA_TRY(lfa_exclusive_scan_u32(s, q.keep, q.keep_off, q.n_cand, q.keep_off + q.n_cand));
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + 105, q.keep_off + q.n_cand, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	*kept = s->h_pinned[105];
	return LFA_OK;
}

int lfa_source_slab_write(lfa_sim *s, size_t base, size_t kept, size_t total_all, uint64_t id_base, uint64_t state, int ltr,
                          double *positions_dev) {
	const lfa_sim::SourceSlab &q = s->src_slab;
	if (!q.n_cand || !kept) return LFA_OK;
	hipLaunchKernelGGL(k_source_slab_write, dim3((unsigned)((q.n_cand + 255) / 256)), dim3(256), 0, s->stream,
	                   source_slab_args(s, total_all, state, ltr), (const uint32_t *)q.keep, (const uint32_t *)q.keep_off,
	                   (const float *)s->src_vel, s->pb[s->cur], base, kept, total_all, id_base, positions_dev);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

// ---------------------------------------------------------------------------------------------------- entry points
/// simulation::world_position_to_cell_index_unclamped (src/simulation.cpp:190-197): max(g, 0) before the conversion.
/// (Anything at or beyond 2^62 cells - far outside every grid - stops there: the conversion itself would not be defined.)
static uint64_t seed_cell_unclamped(double pos, double off, double h) {
	const double g = (pos - off) / h;
	const double m = g < 0.0 ? 0.0 : g;
	return m >= 4611686018427387904.0 ? (uint64_t)1 << 62 : (uint64_t)m;
}

static int seed_shape(lfa_sim *s, SeedShape &q, const double lo[3], const double hi[3], const double velocity[3], uint64_t density,
                      uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions, uint64_t positions_capacity) {
	if (n_seeded) *n_seeded = 0;
	if (s->dist && !(flags & LFA_SEED_COLLECTIVE))
		return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_seed_box / lfa_seed_sphere on a slab decomposition: pass LFA_SEED_COLLECTIVE, and make the "
		                                      "same call with the same arguments and generator state on every rank (each rank scans all "
		                                      "candidates and keeps those of its own tile layers)");
	// ---- what the arguments alone decide: every rank of a collective call fails here alike, or none does
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size before seeding");
	if (density == 0 || density > 16) return lfa_fail(s, LFA_E_INVALID, "seeding density %llu: 1 to 16 per axis", (unsigned long long)density);
	for (int k = 0; k < 3; ++k)
		if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !std::isfinite(velocity[k])) return lfa_fail(s, LFA_E_INVALID, "seeding: a coordinate is not finite");
	if (s->move_pending) return lfa_fail(s, LFA_E_INVALID, "seeding between lfa_advect / lfa_correct and lfa_collide");
	LFA_HIP(s, hipSetDevice(s->device));
	// ---- the reference's cell range (seed_box / seed_sphere, src/simulation.cpp:153-181; seed_func, simulation.h:86-89): e - s + 1 cells, clamped to the grid above
	const uint64_t nn[3] = {(uint64_t)s->g.nx, (uint64_t)s->g.ny, (uint64_t)s->g.nz};
	uint64_t ext[3];
	for (int k = 0; k < 3; ++k) {
		q.off[k] = s->prm.grid_offset[k];
		const uint64_t a = seed_cell_unclamped(lo[k], q.off[k], s->prm.cell_size), e = seed_cell_unclamped(hi[k], q.off[k], s->prm.cell_size);
		const uint64_t end = a + (e - a + 1) < nn[k] ? a + (e - a + 1) : nn[k];
		ext[k] = end > a ? end - a : 0;
		q.s[k] = (uint32_t)(a < nn[k] ? a : nn[k]);
	}
	q.h = s->prm.cell_size;
	q.sub = q.h / (double)density;
	q.density = (uint32_t)density;
	q.d3 = q.density * q.density * q.density;
	q.ex = (uint32_t)ext[0];
	q.ey = (uint32_t)ext[1];
	q.n_cand = ext[0] * ext[1] * ext[2] * q.d3;  // (at most 2^32 cells x 2^12)
	q.state = *rng_state;
	q.ltr = (flags & LFA_SEED_DRAW_LTR) ? 1 : 0;
	q.nz = s->g.nz;
	q.slab_lo = s->dist ? s->slab_lo : 0;
	q.slab_hi = s->dist ? s->slab_hi : s->g.ntz;
	// the id of the call's first particle: the job-wide numbering on slabs, the record index on a single domain
	const uint64_t id_base = s->dist ? s->next_global_id : (uint64_t)s->np;
	if (q.n_cand == 0) {  // an empty range draws nothing
		s->seed_last[0] = s->seed_last[1] = 0;
		s->seed_last[2] = id_base;
		return LFA_OK;
	}
	if (q.n_cand >= (uint64_t)1 << 38) return lfa_fail(s, LFA_E_INVALID, "seeding: %llu candidates", (unsigned long long)q.n_cand);
	q.nbits = 64 - __builtin_clzll(6ull * (q.n_cand - 1) | 1ull);
	const uint64_t new_state = pcg_advance(q.state, 6ull * q.n_cand);

	LFA_TRY(lfa_corr_commit(s));
	const size_t n_waves = (size_t)((q.n_cand + 63) >> 6);
	const unsigned blocks = (unsigned)((q.n_cand + 255) >> 8);
	// [accepted per wave, then their exclusive scan | the total] [the same for accepted-and-owned] [records that survive close_holes]
	uint32_t *wave = nullptr;
	LFA_HIP(s, hipMalloc(&wave, (2 * (n_waves + 1) + 1) * 4));
	uint32_t *const acc = wave, *const own = wave + n_waves + 1, *const n_valid = wave + 2 * (n_waves + 1);
	auto run = [&]() -> int {
		hipLaunchKernelGGL(k_seed_count, dim3(blocks), dim3(256), 0, s->stream, q, acc, own);
		LFA_LAUNCH_CHECK(s);
		LFA_TRY(lfa_exclusive_scan_u32(s, acc, acc, n_waves, acc + n_waves));
		LFA_TRY(lfa_exclusive_scan_u32(s, own, own, n_waves, own + n_waves));
		LFA_HIP(s, hipMemcpyAsync(s->h_pinned + 97, acc + n_waves, 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipMemcpyAsync(s->h_pinned + 98, own + n_waves, 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipStreamSynchronize(s->stream));
		// total_all: accepted in the whole job (the same on every rank); total: kept here; base: resident particles
		const size_t total_all = s->h_pinned[97], total = s->h_pinned[98], base = s->np;
		if (id_base + total_all >= ((uint64_t)1 << 32) || base + total >= ((size_t)1 << 32)) return lfa_fail(s, LFA_E_INVALID, "more than 2^32 particles");
		if (positions && positions_capacity < total)
			return lfa_fail(s, LFA_E_INVALID, "seeding: room for %llu positions but %zu particles", (unsigned long long)positions_capacity, total);
		auto done = [&]() {
			if (s->dist) s->next_global_id = id_base + total_all;
			s->seed_last[0] = q.n_cand;
			s->seed_last[1] = total_all;
			s->seed_last[2] = id_base;
			if (n_seeded) *n_seeded = total;
			*rng_state = new_state;
			return LFA_OK;
		};
		// every candidate was drawn, none kept: the particles stay as they are (slabs: the numbering moves on with the job's)
		if (total == 0) return done();
		if (positions) LFA_TRY(lfa_ensure_io(s, total * 24));
		// records of the current buffer: slabs between a hand-over and the next binning hold the leavers' holes among them
		size_t n_rec = s->binned ? s->np_live : s->np;
		if (base == 0) {  // nothing resident (the usual case): nothing to keep, no deferred binning to complete
			LFA_TRY(lfa_particles_alloc(s, total));
			s->vc_pending = false;
			s->c_home_valid = false;
			s->cur = 0;
		} else {  // append behind the resident particles, like the seeding of lfa_update_sources
			LFA_TRY(lfa_particles_materialize(s));
			LFA_TRY(lfa_c_home_restore(s));  // C of the resident particles back beside them: the new ones carry C = 0 in place
			LFA_TRY(lfa_particles_reserve(s, n_rec, n_rec > base + total ? n_rec : base + total));
			// (nothing below fails for want of memory: from here on the handle changes)
			if (s->dist && s->holes) {  // close the holes: [0, base) are the resident records again, the other buffer is free
				hipLaunchKernelGGL(k_seed_valid_flags, dim3((unsigned)((n_rec + 255) >> 8)), dim3(256), 0, s->stream,
				                   (const uint32_t *)s->pb[s->cur].key, n_rec, s->rank);
				LFA_LAUNCH_CHECK(s);
				LFA_TRY(lfa_exclusive_scan_u32(s, s->rank, s->rank, n_rec, n_valid));
				LFA_HIP(s, hipMemcpyAsync(s->h_pinned + 99, n_valid, 4, hipMemcpyDeviceToHost, s->stream));
				LFA_HIP(s, hipStreamSynchronize(s->stream));
				// (unbinned, np counted the holes too - lfa_dist_migrate -: then the scan is what tells the resident count)
				if (s->binned && (size_t)s->h_pinned[99] != base)
					return lfa_fail(s, LFA_E_INVALID, "seeding: %u resident records but %zu expected", s->h_pinned[99], base);
				const size_t n_dst = s->h_pinned[99];
				hipLaunchKernelGGL(k_seed_close_holes, dim3((unsigned)((n_rec + 255) >> 8)), dim3(256), 0, s->stream, n_rec, s->pb[s->cur],
				                   s->pb[s->cur ^ 1], (const uint32_t *)s->rank, n_dst);
				LFA_LAUNCH_CHECK(s);
				s->cur ^= 1;
				s->binned = false;  // the order of the last binning is gone
				s->np = s->np_live = n_dst;
				s->holes = false;
			}
		}
		const size_t at = s->np;  // (== base, but for an unbinned slab handle whose holes were just closed)
		hipLaunchKernelGGL(k_seed_write, dim3(blocks), dim3(256), 0, s->stream, q, (const uint32_t *)acc, (const uint32_t *)own, s->pb[s->cur], at,
		                   total, id_base, s->g, (float)velocity[0], (float)velocity[1], (float)velocity[2],
		                   positions ? (double *)s->io_buf : (double *)nullptr);
		LFA_LAUNCH_CHECK(s);
		s->np = at + total;
		s->np_live = s->np;
		s->next_global_id = s->np;  // (slabs: done() puts the job-wide count there)
		s->holes = false;
		s->n_arrivals = 0;
		s->n_ghost_particles = 0;
		s->binned = false;
		s->grid_valid = false;
		s->system_valid = false;
		s->unknown_count_valid = false;
		s->vmax2_valid = false;
		if (positions) {
			LFA_HIP(s, hipMemcpyAsync(positions, s->io_buf, total * 24, hipMemcpyDeviceToHost, s->stream));
			LFA_HIP(s, hipStreamSynchronize(s->stream));
		}
		return done();
	};
	const int rc = run();
	// (the release waits for the device, so the kernels that read the scratch are done with it)
	if (hipFree(wave) != hipSuccess && rc >= 0) return lfa_fail(s, LFA_E_HIP, "releasing the seeding scratch failed");
	return rc;
}

extern "C" int lfa_seed_last(const lfa_sim *s, uint64_t out[3]) {
	if (!s || !out) return LFA_E_INVALID;
	for (int k = 0; k < 3; ++k) out[k] = s->seed_last[k];
	return LFA_OK;
}

extern "C" int lfa_seed_box(lfa_sim *s, const double start[3], const double size[3], const double velocity[3], uint64_t density,
                            uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions, uint64_t positions_capacity) {
	if (!s || !start || !size || !velocity || !rng_state) return LFA_E_INVALID;
	SeedShape q{};
	for (int k = 0; k < 3; ++k) {
		q.lo[k] = start[k];
		q.hi[k] = start[k] + size[k];
	}
	return seed_shape(s, q, q.lo, q.hi, velocity, density, rng_state, flags, n_seeded, positions, positions_capacity);
}

extern "C" int lfa_seed_sphere(lfa_sim *s, const double centre[3], double radius, const double velocity[3], uint64_t density,
                               uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions, uint64_t positions_capacity) {
	if (!s || !centre || !velocity || !rng_state) return LFA_E_INVALID;
	SeedShape q{};
	double lo[3], hi[3];
	for (int k = 0; k < 3; ++k) {
		q.lo[k] = centre[k];
		lo[k] = centre[k] - radius;
		hi[k] = centre[k] + radius;
	}
	q.r2 = radius * radius;
	q.sphere = 1;
	return seed_shape(s, q, lo, hi, velocity, density, rng_state, flags, n_seeded, positions, positions_capacity);
}
