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
//
// Fluid sources that draw from the pcg32 (lfa_update_sources_rng) go the same way, one thread per entry: k_source_count (slabs
// only) and k_source_write; a single domain is the write kernel with every layer owned and every entry its own candidate.
//
// One copy of each idea, shared by both: pcg_jump (the jump-ahead), seed_draw3 / seed_draw_z (the three doubles of a particle in
// the reference's order), seed_owned (does this rank keep the particle at z) and born_particle (the record of a new particle).
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

/// `state` after `draws` further 32-bit draws (pcg_advance on the device); nbits: significant bits of the launch's largest `draws`.
__device__ inline uint64_t pcg_jump(uint64_t state, uint64_t draws, int nbits) {
	for (int j = 0; j < nbits; ++j)
		if ((draws >> j) & 1ull) state = state * c_jump.mult[j] + c_jump.plus[j];
	return state;
}
/// `vec3d(dist(random), dist(random), dist(random))` (simulation.h:98-102, src/simulation.cpp:145): g++ evaluates right to left, so z
/// gets the first of the three doubles; ltr (LFA_SEED_DRAW_LTR): x does.
__device__ inline void seed_draw3(uint64_t &state, double width, int ltr, double (&u)[3]) {
	if (ltr) {
		u[0] = seed_uniform(state, width); u[1] = seed_uniform(state, width); u[2] = seed_uniform(state, width);
	} else {
		u[2] = seed_uniform(state, width); u[1] = seed_uniform(state, width); u[0] = seed_uniform(state, width);
	}
}
/// The u[2] of seed_draw3 alone, the state moved on alike: the four draws of x and y are one step through c_jump.
__device__ inline double seed_draw_z(uint64_t &state, double width, int ltr) {
	if (ltr) state = state * c_jump.mult[2] + c_jump.plus[2];
	const double z = seed_uniform(state, width);
	if (!ltr) state = state * c_jump.mult[2] + c_jump.plus[2];
	return z;
}
/// Whether this rank keeps a particle at z: the tile layer of its clamped cell - of its KEY, not of the cell it was drawn for (a
/// draw may round up into the next cell) - is one of [slab_lo, slab_hi). cz, tz: cell_and_fraction of z, as the key takes them.
__device__ inline bool seed_owned(double z, const IngestParams &ip, int nz, int slab_lo, int slab_hi, int &cz, float &tz) {
	cell_and_fraction(z, ip.off[2], ip.h, nz, cz, tz);
	return (cz >> 3) >= slab_lo && (cz >> 3) < slab_hi;
}
/// The record d of a particle born at x: key and fractions as an upload of x stores them (cz, tz: what seed_owned took of x[2]),
/// the velocity, C = 0 and the id; x itself to pos_out[0..2] unless that is null.
__device__ inline void born_particle(const ParticleSoA &p, size_t d, const GridDims &g, const IngestParams &ip, const double (&x)[3], int cz,
                                     float tz, float v0, float v1, float v2, uint32_t id, double *pos_out) {
	int cx, cy;
	float tx, ty;
	cell_and_fraction(x[0], ip.off[0], ip.h, g.nx, cx, tx);
	cell_and_fraction(x[1], ip.off[1], ip.h, g.ny, cy, ty);
	pos_store(p.pos, d, blocked_index(g, cx, cy, cz), tx, ty, tz);
	p.v[0][d] = v0; p.v[1][d] = v1; p.v[2][d] = v2;
	particle_zero_c_set_id(p, d, id);
	if (pos_out) {
		pos_out[0] = x[0]; pos_out[1] = x[1]; pos_out[2] = x[2];
	}
}

// ---------------------------------------------------------------------------------------------------- candidates
struct SeedShape {
	IngestParams ip;        // grid_offset, cell_size
	double sub;             // cell_size / density
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
	uint64_t st = pcg_jump(q.state, 6ull * i, q.nbits);
	double u[3];
	seed_draw3(st, q.sub, q.ltr, u);
	// grid_offset + cell * cell_size + sub_index * sub + u, left to right per component
	pos[0] = ((q.ip.off[0] + (double)(q.s[0] + cx) * q.ip.h) + (double)sx * q.sub) + u[0];
	pos[1] = ((q.ip.off[1] + (double)(q.s[1] + cy) * q.ip.h) + (double)sy * q.sub) + u[1];
	pos[2] = ((q.ip.off[2] + (double)(q.s[2] + cz) * q.ip.h) + (double)sz * q.sub) + u[2];
	if (q.sphere) {
		const double dx = pos[0] - q.lo[0], dy = pos[1] - q.lo[1], dz = pos[2] - q.lo[2];
		double r = dx * dx;
		r += dy * dy;
		r += dz * dz;
		return r < q.r2;
	}
	return pos[0] > q.lo[0] && pos[1] > q.lo[1] && pos[2] > q.lo[2] && pos[0] < q.hi[0] && pos[1] < q.hi[1] && pos[2] < q.hi[2];
}

/// Pass 1: per wave (wave w holds the candidates [64 w, 64 w + 64)) the accepted candidates and those of them this rank keeps.
__global__ void __launch_bounds__(256) k_seed_count(SeedShape q, uint32_t *wave_accepted, uint32_t *wave_owned) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	double pos[3];
	int cz;
	float tz;
	const bool in = i < q.n_cand && seed_candidate(q, i, pos);
	const bool own = in && seed_owned(pos[2], q.ip, q.nz, q.slab_lo, q.slab_hi, cz, tz);
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
	int cz;
	float tz;
	const bool in = i < q.n_cand && seed_candidate(q, i, pos);
	const bool own = in && seed_owned(pos[2], q.ip, q.nz, q.slab_lo, q.slab_hi, cz, tz);
	const unsigned long long m = __ballot(in), mo = __ballot(own);
	if (!own) return;  // (a wave that keeps nothing ends here)
	const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
	const size_t j = (size_t)owned_off[i >> 6] + (size_t)__popcll(mo & below);
	if (j >= total) return;  // (cannot happen: both passes evaluate the same candidates; keeps a write inside the arrays regardless)
	born_particle(p, base + j, g, q.ip, pos, cz, tz, vx, vy, vz, (uint32_t)(id_base + (uint64_t)accepted_off[i >> 6] + (uint64_t)__popcll(m & below)),
	              positions ? positions + 3 * j : nullptr);
}

// ---------------------------------------------------------------------------------------------------- fluid sources
/// simulation::seed_cell (src/simulation.cpp:136-151) for the flattened entries of lfa_update_sources, with the reference's draws:
/// new particle k of the call, counted over the entries of ALL ranks in source order, starts at draw 6 k, and first[] - the
/// exclusive scan of the entries' needs - is the number of an entry's first particle. One thread per entry: one jump to 6 first,
/// then the entry's particles drawn one after the other, as the host loop draws them. position = (grid_offset + cell * cell_size) +
/// draws in fp64; key and fractions are what an upload of that position stores (cell_and_fraction), not the source cell: a sum that
/// rounds up to the cell's far face lands in the next cell.
///
/// Slabs (LFA_SEED_COLLECTIVE): lfa_update_sources has summed the ranks' needs into one vector over the job-wide entry list (one
/// all-reduce) and scanned it. A particle belongs to the rank whose tile layers hold its KEY, as in the collective lfa_seed_box;
/// only a particle of a cell next to a slab face can have its key beyond the face, so the count pass draws those entries (z alone)
/// and takes the need of every other entry as it stands; the write pass places the kept particles by the scan of the kept counts,
/// numbered by their draw number. A single domain keeps every particle: no count pass, keep = need and keep_off = first.
struct SourceArgs {
	const uint32_t *cell, *of, *gidx, *mode;  // the candidate entries (lfa_sim::SourceSlab); gidx null: entry c is job-wide entry c
	const uint32_t *need, *first;             // per job-wide entry
	uint32_t *keep;                           // per candidate: its particles this rank keeps, ...
	const uint32_t *keep_off;                 // ... their exclusive scan
	size_t n_cand;
	GridDims g;
	IngestParams ip;
	uint64_t state;
	int nbits, ltr;
	int slab_lo, slab_hi;  // own tile layers
};

/// Count pass, one thread per candidate entry: keep[c] = its particles whose key lies in the own tile layers.
__global__ void __launch_bounds__(256) k_source_count(SourceArgs a) {
	const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= a.n_cand) return;
	const uint32_t gi = a.gidx[c], cnt = a.need[gi];
	if (!cnt || !a.mode[c]) {  // (mode 0: an own cell with own cells, or the grid's end, below and above it)
		a.keep[c] = cnt;
		return;
	}
	uint64_t st = pcg_jump(a.state, 6ull * a.first[gi], a.nbits);
	int cc[3], cz;
	float tz;
	cell_coords(a.g, a.cell[c], cc);
	const double corner = a.ip.off[2] + (double)cc[2] * a.ip.h;
	uint32_t k = 0;
	for (uint32_t j = 0; j < cnt; ++j)
		k += seed_owned(corner + seed_draw_z(st, a.ip.h, a.ltr), a.ip, a.g.nz, a.slab_lo, a.slab_hi, cz, tz) ? 1u : 0u;
	a.keep[c] = k;
}

/// Write pass: the kept particles of candidate c become the records base + keep_off[c] .. in draw order; id = id_base + draw number.
__global__ void __launch_bounds__(256) k_source_write(SourceArgs a, const float *src_vel, ParticleSoA p, size_t base, size_t kept,
                                                      size_t total_all, uint64_t id_base, double *positions) {
	const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= a.n_cand || !a.keep[c]) return;
	const uint32_t gi = a.gidx ? a.gidx[c] : (uint32_t)c, cnt = a.need[gi], first = a.first[gi];
	uint64_t st = pcg_jump(a.state, 6ull * first, a.nbits);
	int cc[3];
	cell_coords(a.g, a.cell[c], cc);
	double corner[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) corner[k] = a.ip.off[k] + (double)cc[k] * a.ip.h;
	const float *vel = src_vel + 3 * a.of[c];
	const float v0 = vel[0], v1 = vel[1], v2 = vel[2];
	size_t w = a.keep_off[c];
	for (uint32_t j = 0; j < cnt; ++j) {
		double u[3], x[3];
		seed_draw3(st, a.ip.h, a.ltr, u);
#pragma unroll
		for (int k = 0; k < 3; ++k) x[k] = corner[k] + u[k];
		int cz;
		float tz;
		if (!seed_owned(x[2], a.ip, a.g.nz, a.slab_lo, a.slab_hi, cz, tz)) continue;
		// (cannot happen: both passes draw the same numbers, and kept / total_all are the scans' sums; keeps a write inside the arrays regardless)
		if (w >= kept || (size_t)first + j >= total_all) return;
		born_particle(p, base + w, a.g, a.ip, x, cz, tz, v0, v1, v2, (uint32_t)(id_base + (uint64_t)first + (uint64_t)j),
		              positions ? positions + 3 * w : nullptr);
		++w;
	}
}

static SourceArgs source_args(lfa_sim *s, size_t total_all, uint64_t state, int ltr) {
	const lfa_sim::SourceSlab &q = s->src_slab;
	SourceArgs a{};
	if (s->dist) {
		a.cell = q.cell; a.of = q.of; a.gidx = q.gidx; a.mode = q.mode;
		a.need = q.need; a.first = q.first; a.keep = q.keep; a.keep_off = q.keep_off;
		a.n_cand = q.n_cand;
		a.slab_lo = s->slab_lo;
		a.slab_hi = s->slab_hi;
	} else {  // every layer owned, every entry its own candidate and keeping all it needs
		a.cell = s->src_cell; a.of = s->src_of;
		a.need = a.keep = s->src_need;
		a.first = a.keep_off = s->src_need + s->src_cap + 1;
		a.n_cand = s->n_src_entries;
		a.slab_hi = s->g.ntz;
	}
	a.g = s->g;
	a.ip = lfa_ingest_params(s);
	a.state = state;
	a.nbits = 64 - __builtin_clzll(6ull * total_all | 1ull);
	a.ltr = ltr;
	return a;
}

int lfa_source_count(lfa_sim *s, size_t total_all, uint64_t state, int ltr, size_t *kept) {
	const lfa_sim::SourceSlab &q = s->src_slab;
	*kept = 0;
	if (!q.n_cand) return LFA_OK;
	hipLaunchKernelGGL(k_source_count, dim3((unsigned)((q.n_cand + 255) / 256)), dim3(256), 0, s->stream, source_args(s, total_all, state, ltr));
	LFA_LAUNCH_CHECK(s);
	return lfa_scan_total(s, q.keep, q.keep_off, q.n_cand, q.keep_off + q.n_cand, LFA_PIN_SOURCE_KEPT, kept);
}

int lfa_source_write(lfa_sim *s, size_t base, size_t kept, size_t total_all, uint64_t id_base, uint64_t state, int ltr,
                     double *positions_dev) {
	const size_t n_cand = s->dist ? s->src_slab.n_cand : s->n_src_entries;
	if (!n_cand || !kept) return LFA_OK;
	hipLaunchKernelGGL(k_source_write, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, s->stream, source_args(s, total_all, state, ltr),
	                   (const float *)s->src_vel, s->pb[s->cur], base, kept, total_all, id_base, positions_dev);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

uint64_t lfa_pcg32_advance(uint64_t state, uint64_t draws) { return pcg_advance(state, draws); }

// ---------------------------------------------------------------------------------------------------- entry points
/// simulation::world_position_to_cell_index_unclamped (src/simulation.cpp:190-197): max(g, 0) before the conversion.
/// (Anything at or beyond 2^62 cells - far outside every grid - stops there: the conversion itself would not be defined.)
static uint64_t seed_cell_unclamped(double pos, double off, double h) {
	const double g = (pos - off) / h;
	const double m = g < 0.0 ? 0.0 : g;
	return m >= 4611686018427387904.0 ? (uint64_t)1 << 62 : (uint64_t)m;
}

/// The reference's cell range (seed_box / seed_sphere, src/simulation.cpp:153-181; seed_func, simulation.h:86-89) - e - s + 1 cells,
/// clamped to the grid above - and with it everything of q that the arguments decide (the predicate's own fields are the caller's).
static void seed_range(const lfa_sim *s, SeedShape &q, const double lo[3], const double hi[3], uint64_t density, uint64_t state, int flags) {
	const uint64_t nn[3] = {(uint64_t)s->g.nx, (uint64_t)s->g.ny, (uint64_t)s->g.nz};
	uint64_t ext[3];
	q.ip = lfa_ingest_params(s);
	for (int k = 0; k < 3; ++k) {
		const uint64_t a = seed_cell_unclamped(lo[k], q.ip.off[k], q.ip.h), e = seed_cell_unclamped(hi[k], q.ip.off[k], q.ip.h);
		const uint64_t end = a + (e - a + 1) < nn[k] ? a + (e - a + 1) : nn[k];
		ext[k] = end > a ? end - a : 0;
		q.s[k] = (uint32_t)(a < nn[k] ? a : nn[k]);
	}
	q.sub = q.ip.h / (double)density;
	q.density = (uint32_t)density;
	q.d3 = q.density * q.density * q.density;
	q.ex = (uint32_t)ext[0];
	q.ey = (uint32_t)ext[1];
	q.n_cand = ext[0] * ext[1] * ext[2] * q.d3;  // (at most 2^32 cells x 2^12)
	q.nbits = q.n_cand ? 64 - __builtin_clzll(6ull * (q.n_cand - 1) | 1ull) : 0;
	q.state = state;
	q.ltr = (flags & LFA_SEED_DRAW_LTR) ? 1 : 0;
	q.nz = s->g.nz;
	q.slab_lo = s->dist ? s->slab_lo : 0;
	q.slab_hi = s->dist ? s->slab_hi : s->g.ntz;
}

/// The `total` kept candidates behind the resident particles: room, the write pass, the handle's bookkeeping.
static int seed_append(lfa_sim *s, const SeedShape &q, const uint32_t *acc, const uint32_t *own, size_t total, uint64_t id_base,
                       const double velocity[3], double *positions) {
	const size_t base = s->np;
	if (positions) LFA_TRY(lfa_ensure_io(s, total * 24));
	// records of the current buffer: slabs between a hand-over and the next binning hold the leavers' holes among them
	const size_t n_rec = s->binned ? s->np_live : s->np;
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
		if (s->dist && s->holes) LFA_TRY(lfa_particles_close_holes(s, n_rec));  // [0, np) are the resident records again, the other buffer is free
	}
	const size_t at = s->np;  // (== base, but for an unbinned slab handle whose holes were just closed)
	hipLaunchKernelGGL(k_seed_write, dim3((unsigned)((q.n_cand + 255) >> 8)), dim3(256), 0, s->stream, q, acc, own, s->pb[s->cur], at, total,
	                   id_base, s->g, (float)velocity[0], (float)velocity[1], (float)velocity[2],
	                   positions ? (double *)s->io_buf : (double *)nullptr);
	LFA_LAUNCH_CHECK(s);
	s->np = at + total;
	s->np_live = s->np;
	s->next_global_id = s->np;  // (slabs: the caller puts the job-wide count there)
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
	return LFA_OK;
}

/// The two passes. wave: [accepted per wave, then their exclusive scan | the total] [the same for accepted-and-owned].
static int seed_passes(lfa_sim *s, const SeedShape &q, uint32_t *wave, uint64_t id_base, const double velocity[3], uint64_t *rng_state,
                       uint64_t *n_seeded, double *positions, uint64_t positions_capacity) {
	const size_t n_waves = (size_t)((q.n_cand + 63) >> 6);
	uint32_t *const acc = wave, *const own = wave + n_waves + 1;
	hipLaunchKernelGGL(k_seed_count, dim3((unsigned)((q.n_cand + 255) >> 8)), dim3(256), 0, s->stream, q, acc, own);
	LFA_LAUNCH_CHECK(s);
	LFA_TRY(lfa_exclusive_scan_u32(s, acc, acc, n_waves, acc + n_waves));
	LFA_TRY(lfa_exclusive_scan_u32(s, own, own, n_waves, own + n_waves));
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + LFA_PIN_SEED_ACCEPTED, acc + n_waves, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + LFA_PIN_SEED_OWNED, own + n_waves, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	// total_all: accepted in the whole job (the same on every rank); total: kept here
	const size_t total_all = s->h_pinned[LFA_PIN_SEED_ACCEPTED], total = s->h_pinned[LFA_PIN_SEED_OWNED];
	if (id_base + total_all >= ((uint64_t)1 << 32) || s->np + total >= ((size_t)1 << 32)) return lfa_fail(s, LFA_E_INVALID, "more than 2^32 particles");
	if (positions && positions_capacity < total)
		return lfa_fail(s, LFA_E_INVALID, "seeding: room for %llu positions but %zu particles", (unsigned long long)positions_capacity, total);
	// every candidate was drawn, none kept: the particles stay as they are (slabs: the numbering moves on with the job's)
	if (total) LFA_TRY(seed_append(s, q, acc, own, total, id_base, velocity, positions));
	if (s->dist) s->next_global_id = id_base + total_all;
	s->seed_last[0] = q.n_cand;
	s->seed_last[1] = total_all;
	s->seed_last[2] = id_base;
	if (n_seeded) *n_seeded = total;
	*rng_state = pcg_advance(q.state, 6ull * q.n_cand);
	return LFA_OK;
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
	seed_range(s, q, lo, hi, density, *rng_state, flags);
	// the id of the call's first particle: the job-wide numbering on slabs, the record index on a single domain
	const uint64_t id_base = s->dist ? s->next_global_id : (uint64_t)s->np;
	if (q.n_cand == 0) {  // an empty range draws nothing
		s->seed_last[0] = s->seed_last[1] = 0;
		s->seed_last[2] = id_base;
		return LFA_OK;
	}
	if (q.n_cand >= (uint64_t)1 << 38) return lfa_fail(s, LFA_E_INVALID, "seeding: %llu candidates", (unsigned long long)q.n_cand);
	LFA_TRY(lfa_corr_commit(s));
	uint32_t *wave = nullptr;
	LFA_HIP(s, hipMalloc(&wave, 2 * (((q.n_cand + 63) >> 6) + 1) * 4));
	const int rc = seed_passes(s, q, wave, id_base, velocity, rng_state, n_seeded, positions, positions_capacity);
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
