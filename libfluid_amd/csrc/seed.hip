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

/// Pass 1: accepted candidates per wave (wave w holds the candidates [64 w, 64 w + 64)).
__global__ void __launch_bounds__(256) k_seed_count(SeedShape q, uint32_t *wave_count) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	double pos[3];
	const bool in = i < q.n_cand && seed_candidate(q, i, pos);
	const unsigned long long m = __ballot(in);
	if ((threadIdx.x & 63) == 0 && (i >> 6) < ((q.n_cand + 63) >> 6)) wave_count[i >> 6] = (uint32_t)__popcll(m);
}

/// Pass 2: the accepted candidates become the particles [base, base + total) in candidate order.
__global__ void __launch_bounds__(256) k_seed_write(SeedShape q, const uint32_t *wave_off, ParticleSoA p, size_t base, size_t total,
                                                    GridDims g, float vx, float vy, float vz, double *positions) {
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	double pos[3];
	const bool in = i < q.n_cand && seed_candidate(q, i, pos);
	const unsigned long long m = __ballot(in);
	if (!in) return;
	const int lane = threadIdx.x & 63;
	const size_t j = (size_t)wave_off[i >> 6] + (size_t)__popcll(m & ((1ull << lane) - 1ull));
	if (j >= total) return;  // (cannot happen: both passes evaluate the same candidates; keeps a write inside the arrays regardless)
	const size_t d = base + j;
	int c[3];
	float t[3];
	cell_and_fraction(pos[0], q.off[0], q.h, g.nx, c[0], t[0]);
	cell_and_fraction(pos[1], q.off[1], q.h, g.ny, c[1], t[1]);
	cell_and_fraction(pos[2], q.off[2], q.h, g.nz, c[2], t[2]);
	p.key[d] = blocked_index(g, c[0], c[1], c[2]);
#pragma unroll
	for (int k = 0; k < 3; ++k) p.t[k][d] = t[k];
	p.v[0][d] = vx; p.v[1][d] = vy; p.v[2][d] = vz;
#pragma unroll
	for (int k = 0; k < 9; ++k) p.c[k][d] = 0.0f;
	p.id[d] = (uint32_t)d;
	if (positions) {
		positions[3 * j] = pos[0]; positions[3 * j + 1] = pos[1]; positions[3 * j + 2] = pos[2];
	}
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
	if (s->dist)
		return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_seed_box / lfa_seed_sphere: not on a slab decomposition (every rank would have to scan "
		                                      "all candidates and keep those of its own layers)");
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
	if (q.n_cand == 0) return LFA_OK;  // an empty range draws nothing
	if (q.n_cand >= (uint64_t)1 << 38) return lfa_fail(s, LFA_E_INVALID, "seeding: %llu candidates", (unsigned long long)q.n_cand);
	q.nbits = 64 - __builtin_clzll(6ull * (q.n_cand - 1) | 1ull);
	const uint64_t new_state = pcg_advance(q.state, 6ull * q.n_cand);

	LFA_TRY(lfa_corr_commit(s));
	const size_t n_waves = (size_t)((q.n_cand + 63) >> 6);
	const unsigned blocks = (unsigned)((q.n_cand + 255) >> 8);
	uint32_t *wave = nullptr;  // counts, then their exclusive scan | the total
	LFA_HIP(s, hipMalloc(&wave, (n_waves + 1) * 4));
	auto run = [&]() -> int {
		hipLaunchKernelGGL(k_seed_count, dim3(blocks), dim3(256), 0, s->stream, q, wave);
		LFA_LAUNCH_CHECK(s);
		LFA_TRY(lfa_exclusive_scan_u32(s, wave, wave, n_waves, wave + n_waves));
		LFA_HIP(s, hipMemcpyAsync(s->h_pinned + 97, wave + n_waves, 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipStreamSynchronize(s->stream));
		const size_t total = s->h_pinned[97], base = s->np;
		if (positions && positions_capacity < total)
			return lfa_fail(s, LFA_E_INVALID, "seeding: room for %llu positions but %zu particles", (unsigned long long)positions_capacity, total);
		if (base + total >= ((size_t)1 << 32)) return lfa_fail(s, LFA_E_INVALID, "more than 2^32 particles");
		if (total == 0) {  // every candidate was drawn, none accepted: the handle stays as it is
			*rng_state = new_state;
			return LFA_OK;
		}
		if (base == 0) {  // nothing resident (the usual case): nothing to keep, no deferred binning to complete
			LFA_TRY(lfa_particles_alloc(s, total));
			s->vc_pending = false;
			s->c_home_valid = false;
			s->cur = 0;
		} else {  // append behind the resident particles, like the seeding of lfa_update_sources
			LFA_TRY(lfa_particles_materialize(s));
			LFA_TRY(lfa_c_home_restore(s));  // C of the resident particles back beside them: the new ones carry C = 0 in place
			LFA_TRY(lfa_particles_reserve(s, base, base + total));
		}
		if (positions) LFA_TRY(lfa_ensure_io(s, total * 24));
		hipLaunchKernelGGL(k_seed_write, dim3(blocks), dim3(256), 0, s->stream, q, (const uint32_t *)wave, s->pb[s->cur], base, total, s->g,
		                   (float)velocity[0], (float)velocity[1], (float)velocity[2], positions ? (double *)s->io_buf : (double *)nullptr);
		LFA_LAUNCH_CHECK(s);
		s->np = base + total;
		s->np_live = s->np;
		s->next_global_id = s->np;
		s->binned = false;
		s->grid_valid = false;
		s->system_valid = false;
		s->unknown_count_valid = false;
		s->vmax2_valid = false;
		if (positions) {
			LFA_HIP(s, hipMemcpyAsync(positions, s->io_buf, total * 24, hipMemcpyDeviceToHost, s->stream));
			LFA_HIP(s, hipStreamSynchronize(s->stream));
		}
		if (n_seeded) *n_seeded = total;
		*rng_state = new_state;
		return LFA_OK;
	};
	const int rc = run();
	// (the release waits for the device, so the kernels that read the scratch are done with it)
	if (hipFree(wave) != hipSuccess && rc >= 0) return lfa_fail(s, LFA_E_HIP, "releasing the seeding scratch failed");
	return rc;
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
