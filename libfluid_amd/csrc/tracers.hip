// libfluid_amd/csrc/tracers.hip -- tracers: massless markers that live on the device and move as a PIC particle of the reference does,
// seen by no grid stage (P2G, pressure solve, position correction). Dye, debris, foam seeds, streak lines.
//
// A host with such points had one route per step: lfa_sample_velocity (24 bytes per point up, 24 down), the move on the host, and
// for the obstacles lfa_download_cells (32 bytes per cell) plus its own copy of _detect_collisions. Here the points stay where the
// grid is; a step reads 48 bytes per tracer and writes 49.
//
// Step n of the tracers runs after lfa_time_step number n with the same dt and does what simulation::time_step does to a particle:
//  1. move     (_advect_particles, src/simulation.cpp:240-248): x += v dt, clamped to [grid_offset + skin, cell_size n + grid_offset
//              - skin], the corners computed as the reference computes them (on the host, once per call).
//  2. collide  (_detect_collisions, :612-683, with grid::march_cells, include/fluid/data_structures/grid.h:140-209): from = the
//              position before the move; up to three bounces; the march runs over (from - grid_offset) / cell_size and
//              (to - grid_offset) / cell_size, the bounce update is in WORLD units (t += skin / dot(offset, normal), t = max(t, 0),
//              from = t to + (1 - t) from, to[dim] = from[dim]); then the skin push-out of :654-681.
//  3. transfer (_transfer_from_grid_pic, :447-461): velocity = sample_classify + sample_value (sample.h) at the new position, and
//              the cell type with it.
// 1 and 2 read the stored velocity and the solid cells, 3 the grid the step's G2P read: the result is what a placement inside the
// step would give. All fp64, + - * /, floor, fabs and comparisons in the reference's order, no contraction: bit for bit the oracle's
// advect, detect_collisions and PIC transfer. NOT collide() of particles.hip: that one works in grid units from fp32 fractions.
//
// Two deliberate differences, invisible on finite inputs:
//  * the march of a bounce takes at most nx + ny + nz + 3 face crossings (a segment between two points of the clamped box cannot
//    cross more): the loop's end does not depend on its input.
//  * a tracer whose moved position x + v dt is not finite in every coordinate (a NaN velocity, which a poisoned grid yields) does
//    not move: it is counted as frozen, keeps its position, and still takes a new velocity in 3.
// The open-water short cut of particles.hip (tile_clear) is not used: every tracer marches and every tracer's push-out is evaluated.
//
// One lane per tracer, SoA. tracer_move_collide and tracer_transfer are the ONE statement of the arithmetic; k_tracer_step (fused),
// k_tracer_advect_collide and k_tracer_transfer are instantiations of one body, so the fused form and the stages agree bit for bit.
// The fi of the new position serves the push-out's end cell and sample_value alike. Counts: one ballot and one atomic add per wave
// (integers: their order does not matter); no atomic decides a result.
#include <math.h>

#include <algorithm>
#include <utility>

#include "sample.h"

namespace {

struct TracerParams {
	SampleParams q;
	double dt, skin;
	double lo[3], hi[3];  // the clamp's corners (src/simulation.cpp:242-243)
	int max_cross;        // face crossings per bounce
};

struct TracerArrays {
	double *x[3], *v[3];
	uint32_t *counts;  // [0] stopped in the march, [1] frozen
	uint8_t *type;
};

__device__ inline bool tracer_solid_or_outside(const GridDims &g, const uint8_t *solid, int x, int y, int z) {
	if (!in_grid(g, x, y, z)) return true;
	return solid[blocked_index(g, x, y, z)] != 0;
}

/// Steps 1 and 2 for one tracer at x with velocity v. Returns the new position in `to` and its fi = (to - grid_offset) / cell_size
/// with `inside` as sample_classify states them. stopped: a march met a solid cell or a wall; frozen: x + v dt is not finite.
__device__ inline void tracer_move_collide(const GridDims &g, const uint8_t *solid, const TracerParams &P, const double (&x)[3], const double (&v)[3],
                                           double (&to)[3], double (&fi)[3], bool &inside, bool &stopped, bool &frozen) {
	const double h = P.q.ip.h, skin = P.skin;
	double from[3];
	stopped = false;
	frozen = false;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		from[d] = x[d];
		to[d] = x[d] + v[d] * P.dt;
		frozen = frozen || !(fabs(to[d]) < INFINITY);
	}
	if (frozen) {
#pragma unroll
		for (int d = 0; d < 3; ++d) to[d] = x[d];
		inside = sample_classify(to, 0, P.q, fi);
		return;
	}
#pragma unroll
	for (int d = 0; d < 3; ++d) to[d] = to[d] < P.lo[d] ? P.lo[d] : (P.hi[d] < to[d] ? P.hi[d] : to[d]);  // std::clamp(v, lo, hi)
	for (int bounce = 0; bounce < 3; ++bounce) {
		bool hit = false;
		double diff[3], inv[3], t[3];
		int cur[3], last[3], adv[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			const double a = (from[d] - P.q.ip.off[d]) / h, b = (to[d] - P.q.ip.off[d]) / h;
			cur[d] = (int)floor(a);
			last[d] = (int)floor(b);
			diff[d] = b - a;
			adv[d] = diff[d] > 0.0 ? 1 : -1;
			inv[d] = 1.0 / fabs(diff[d]);
			t[d] = fabs((double)(cur[d] + (diff[d] > 0.0 ? 1 : 0)) - a) * inv[d];
		}
		for (int guard = 0; guard < P.max_cross && (cur[0] != last[0] || cur[1] != last[1] || cur[2] != last[2]); ++guard) {
			int dim = 0;
			double tmin = 2.0;
			if (t[0] < tmin) { tmin = t[0]; dim = 0; }
			if (t[1] < tmin) { tmin = t[1]; dim = 1; }
			if (t[2] < tmin) { tmin = t[2]; dim = 2; }
			if (!(tmin <= 1.0)) break;  // grid.h:196-199
			// static indexing (no scratch): update the chosen axis
			const int a0 = dim == 0, a1 = dim == 1, a2 = dim == 2;
			cur[0] += a0 ? adv[0] : 0; cur[1] += a1 ? adv[1] : 0; cur[2] += a2 ? adv[2] : 0;
			if (tracer_solid_or_outside(g, solid, cur[0], cur[1], cur[2])) {
				const double td = a0 ? t[0] : (a1 ? t[1] : t[2]);
				const double od = a0 ? to[0] - from[0] : (a1 ? to[1] - from[1] : to[2] - from[2]);  // offset = to - from, world units
				const int ad = a0 ? adv[0] : (a1 ? adv[1] : adv[2]);
				double tt = td + skin / (od * (double)(-ad));  // normal = -advance on `dim`
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
		stopped = true;
	}
	// the skin of neighbouring solid cells and walls (:654-681): grid_pos / cell_size is the fi of sample_classify
	inside = sample_classify(to, 0, P.q, fi);
	const int n[3] = {g.nx, g.ny, g.nz};
	const double skin_max = h - skin;
	int ci[3];
	double cp[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		ci[d] = fi[d] >= 0.0 ? (int)fi[d] : 0;  // (to lies in the clamped box: never negative; the reference casts to size_t)
		cp[d] = (to[d] - P.q.ip.off[d]) - (double)ci[d] * h;
	}
	bool pushed = false;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		if (cp[d] < skin) {
			if (ci[d] == 0 || tracer_solid_or_outside(g, solid, ci[0] - (d == 0), ci[1] - (d == 1), ci[2] - (d == 2))) {
				to[d] += skin - cp[d];
				pushed = true;
			}
		}
		if (cp[d] > skin_max) {
			if (ci[d] + 1 >= n[d] || tracer_solid_or_outside(g, solid, ci[0] + (d == 0), ci[1] + (d == 1), ci[2] + (d == 2))) {
				to[d] += skin_max - cp[d];
				pushed = true;
			}
		}
	}
	if (pushed) inside = sample_classify(to, 0, P.q, fi);
}

/// Step 3 for a tracer whose position has the fi and `inside` of sample_classify: outside the grid (+0, +0, +0) and type 0, as
/// lfa_sample_velocity answers. SLAB: the view carries the owners' tile rules (lfa_sample_refresh), as in sample.hip.
template <bool SLAB>
__device__ inline void tracer_transfer(const GridDims &g, const CellView &cv, const double (&fi)[3], bool inside, double (&vel)[3], uint8_t &type) {
	vel[0] = vel[1] = vel[2] = 0.0;
	type = 0;
	if (inside) sample_value<SLAB>(g, cv, fi, vel, type);
}

/// MOVE: steps 1 and 2, TRANSFER: step 3; both: the fused step. SLAB: see tracer_transfer.
template <bool MOVE, bool TRANSFER, bool SLAB = false>
__device__ inline void tracer_pass(const TracerArrays &tr, size_t n, const GridDims &g, const uint8_t *solid, const TracerParams &P, const CellView &cv) {
	const int lane = threadIdx.x & 63;
	uint32_t stopped_wave = 0, frozen_wave = 0;  // (the same numbers in every lane of the wave)
	// the whole wave walks the loop together: the ballots below need every lane
	for (size_t base = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (size_t)gridDim.x * 256) {
		const size_t i = base + lane;
		const bool live = i < n;
		double x[3] = {0.0, 0.0, 0.0}, fi[3] = {0.0, 0.0, 0.0};
		bool inside = false, stopped = false, frozen = false;
		if (live) {
#pragma unroll
			for (int d = 0; d < 3; ++d) x[d] = tr.x[d][i];
			if (MOVE) {
				double v[3], to[3];
#pragma unroll
				for (int d = 0; d < 3; ++d) v[d] = tr.v[d][i];
				tracer_move_collide(g, solid, P, x, v, to, fi, inside, stopped, frozen);
#pragma unroll
				for (int d = 0; d < 3; ++d) tr.x[d][i] = to[d];
			} else {
				inside = sample_classify(x, 0, P.q, fi);
			}
		}
		if (MOVE) {
			stopped_wave += (uint32_t)__popcll(__ballot(stopped));
			frozen_wave += (uint32_t)__popcll(__ballot(frozen));
		}
		if (TRANSFER && live) {
			double vel[3];
			uint8_t type;
			tracer_transfer<SLAB>(g, cv, fi, inside, vel, type);
#pragma unroll
			for (int d = 0; d < 3; ++d) tr.v[d][i] = vel[d];
			tr.type[i] = type;
		}
	}
	if (MOVE) {  // integer adds: the totals do not depend on their order
		if (lane == 0 && stopped_wave) atomicAdd(tr.counts, stopped_wave);
		if (lane == 0 && frozen_wave) atomicAdd(tr.counts + 1, frozen_wave);
	}
}

__global__ void __launch_bounds__(256) k_tracer_step(TracerArrays tr, size_t n, GridDims g, const uint8_t *solid, TracerParams P, CellView cv) {
	tracer_pass<true, true>(tr, n, g, solid, P, cv);
}
__global__ void __launch_bounds__(256) k_tracer_advect_collide(TracerArrays tr, size_t n, GridDims g, const uint8_t *solid, TracerParams P, CellView cv) {
	tracer_pass<true, false>(tr, n, g, solid, P, cv);
}
__global__ void __launch_bounds__(256) k_tracer_transfer(TracerArrays tr, size_t n, GridDims g, const uint8_t *solid, TracerParams P, CellView cv) {
	tracer_pass<false, true>(tr, n, g, solid, P, cv);
}
/// The transfer on a slab decomposition: the tracers a rank holds lie in its own layers, their sample blocks reach into the ghost
/// layers, which answer like their owners after lfa_sample_refresh.
__global__ void __launch_bounds__(256) k_tracer_transfer_slab(TracerArrays tr, size_t n, GridDims g, const uint8_t *solid, TracerParams P, CellView cv) {
	tracer_pass<false, true, true>(tr, n, g, solid, P, cv);
}

/// AoS rows of the caller -> the SoA arrays from `at` on; vel null: zeros. The type of a tracer is 0 until its first transfer.
__global__ void __launch_bounds__(256) k_tracer_append(TracerArrays tr, size_t at, const double *xyz, const double *vel, size_t n) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		tr.x[d][at + i] = xyz[3 * i + d];
		tr.v[d][at + i] = vel ? vel[3 * i + d] : 0.0;
	}
	tr.type[at + i] = 0;
}
/// The SoA arrays -> AoS rows (either may be null).
__global__ void __launch_bounds__(256) k_tracer_export(TracerArrays tr, size_t n, double *xyz, double *vel) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		if (xyz) xyz[3 * i + d] = tr.x[d][i];
		if (vel) vel[3 * i + d] = tr.v[d][i];
	}
}

// ---------------------------------------------------------------------------------------------------- slabs: owner and records
// A job of N ranks holds a partition of the single domain's tracers: a tracer lives on the rank whose tile layers hold its cell
// layer, carries its job-wide id, and changes ranks when a move takes it across a slab face - hop by hop through z-1 / z+1, as many
// rounds as the farthest mover of the job needs. Placement follows k_sample_count / k_sample_write: a ballot per 64 consecutive
// records, a scan of the per-chunk counts, the record at offset + popcount(below). No atomic decides a position.

/// The tile layer that owns a position: cz = floor((z - grid_offset_z) / cell_size) with the division of sample_classify, clamped to
/// [0, nz - 1] ON THE DOUBLE, before any cast (1e300 never reaches a conversion; a NaN, which no stored position is, gives 0); >> 3.
__device__ inline int tracer_owner_layer(double z, const SampleParams &q) {
	double c = floor((z - q.ip.off[2]) / q.ip.h);
	const double top = q.n[2] - 1.0;
	c = !(c >= 0.0) ? 0.0 : (top < c ? top : c);
	return (int)c >> 3;
}

/// Pass 1 over z[zs i], i < n, on the rank of the layers [lo, hi): per chunk of 64 the records whose owner lies below, above, here.
/// span (zeroed by the caller): [0] ntz - the lowest, [1] 1 + the highest destination layer of the records that leave, 0: none
/// (integer maxima: their order does not matter).
__global__ void __launch_bounds__(256) k_tracer_slab_count(const double *z, size_t zs, size_t n, SampleParams q, int lo, int hi, int ntz,
                                                           uint32_t *down, uint32_t *up, uint32_t *stay, int *span) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool live = i < n;
	const int layer = live ? tracer_owner_layer(z[zs * i], q) : lo;
	const bool dn = live && layer < lo, ab = live && layer >= hi;
	const unsigned long long md = __ballot(dn), ma = __ballot(ab), ml = __ballot(live);
	const int lowest = wave_max(dn ? ntz - layer : 0), highest = wave_max(ab ? layer + 1 : 0);
	if ((threadIdx.x & 63) != 0 || !live) return;
	down[i >> 6] = (uint32_t)__popcll(md);
	up[i >> 6] = (uint32_t)__popcll(ma);
	stay[i >> 6] = (uint32_t)__popcll(ml & ~md & ~ma);
	if (lowest) atomicMax(span, lowest);
	if (highest) atomicMax(span + 1, highest);
}

/// The record on the wire, 56 bytes: x, y, z, vx, vy, vz, then id (low word) and type (the byte above it) in the seventh.
__device__ inline void tracer_record_store(double *rec, const double (&x)[3], const double (&v)[3], uint32_t id, uint8_t type) {
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		rec[d] = x[d];
		rec[3 + d] = v[d];
	}
	((unsigned long long *)rec)[6] = (unsigned long long)id | ((unsigned long long)type << 32);
}

/// Pass 2 of a migration round: the classification again; a stayer becomes record stay[chunk] + its rank among the chunk's stayers
/// of `dst` (the other block: stayers in their previous order, compact), a leaver a record of the buffer of its side.
__global__ void __launch_bounds__(256) k_tracer_slab_write(TracerArrays src, const uint32_t *src_id, size_t n, SampleParams q, int lo, int hi,
                                                           const uint32_t *down, const uint32_t *up, const uint32_t *stay, size_t n_down, size_t n_up,
                                                           size_t n_stay, TracerArrays dst, uint32_t *dst_id, double *buf_lo, double *buf_hi) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool live = i < n;
	const int layer = live ? tracer_owner_layer(src.x[2][i], q) : lo;
	const bool dn = live && layer < lo, ab = live && layer >= hi;
	const unsigned long long md = __ballot(dn), ma = __ballot(ab), ml = __ballot(live);
	if (!live) return;
	const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
	double x[3], v[3];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		x[d] = src.x[d][i];
		v[d] = src.v[d][i];
	}
	const uint32_t id = src_id[i];
	const uint8_t type = src.type[i];
	// (j beyond its total cannot happen: both passes classify the same records; the test keeps every write inside its array regardless)
	if (dn || ab) {
		const size_t j = (size_t)(dn ? down : up)[i >> 6] + (size_t)__popcll((dn ? md : ma) & below);
		if (j < (dn ? n_down : n_up)) tracer_record_store((dn ? buf_lo : buf_hi) + 7 * j, x, v, id, type);
		return;
	}
	const size_t j = (size_t)stay[i >> 6] + (size_t)__popcll(ml & ~md & ~ma & below);
	if (j >= n_stay) return;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		dst.x[d][j] = x[d];
		dst.v[d][j] = v[d];
	}
	dst.type[j] = type;
	dst_id[j] = id;
}

/// n received records -> the arrays from `at` on, in the sender's order.
__global__ void __launch_bounds__(256) k_tracer_slab_unpack(const double *buf, size_t n, TracerArrays dst, uint32_t *dst_id, size_t at) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const double *rec = buf + 7 * i;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		dst.x[d][at + i] = rec[d];
		dst.v[d][at + i] = rec[3 + d];
	}
	const unsigned long long w = ((const unsigned long long *)rec)[6];
	dst_id[at + i] = (uint32_t)w;
	dst.type[at + i] = (uint8_t)(w >> 32);
}

/// lfa_tracers_add_collective, pass 2: the rows of the list this rank owns, appended from `at` on in list order, id = first_id + row.
__global__ void __launch_bounds__(256) k_tracer_slab_keep(const double *xyz, const double *vel, size_t n, SampleParams q, int lo, int hi,
                                                          const uint32_t *stay, size_t n_stay, TracerArrays dst, uint32_t *dst_id, size_t at,
                                                          uint32_t first_id) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool live = i < n;
	const int layer = live ? tracer_owner_layer(xyz[3 * i + 2], q) : lo - 1;
	const bool own = live && layer >= lo && layer < hi;
	const unsigned long long mo = __ballot(own);
	if (!own) return;
	const size_t j = (size_t)stay[i >> 6] + (size_t)__popcll(mo & ((1ull << (threadIdx.x & 63)) - 1ull));
	if (j >= n_stay) return;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		dst.x[d][at + j] = xyz[3 * i + d];
		dst.v[d][at + j] = vel ? vel[3 * i + d] : 0.0;
	}
	dst.type[at + j] = 0;
	dst_id[at + j] = first_id + (uint32_t)i;
}

TracerArrays tracer_arrays(void *base, size_t cap) {
	TracerArrays tr;
	double *f = (double *)base;
	for (int d = 0; d < 3; ++d) {
		tr.x[d] = f + cap * d;
		tr.v[d] = f + cap * (3 + d);
	}
	tr.counts = (uint32_t *)(f + cap * 6);
	tr.type = (uint8_t *)(tr.counts + 2);
	return tr;
}
size_t tracer_bytes(size_t cap) { return cap * 48 + 8 + cap; }
/// The block of a slab handle: the same arrays, then the job-wide ids uint32[cap] (cap is a multiple of 1024: they are aligned).
size_t tracer_block_bytes(const lfa_sim *s, size_t cap) { return tracer_bytes(cap) + (s->dist ? cap * 4 : 0); }
uint32_t *tracer_ids(void *base, size_t cap) { return (uint32_t *)((char *)base + tracer_bytes(cap)); }
size_t tracer_cap_for(size_t have, size_t n) {
	size_t cap = have ? 2 * have : 1024;
	if (cap < n) cap = n;
	return (cap + 1023) & ~(size_t)1023;
}

/// Room for n tracers; the live ones keep their places. Everything new is allocated before anything old is released.
int tracers_reserve(lfa_sim *s, size_t n) {
	lfa_sim::Tracers &T = s->tracers;
	if (n <= T.cap) return LFA_OK;
	const size_t cap = tracer_cap_for(T.cap, n);
	void *nb = nullptr;
	if (hipMalloc(&nb, tracer_block_bytes(s, cap)) != hipSuccess) return lfa_fail(s, LFA_E_OOM, "hipMalloc of the tracer arrays (%zu tracers) failed", cap);
	if (T.n) {
		const TracerArrays o = tracer_arrays(T.base, T.cap), w = tracer_arrays(nb, cap);
		hipError_t e = hipSuccess;
		for (int d = 0; d < 3 && e == hipSuccess; ++d) {
			e = hipMemcpyAsync(w.x[d], o.x[d], T.n * 8, hipMemcpyDeviceToDevice, s->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(w.v[d], o.v[d], T.n * 8, hipMemcpyDeviceToDevice, s->stream);
		}
		if (e == hipSuccess) e = hipMemcpyAsync(w.type, o.type, T.n, hipMemcpyDeviceToDevice, s->stream);
		if (e == hipSuccess && s->dist)
			e = hipMemcpyAsync(tracer_ids(nb, cap), tracer_ids(T.base, T.cap), T.n * 4, hipMemcpyDeviceToDevice, s->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
		if (e != hipSuccess) {
			(void)hipFree(nb);
			return lfa_fail(s, LFA_E_HIP, "copying the tracers to their new arrays failed: %s", hipGetErrorString(e));
		}
	}
	if (T.base) LFA_HIP(s, hipFree(T.base));
	T.base = nb;
	T.cap = cap;
	return LFA_OK;
}

/// The second block of a slab handle, for n tracers; nothing in it is kept.
int tracers_reserve_alt(lfa_sim *s, size_t n) {
	lfa_sim::Tracers &T = s->tracers;
	if (n <= T.alt_cap) return LFA_OK;
	const size_t cap = tracer_cap_for(T.alt_cap, n);
	void *nb = nullptr;
	if (hipMalloc(&nb, tracer_block_bytes(s, cap)) != hipSuccess) return lfa_fail(s, LFA_E_OOM, "hipMalloc of the tracer arrays (%zu tracers) failed", cap);
	if (T.alt) LFA_HIP(s, hipFree(T.alt));
	T.alt = nb;
	T.alt_cap = cap;
	return LFA_OK;
}

enum { TR_STEP = 0, TR_ADVECT_COLLIDE = 1, TR_TRANSFER = 2 };

/// tile_rule: null, or - the transfer on a slab decomposition - what lfa_sample_refresh returned.
int tracers_launch(lfa_sim *s, int which, double dt, const char *who, const uint32_t *tile_rule = nullptr) {
	lfa_sim::Tracers &T = s->tracers;
	if (which != TR_TRANSFER && !(fabs(dt) < INFINITY)) return lfa_fail(s, LFA_E_INVALID, "%s: dt is not finite", who);
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before %s", who);
	if (T.n == 0) return LFA_OK;
	LFA_HIP(s, hipSetDevice(s->device));
	TracerParams P;
	P.q = sample_params(s, 0, s->g.nz);
	P.dt = dt;
	P.skin = s->prm.boundary_skin_width;
	const int nn[3] = {s->g.nx, s->g.ny, s->g.nz};
	for (int d = 0; d < 3; ++d) {
		// min_corner = grid_offset + skin_width, max_corner = cell_size * vec3d(size) + grid_offset - skin_width
		P.lo[d] = P.q.ip.off[d] + P.skin;
		P.hi[d] = P.q.ip.h * (double)nn[d] + P.q.ip.off[d] - P.skin;
	}
	P.max_cross = s->g.nx + s->g.ny + s->g.nz + 3;
	const TracerArrays tr = tracer_arrays(T.base, T.cap);
	const CellView cv = sample_view(s, tile_rule);
	size_t blocks = (T.n + 255) / 256;
	if (blocks > SAMPLE_GRID_CAP) blocks = SAMPLE_GRID_CAP;
	for (hipEvent_t &e : T.ev)
		if (!e) LFA_HIP(s, hipEventCreate(&e));
	T.timed = false;
	if (which != TR_TRANSFER) LFA_HIP(s, hipMemsetAsync(tr.counts, 0, 8, s->stream));
	LFA_HIP(s, hipEventRecord(T.ev[0], s->stream));
	const dim3 grid((unsigned)blocks), block(256);
	if (which == TR_STEP)
		hipLaunchKernelGGL(k_tracer_step, grid, block, 0, s->stream, tr, T.n, s->g, (const uint8_t *)s->solid, P, cv);
	else if (which == TR_ADVECT_COLLIDE)
		hipLaunchKernelGGL(k_tracer_advect_collide, grid, block, 0, s->stream, tr, T.n, s->g, (const uint8_t *)s->solid, P, cv);
	else if (tile_rule)
		hipLaunchKernelGGL(k_tracer_transfer_slab, grid, block, 0, s->stream, tr, T.n, s->g, (const uint8_t *)s->solid, P, cv);
	else
		hipLaunchKernelGGL(k_tracer_transfer, grid, block, 0, s->stream, tr, T.n, s->g, (const uint8_t *)s->solid, P, cv);
	LFA_LAUNCH_CHECK(s);
	LFA_HIP(s, hipEventRecord(T.ev[1], s->stream));
	T.timed = true;
	return LFA_OK;
}

/// Reads the two count words of the last move through their pinned slot (one synchronisation of the stream).
int tracers_read_counts(lfa_sim *s, uint64_t *stopped, uint64_t *frozen) {
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + LFA_PIN_TRACER_COUNTS, tracer_arrays(s->tracers.base, s->tracers.cap).counts, 8, hipMemcpyDeviceToHost,
	                          s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	*stopped = s->h_pinned[LFA_PIN_TRACER_COUNTS];
	*frozen = s->h_pinned[LFA_PIN_TRACER_COUNTS + 1];
	return LFA_OK;
}

/// What the handle's state alone decides - the same on every rank of a collective call, so all fail here or none does, and no message
/// has been sent (sample.hip: sample_state_checks is the transfer's own, repeated inside lfa_sample_refresh).
int tracers_state_checks(lfa_sim *s, const char *who, bool moves, double dt, bool transfers) {
	if (moves && !(fabs(dt) < INFINITY)) return lfa_fail(s, LFA_E_INVALID, "%s: dt is not finite", who);
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before %s", who);
	if (transfers && s->dist && !s->binned)
		return lfa_fail(s, LFA_E_INVALID, "%s on a slab decomposition: call lfa_hash_particles (on every rank) first", who);
	return LFA_OK;
}

/// A step of a collective call fails on this rank alone after messages may have crossed: the peers must not wait for it.
int tracers_alone(lfa_sim *s, int rc) {
	if (rc != LFA_OK) s->dist->give_up();
	return rc;
}

/// The tracers this rank holds but does not own go to their owners, theirs come here. moved[0 .. 4): records handed down, handed up,
/// received (a forwarded record counts on every rank it passes), the rounds R of the job.
///  1. the lowest and the highest destination layer over the records that leave (k_tracer_slab_count), mapped to a hop distance
///     through the layer bounds of every rank; ONE max all-reduce makes it the job's R. R == 0: nothing crosses anywhere, done.
///  2. R rounds, each a count exchange and a payload exchange with z-1 / z+1. A round packs every record the rank holds and does not
///     own, the arrivals of the round before included, down or up by the owner's side; the stayers move compact and in order to the
///     front of the other block, the arrivals from below, then from above, follow in the senders' order, and the blocks change
///     places. A rank with no leaver in a round appends its arrivals in place.
int tracers_migrate(lfa_sim *s, uint64_t moved[4]) {
	lfa_sim::Tracers &T = s->tracers;
	const SampleParams q = sample_params(s, 0, s->g.nz);
	const bool has_lo = lfa_has_lo(s), has_hi = lfa_has_hi(s);
	const int rank = s->dist->rank;
	uint32_t *pin = s->h_pinned + LFA_PIN_TRACER_MIGRATE;
	moved[0] = moved[1] = moved[2] = moved[3] = 0;
	int rounds = 0;
	for (int round = 0; round == 0 || round < rounds; ++round) {
		// io buffer: the chunk words of the three kinds, each with its total behind | arriving from below, from above | the span
		const size_t n = T.n, nc = (n + 63) >> 6;
		LFA_TRY(tracers_alone(s, lfa_ensure_io(s, (3 * (nc + 1) + 4) * 4)));
		uint32_t *down = (uint32_t *)s->io_buf, *up = down + nc + 1, *stay = up + nc + 1, *arrive = stay + nc + 1;
		int *span = (int *)(arrive + 2);
		LFA_HIP(s, hipMemsetAsync(arrive, 0, 16, s->stream));
		if (n) {
			hipLaunchKernelGGL(k_tracer_slab_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
			                   (const double *)tracer_arrays(T.base, T.cap).x[2], (size_t)1, n, q, s->slab_lo, s->slab_hi, s->g.ntz, down, up, stay, span);
			LFA_LAUNCH_CHECK(s);
		}
		LFA_TRY(lfa_exclusive_scan_u32(s, down, down, nc, down + nc));
		LFA_TRY(lfa_exclusive_scan_u32(s, up, up, nc, up + nc));
		LFA_TRY(lfa_exclusive_scan_u32(s, stay, stay, nc, stay + nc));
		if (round == 0) {
			LFA_HIP(s, hipMemcpyAsync(pin + 5, span, 8, hipMemcpyDeviceToHost, s->stream));
			LFA_HIP(s, hipStreamSynchronize(s->stream));
			const int32_t *b = s->slab_bounds.data(), *e = b + s->slab_bounds.size();
			int hops = 0;
			if (pin[5]) hops = rank - (int)(std::upper_bound(b, e, (int32_t)(s->g.ntz - (int)pin[5])) - b - 1);
			if (pin[6]) hops = std::max(hops, (int)(std::upper_bound(b, e, (int32_t)(pin[6] - 1)) - b - 1) - rank);
			double *red = s->dist_red + LFA_DR_TRACER_ROUNDS, *host = (double *)(s->h_pinned + LFA_PIN_TRACER_ROUNDS);
			*host = (double)hops;
			LFA_HIP(s, hipMemcpyAsync(red + 1, host, 8, hipMemcpyHostToDevice, s->stream));
			LFA_TRY(lfa_dist_allreduce(s, red + 1, 1, LFA_DR_TRACER_ROUNDS, true));
			LFA_HIP(s, hipMemcpyAsync(host, red, 8, hipMemcpyDeviceToHost, s->stream));
			LFA_HIP(s, hipStreamSynchronize(s->stream));
			rounds = (int)*host;
			if (rounds <= 0) break;
		}
		// how many arrive: the neighbours' leave counts
		LFA_TRY(s->dist->exchange(s, has_lo ? down + nc : nullptr, has_lo ? 4 : 0, has_lo ? arrive : nullptr, has_lo ? 4 : 0, has_hi ? up + nc : nullptr,
		                          has_hi ? 4 : 0, has_hi ? arrive + 1 : nullptr, has_hi ? 4 : 0));
		LFA_HIP(s, hipMemcpyAsync(pin + 0, down + nc, 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipMemcpyAsync(pin + 1, up + nc, 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipMemcpyAsync(pin + 2, stay + nc, 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipMemcpyAsync(pin + 3, arrive, 8, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipStreamSynchronize(s->stream));
		// (the clamp keeps every layer inside the job's: nothing leaves through a domain wall)
		const size_t n_down = has_lo ? pin[0] : 0, n_up = has_hi ? pin[1] : 0, n_stay = n - n_down - n_up;
		const size_t from_lo = has_lo ? pin[3] : 0, from_hi = has_hi ? pin[4] : 0;
		if (n_stay != pin[2]) return tracers_alone(s, lfa_fail(s, LFA_E_HIP, "tracer migration: the two classifications of rank %d disagree", rank));
		const size_t bytes[4] = {n_down * 56, n_up * 56, from_lo * 56, from_hi * 56};
		for (int w = 0; w < 4; ++w) LFA_TRY(tracers_alone(s, lfa_dist_ensure_xbuf(s, w, bytes[w])));
		// everything new is allocated before anything old is released; a rank that cannot grow tells its peers
		const bool compact = n_down + n_up > 0;
		const size_t total = n_stay + from_lo + from_hi;
		LFA_TRY(tracers_alone(s, compact ? tracers_reserve_alt(s, total) : tracers_reserve(s, total)));
		void *dst_base = compact ? T.alt : T.base;
		const size_t dst_cap = compact ? T.alt_cap : T.cap;
		const TracerArrays dst = tracer_arrays(dst_base, dst_cap);
		uint32_t *dst_id = tracer_ids(dst_base, dst_cap);
		if (compact) {
			hipLaunchKernelGGL(k_tracer_slab_write, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, tracer_arrays(T.base, T.cap),
			                   (const uint32_t *)tracer_ids(T.base, T.cap), n, q, s->slab_lo, s->slab_hi, (const uint32_t *)down, (const uint32_t *)up,
			                   (const uint32_t *)stay, n_down, n_up, n_stay, dst, dst_id, (double *)s->xbuf[0], (double *)s->xbuf[1]);
			LFA_LAUNCH_CHECK(s);
		}
		LFA_TRY(s->dist->exchange(s, s->xbuf[0], bytes[0], s->xbuf[2], bytes[2], s->xbuf[1], bytes[1], s->xbuf[3], bytes[3]));
		size_t at = n_stay;
		for (int w = 2; w < 4; ++w) {
			const size_t m = w == 2 ? from_lo : from_hi;
			if (!m) continue;
			hipLaunchKernelGGL(k_tracer_slab_unpack, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s->stream, (const double *)s->xbuf[w], m, dst, dst_id, at);
			LFA_LAUNCH_CHECK(s);
			at += m;
		}
		if (compact) {
			std::swap(T.base, T.alt);
			std::swap(T.cap, T.alt_cap);
		}
		T.n = total;
		moved[0] += n_down;
		moved[1] += n_up;
		moved[2] += from_lo + from_hi;
	}
	moved[3] = (uint64_t)(rounds > 0 ? rounds : 0);
	return LFA_OK;
}

/// lfa_tracers_advect_collide_collective behind its state checks. counts: the six of the header, or NULL.
int tracers_move_collective(lfa_sim *s, double dt, const char *who, uint64_t *counts) {
	lfa_sim::Tracers &T = s->tracers;
	uint64_t c[6] = {0, 0, 0, 0, 0, 0};
	if (!s->dist) {
		LFA_TRY(tracers_launch(s, TR_ADVECT_COLLIDE, dt, who));
		if (counts && T.n) LFA_TRY(tracers_read_counts(s, &c[0], &c[1]));
	} else {
		LFA_TRY(tracers_alone(s, tracers_launch(s, TR_ADVECT_COLLIDE, dt, who)));
		if (T.n) LFA_TRY(tracers_alone(s, tracers_read_counts(s, &c[0], &c[1])));  // (of the tracers resident before the move)
		LFA_HIP(s, hipSetDevice(s->device));
		LFA_TRY(tracers_migrate(s, c + 2));
		if (T.timed) LFA_HIP(s, hipEventRecord(T.ev[1], s->stream));  // (lfa_tracers_time: the move and this rank's share of the migration)
	}
	if (counts)
		for (int k = 0; k < 6; ++k) counts[k] = c[k];
	return LFA_OK;
}

/// lfa_tracers_transfer_collective behind its state checks.
int tracers_transfer_collective(lfa_sim *s, const char *who) {
	if (!s->dist) return tracers_launch(s, TR_TRANSFER, 0.0, who);
	const uint32_t *rule = nullptr;
	void *room = nullptr;
	int z_lo, z_hi;
	LFA_TRY(lfa_sample_refresh(s, who, 0, &rule, &room, &z_lo, &z_hi));  // (a rank with no tracers too: the refresh is a collective)
	return tracers_launch(s, TR_TRANSFER, 0.0, who, rule);
}

}  // namespace

extern "C" int lfa_tracers_add(lfa_sim *s, const double *xyz, const double *velocity, uint64_t n) {
	if (!s) return LFA_E_INVALID;
	if (s->dist) return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_tracers_add: not on a slab decomposition (lfa_tracers_add_collective gives every tracer to the rank that owns it)");
	if (n == 0) return LFA_OK;
	if (!xyz) return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_add: xyz is NULL");
	lfa_sim::Tracers &T = s->tracers;
	if (n >= (1ull << 32) || T.n + n >= (1ull << 32)) return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_add: 2^32 tracers or more");
	for (uint64_t i = 0; i < 3 * n; ++i)
		if (!(fabs(xyz[i]) < INFINITY))
			return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_add: the position of tracer %llu of the call is not finite; nothing was added",
			                (unsigned long long)(i / 3));
	LFA_HIP(s, hipSetDevice(s->device));
	const size_t np = (size_t)n;
	LFA_TRY(tracers_reserve(s, T.n + np));
	LFA_TRY(lfa_ensure_io(s, np * 48));
	double *d_xyz = (double *)s->io_buf, *d_vel = velocity ? d_xyz + 3 * np : (double *)nullptr;
	LFA_HIP(s, hipMemcpyAsync(d_xyz, xyz, np * 24, hipMemcpyHostToDevice, s->stream));
	if (velocity) LFA_HIP(s, hipMemcpyAsync(d_vel, velocity, np * 24, hipMemcpyHostToDevice, s->stream));
	hipLaunchKernelGGL(k_tracer_append, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s->stream, tracer_arrays(T.base, T.cap), T.n,
	                   (const double *)d_xyz, (const double *)d_vel, np);
	LFA_LAUNCH_CHECK(s);
	LFA_HIP(s, hipStreamSynchronize(s->stream));  // (the caller's arrays are free again on return)
	T.n += np;
	return LFA_OK;
}

extern "C" int lfa_tracers_add_collective(lfa_sim *s, const double *xyz, const double *velocity, uint64_t n, uint64_t counts[2]) {
	if (!s) return LFA_E_INVALID;
	lfa_sim::Tracers &T = s->tracers;
	const uint64_t first = s->dist ? T.first_id : (uint64_t)T.n;
	if (counts) {
		counts[0] = 0;
		counts[1] = first;
	}
	if (!s->dist) {  // every layer is the handle's own: the plain call
		LFA_TRY(lfa_tracers_add(s, xyz, velocity, n));
		if (counts) counts[0] = n;
		return LFA_OK;
	}
	// the host checks of lfa_tracers_add: the list is the same on every rank, so all fail here or none does
	if (n == 0) return LFA_OK;
	if (!xyz) return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_add_collective: xyz is NULL");
	if (n >= (1ull << 32) || first + n >= (1ull << 32))
		return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_add_collective: 2^32 tracers or more in the job");
	for (uint64_t i = 0; i < 3 * n; ++i)
		if (!(fabs(xyz[i]) < INFINITY))
			return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_add_collective: the position of tracer %llu of the call is not finite; nothing was added",
			                (unsigned long long)(i / 3));
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before lfa_tracers_add_collective: the owner of a tracer is its cell layer's");
	T.first_id = first + n;  // (on every rank alike, whatever it keeps)
	LFA_HIP(s, hipSetDevice(s->device));
	// io buffer: positions | velocities | the chunk words of the three kinds, each with its total behind | the span
	const size_t np = (size_t)n, nc = (np + 63) >> 6;
	LFA_TRY(lfa_ensure_io(s, np * 48 + (3 * (nc + 1) + 2) * 4));
	double *d_xyz = (double *)s->io_buf, *d_vel = d_xyz + 3 * np;
	uint32_t *stay = (uint32_t *)(d_vel + 3 * np), *down = stay + nc + 1, *up = down + nc + 1;
	int *span = (int *)(up + nc + 1);
	const SampleParams q = sample_params(s, 0, s->g.nz);
	const dim3 grid((unsigned)((np + 255) / 256));
	LFA_HIP(s, hipMemcpyAsync(d_xyz, xyz, np * 24, hipMemcpyHostToDevice, s->stream));
	if (velocity) LFA_HIP(s, hipMemcpyAsync(d_vel, velocity, np * 24, hipMemcpyHostToDevice, s->stream));
	LFA_HIP(s, hipMemsetAsync(span, 0, 8, s->stream));
	hipLaunchKernelGGL(k_tracer_slab_count, grid, dim3(256), 0, s->stream, (const double *)d_xyz + 2, (size_t)3, np, q, s->slab_lo, s->slab_hi, s->g.ntz,
	                   down, up, stay, span);
	LFA_LAUNCH_CHECK(s);
	size_t kept = 0;
	LFA_TRY(lfa_scan_total(s, stay, stay, nc, stay + nc, LFA_PIN_TRACER_KEPT, &kept));
	if (counts) counts[0] = kept;
	if (kept == 0) return LFA_OK;
	LFA_TRY(tracers_reserve(s, T.n + kept));
	hipLaunchKernelGGL(k_tracer_slab_keep, grid, dim3(256), 0, s->stream, (const double *)d_xyz, velocity ? (const double *)d_vel : (const double *)nullptr,
	                   np, q, s->slab_lo, s->slab_hi, (const uint32_t *)stay, kept, tracer_arrays(T.base, T.cap), tracer_ids(T.base, T.cap), T.n,
	                   (uint32_t)first);
	LFA_LAUNCH_CHECK(s);
	LFA_HIP(s, hipStreamSynchronize(s->stream));  // (the caller's arrays are free again on return)
	T.n += kept;
	return LFA_OK;
}

extern "C" int lfa_tracers_clear(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	s->tracers.n = 0;  // (the arrays stay for the next lfa_tracers_add)
	s->tracers.first_id = 0;
	s->tracers.timed = false;
	return LFA_OK;
}

extern "C" int lfa_tracers_count(const lfa_sim *s, uint64_t *n) {
	if (!s || !n) return LFA_E_INVALID;
	*n = s->tracers.n;
	return LFA_OK;
}

/// The plain calls move and sample without a message: on a slab decomposition a tracer would stay with a rank that no longer owns it.
static int tracers_refuse_slabs(lfa_sim *s, const char *who) {
	if (!s->dist) return LFA_OK;
	return lfa_fail(s, LFA_E_UNSUPPORTED, "%s: not on a slab decomposition (%s_collective migrates the tracers and refreshes the ghost layers)", who, who);
}

extern "C" int lfa_tracers_advect_collide(lfa_sim *s, double dt) {
	if (!s) return LFA_E_INVALID;
	LFA_TRY(tracers_refuse_slabs(s, "lfa_tracers_advect_collide"));
	return tracers_launch(s, TR_ADVECT_COLLIDE, dt, "lfa_tracers_advect_collide");
}

extern "C" int lfa_tracers_transfer(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	LFA_TRY(tracers_refuse_slabs(s, "lfa_tracers_transfer"));
	return tracers_launch(s, TR_TRANSFER, 0.0, "lfa_tracers_transfer");
}

extern "C" int lfa_tracers_step(lfa_sim *s, double dt, uint64_t counts[2]) {
	if (!s) return LFA_E_INVALID;
	LFA_TRY(tracers_refuse_slabs(s, "lfa_tracers_step"));
	if (counts) counts[0] = counts[1] = 0;
	LFA_TRY(tracers_launch(s, TR_STEP, dt, "lfa_tracers_step"));
	if (!counts || s->tracers.n == 0) return LFA_OK;
	return tracers_read_counts(s, &counts[0], &counts[1]);
}

extern "C" int lfa_tracers_advect_collide_collective(lfa_sim *s, double dt, uint64_t counts[6]) {
	if (!s) return LFA_E_INVALID;
	if (counts)
		for (int k = 0; k < 6; ++k) counts[k] = 0;
	LFA_TRY(tracers_state_checks(s, "lfa_tracers_advect_collide_collective", true, dt, false));
	return tracers_move_collective(s, dt, "lfa_tracers_advect_collide_collective", counts);
}

extern "C" int lfa_tracers_transfer_collective(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	LFA_TRY(tracers_state_checks(s, "lfa_tracers_transfer_collective", false, 0.0, true));
	return tracers_transfer_collective(s, "lfa_tracers_transfer_collective");
}

extern "C" int lfa_tracers_step_collective(lfa_sim *s, double dt, uint64_t counts[6]) {
	if (!s) return LFA_E_INVALID;
	if (counts)
		for (int k = 0; k < 6; ++k) counts[k] = 0;
	// the state checks of BOTH stages first: a refusal of the transfer must not follow the migration's messages
	LFA_TRY(tracers_state_checks(s, "lfa_tracers_step_collective", true, dt, true));
	if (!s->dist) {  // one kernel, as lfa_tracers_step
		LFA_TRY(tracers_launch(s, TR_STEP, dt, "lfa_tracers_step_collective"));
		if (counts && s->tracers.n) LFA_TRY(tracers_read_counts(s, &counts[0], &counts[1]));
		return LFA_OK;
	}
	LFA_TRY(tracers_move_collective(s, dt, "lfa_tracers_step_collective", counts));
	return tracers_transfer_collective(s, "lfa_tracers_step_collective");
}

extern "C" int lfa_tracers_download_ids(lfa_sim *s, uint32_t *ids, double *xyz, double *velocity, uint8_t *types, uint64_t n) {
	if (!s) return LFA_E_INVALID;
	const lfa_sim::Tracers &T = s->tracers;
	if (n != T.n) return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_download_ids: n = %llu but the handle holds %zu tracers", (unsigned long long)n, T.n);
	if (n == 0) return LFA_OK;
	if (ids && !s->dist) {
		for (uint64_t i = 0; i < n; ++i) ids[i] = (uint32_t)i;  // a single domain stores none: a tracer's id is its index
	} else if (ids) {
		LFA_HIP(s, hipSetDevice(s->device));
		LFA_HIP(s, hipMemcpyAsync(ids, tracer_ids(T.base, T.cap), (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipStreamSynchronize(s->stream));
	}
	return lfa_tracers_download(s, xyz, velocity, types, n);
}

extern "C" int lfa_tracers_download(lfa_sim *s, double *xyz, double *velocity, uint8_t *types, uint64_t n) {
	if (!s) return LFA_E_INVALID;
	const lfa_sim::Tracers &T = s->tracers;
	if (n != T.n) return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_download: n = %llu but the handle holds %zu tracers", (unsigned long long)n, T.n);
	if (n == 0 || (!xyz && !velocity && !types)) return LFA_OK;
	LFA_HIP(s, hipSetDevice(s->device));
	const size_t np = (size_t)n;
	const TracerArrays tr = tracer_arrays(T.base, T.cap);
	if (xyz || velocity) {
		LFA_TRY(lfa_ensure_io(s, np * 48));
		double *d_xyz = xyz ? (double *)s->io_buf : (double *)nullptr, *d_vel = velocity ? (double *)s->io_buf + 3 * np : (double *)nullptr;
		hipLaunchKernelGGL(k_tracer_export, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s->stream, tr, np, d_xyz, d_vel);
		LFA_LAUNCH_CHECK(s);
		if (xyz) LFA_HIP(s, hipMemcpyAsync(xyz, d_xyz, np * 24, hipMemcpyDeviceToHost, s->stream));
		if (velocity) LFA_HIP(s, hipMemcpyAsync(velocity, d_vel, np * 24, hipMemcpyDeviceToHost, s->stream));
	}
	if (types) LFA_HIP(s, hipMemcpyAsync(types, tr.type, np, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	return LFA_OK;
}

extern "C" int lfa_tracers_time(lfa_sim *s, double *ms) {
	if (!s || !ms) return LFA_E_INVALID;
	if (!s->tracers.timed) return lfa_fail(s, LFA_E_INVALID, "lfa_tracers_time: no tracer kernel has run since the last lfa_tracers_clear");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_HIP(s, hipEventSynchronize(s->tracers.ev[1]));
	float f = 0.0f;
	LFA_HIP(s, hipEventElapsedTime(&f, s->tracers.ev[0], s->tracers.ev[1]));
	*ms = (double)f;
	return LFA_OK;
}
