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
/// lfa_sample_velocity answers.
__device__ inline void tracer_transfer(const GridDims &g, const CellView &cv, const double (&fi)[3], bool inside, double (&vel)[3], uint8_t &type) {
	vel[0] = vel[1] = vel[2] = 0.0;
	type = 0;
	if (inside) sample_value<false>(g, cv, fi, vel, type);
}

/// MOVE: steps 1 and 2, TRANSFER: step 3; both: the fused step.
template <bool MOVE, bool TRANSFER>
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
			tracer_transfer(g, cv, fi, inside, vel, type);
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

/// Room for n tracers; the live ones keep their places. Everything new is allocated before anything old is released.
int tracers_reserve(lfa_sim *s, size_t n) {
	lfa_sim::Tracers &T = s->tracers;
	if (n <= T.cap) return LFA_OK;
	size_t cap = T.cap ? 2 * T.cap : 1024;
	if (cap < n) cap = n;
	cap = (cap + 1023) & ~(size_t)1023;
	void *nb = nullptr;
	if (hipMalloc(&nb, tracer_bytes(cap)) != hipSuccess) return lfa_fail(s, LFA_E_OOM, "hipMalloc of the tracer arrays (%zu tracers) failed", cap);
	if (T.n) {
		const TracerArrays o = tracer_arrays(T.base, T.cap), w = tracer_arrays(nb, cap);
		hipError_t e = hipSuccess;
		for (int d = 0; d < 3 && e == hipSuccess; ++d) {
			e = hipMemcpyAsync(w.x[d], o.x[d], T.n * 8, hipMemcpyDeviceToDevice, s->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(w.v[d], o.v[d], T.n * 8, hipMemcpyDeviceToDevice, s->stream);
		}
		if (e == hipSuccess) e = hipMemcpyAsync(w.type, o.type, T.n, hipMemcpyDeviceToDevice, s->stream);
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

enum { TR_STEP = 0, TR_ADVECT_COLLIDE = 1, TR_TRANSFER = 2 };

int tracers_launch(lfa_sim *s, int which, double dt, const char *who) {
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
	const CellView cv = sample_view(s, nullptr);
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
	else
		hipLaunchKernelGGL(k_tracer_transfer, grid, block, 0, s->stream, tr, T.n, s->g, (const uint8_t *)s->solid, P, cv);
	LFA_LAUNCH_CHECK(s);
	LFA_HIP(s, hipEventRecord(T.ev[1], s->stream));
	T.timed = true;
	return LFA_OK;
}

}  // namespace

extern "C" int lfa_tracers_add(lfa_sim *s, const double *xyz, const double *velocity, uint64_t n) {
	if (!s) return LFA_E_INVALID;
	if (s->dist) return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_tracers_add: not on a slab decomposition (tracers do not migrate between ranks yet)");
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

extern "C" int lfa_tracers_clear(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	s->tracers.n = 0;  // (the arrays stay for the next lfa_tracers_add)
	s->tracers.timed = false;
	return LFA_OK;
}

extern "C" int lfa_tracers_count(const lfa_sim *s, uint64_t *n) {
	if (!s || !n) return LFA_E_INVALID;
	*n = s->tracers.n;
	return LFA_OK;
}

extern "C" int lfa_tracers_advect_collide(lfa_sim *s, double dt) {
	if (!s) return LFA_E_INVALID;
	return tracers_launch(s, TR_ADVECT_COLLIDE, dt, "lfa_tracers_advect_collide");
}

extern "C" int lfa_tracers_transfer(lfa_sim *s) {
	if (!s) return LFA_E_INVALID;
	return tracers_launch(s, TR_TRANSFER, 0.0, "lfa_tracers_transfer");
}

extern "C" int lfa_tracers_step(lfa_sim *s, double dt, uint64_t counts[2]) {
	if (!s) return LFA_E_INVALID;
	if (counts) counts[0] = counts[1] = 0;
	LFA_TRY(tracers_launch(s, TR_STEP, dt, "lfa_tracers_step"));
	if (!counts || s->tracers.n == 0) return LFA_OK;
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + LFA_PIN_TRACER_COUNTS, tracer_arrays(s->tracers.base, s->tracers.cap).counts, 8, hipMemcpyDeviceToHost,
	                          s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	counts[0] = s->h_pinned[LFA_PIN_TRACER_COUNTS];
	counts[1] = s->h_pinned[LFA_PIN_TRACER_COUNTS + 1];
	return LFA_OK;
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
