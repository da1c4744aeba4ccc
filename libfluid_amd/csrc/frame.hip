// libfluid_amd/csrc/frame.hip -- what the hosts read from the particles after every step, computed where the particles are.
//
// The testbed's update_simulation (testbed/main.cpp:50-88) copies every particle, sums 0.5 |v|^2 - g . x into its "total energy"
// and counts particles per cell into an occupation grid; its post_grid_to_particle_transfer_callback (:117-123) takes the largest
// |v|^2; the Maya GridNode copies every position into its frame cache (plugins/maya/nodes/grid_node.cpp:356-364). Through
// lfa_download_particles that is 152 bytes per particle up and 152 down. Here: one pass over key, t and v (28 bytes per particle)
// that leaves three scalars, a bounding box and the integer grid, and a narrow unpack of the positions (24 bytes per particle, one way).
//
// Arithmetic: the world position is particle_world_position (common.h), the function a download uses, so every per-particle term
// is the one the caller's loop forms from an LFA_DL_POSITIONS download: sq = vx vx; sq += vy vy; sq += vz vz (squared_length),
// dot = gx x; dot += gy y; dot += gz z, term = 0.5 sq - dot, all fp64, no contraction. The occupation cell is the caller's
// (int)((x - off) / h) with a true division - NOT the cell of the key: off + c h, divided by h again, often lands one cell lower.
//
// Order: maximum, box, counts and the grid (integer atomics) do not depend on it. The two sums are reproducible: a thread adds its
// particles in index order, a wave reduces by shuffles, a workgroup adds its waves' sums in wave order and writes ONE partial into
// its own slot; a single workgroup then adds the slots in the same fixed way. The number of workgroups follows from the number of
// records alone, so two calls on the same resident state - on any box - return the same bits. No floating-point atomics.
#include "common.h"

#include <cmath>
#include <cstring>
#include <limits>

#define FRAME_GRID_CAP 1024  // workgroups of the pass; above 256 x FRAME_GRID_CAP records a thread walks several (grid-stride)
#define FRAME_FIELDS 11      // energy, energy_abs, max_speed2, lo[3], hi[3] | n, n_in_grid (the bits of two uint64)
#define FRAME_PART_DOUBLES ((FRAME_GRID_CAP + 1) * FRAME_FIELDS)  // [field][workgroup], then the reduced result

struct FrameAcc {
	double e, ea, m, lo[3], hi[3];
	unsigned long long n, nin;
};
__device__ inline FrameAcc frame_neutral() {
	FrameAcc a;
	a.e = a.ea = a.m = 0.0;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		a.lo[k] = INFINITY;
		a.hi[k] = -INFINITY;
	}
	a.n = a.nin = 0ull;
	return a;
}
__device__ inline void frame_merge(FrameAcc &a, const FrameAcc &b) {
	a.e += b.e;
	a.ea += b.ea;
	a.m = b.m > a.m ? b.m : a.m;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		a.lo[k] = b.lo[k] < a.lo[k] ? b.lo[k] : a.lo[k];
		a.hi[k] = b.hi[k] > a.hi[k] ? b.hi[k] : a.hi[k];
	}
	a.n += b.n;
	a.nin += b.nin;
}
__device__ inline FrameAcc frame_shfl_xor(const FrameAcc &a, int o) {
	FrameAcc b;
	b.e = __shfl_xor(a.e, o, 64);
	b.ea = __shfl_xor(a.ea, o, 64);
	b.m = __shfl_xor(a.m, o, 64);
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		b.lo[k] = __shfl_xor(a.lo[k], o, 64);
		b.hi[k] = __shfl_xor(a.hi[k], o, 64);
	}
	b.n = __shfl_xor(a.n, o, 64);
	b.nin = __shfl_xor(a.nin, o, 64);
	return b;
}
__device__ inline void frame_store(const FrameAcc &a, double *f, size_t stride) {
	f[0] = a.e;
	f[stride] = a.ea;
	f[2 * stride] = a.m;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		f[(3 + k) * stride] = a.lo[k];
		f[(6 + k) * stride] = a.hi[k];
	}
	f[9 * stride] = __longlong_as_double((long long)a.n);
	f[10 * stride] = __longlong_as_double((long long)a.nin);
}
__device__ inline FrameAcc frame_load(const double *f, size_t stride) {
	FrameAcc a;
	a.e = f[0];
	a.ea = f[stride];
	a.m = f[2 * stride];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		a.lo[k] = f[(3 + k) * stride];
		a.hi[k] = f[(6 + k) * stride];
	}
	a.n = (unsigned long long)__double_as_longlong(f[9 * stride]);
	a.nin = (unsigned long long)__double_as_longlong(f[10 * stride]);
	return a;
}

/// The 256 threads' accumulators -> thread 0's: shuffles inside a wave (every lane ends with the same sum: the two operands of a
/// butterfly step are the same pair in both lanes), then the four waves through LDS, in wave order.
__device__ inline void frame_block_reduce(FrameAcc &a) {
	__shared__ double lds[4][FRAME_FIELDS];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const FrameAcc b = frame_shfl_xor(a, o);
		frame_merge(a, b);
	}
	if ((threadIdx.x & 63) == 0) frame_store(a, lds[threadIdx.x >> 6], 1);
	__syncthreads();
	if (threadIdx.x == 0)
		for (int w = 1; w < 4; ++w) {
			const FrameAcc b = frame_load(lds[w], 1);
			frame_merge(a, b);
		}
}

struct FrameParams {
	IngestParams ip;
	double g[3];
};

/// The pass: records [0, n) of the current buffer (slabs: a record handed to a neighbour rank carries an invalid key and is no
/// particle of this rank). OCC: also count into occupation[nx ny nz], x fastest; n_in_grid is counted either way.
template <bool OCC>
__global__ void __launch_bounds__(256) k_frame_stats(size_t n, const PosRec *pos, const float *v0, const float *v1, const float *v2, GridDims g, FrameParams q,
                                                     uint32_t *occupation, double *part) {
	FrameAcc a = frame_neutral();
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
		const PosRec me = pos_load(pos, i);
		const uint32_t b = me.key;
		if (b == 0xFFFFFFFFu) continue;
		double x[3];
		particle_world_position(g, q.ip, b, me.t[0], me.t[1], me.t[2], x);
		const double vx = (double)v0[i], vy = (double)v1[i], vz = (double)v2[i];
		double sq = vx * vx;
		sq += vy * vy;
		sq += vz * vz;
		double dot = q.g[0] * x[0];
		dot += q.g[1] * x[1];
		dot += q.g[2] * x[2];
		const double half = 0.5 * sq;
		a.e += half - dot;
		a.ea += half + fabs(dot);
		a.m = sq > a.m ? sq : a.m;  // (a NaN compares false: skipped, like std::max(fastest, nan))
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			a.lo[k] = x[k] < a.lo[k] ? x[k] : a.lo[k];
			a.hi[k] = x[k] > a.hi[k] ? x[k] : a.hi[k];
		}
		++a.n;
		// vec3s(vec3i((position - grid_offset) / cell_size)): true division, truncation toward zero, a negative index is out
		const int ix = (int)((x[0] - q.ip.off[0]) / q.ip.h), iy = (int)((x[1] - q.ip.off[1]) / q.ip.h), iz = (int)((x[2] - q.ip.off[2]) / q.ip.h);
		if (in_grid(g, ix, iy, iz)) {
			++a.nin;
			if (OCC) atomicAdd(&occupation[(size_t)ix + (size_t)g.nx * ((size_t)iy + (size_t)g.ny * (size_t)iz)], 1u);
		}
	}
	frame_block_reduce(a);
	if (threadIdx.x == 0) frame_store(a, part + blockIdx.x, FRAME_GRID_CAP);
}

/// The second level: one workgroup adds the n_part slots - thread j the slots j, j + 256, ... in ascending order - and leaves the
/// result behind the slots.
__global__ void __launch_bounds__(256) k_frame_finish(int n_part, double *part) {
	FrameAcc a = frame_neutral();
	for (int i = (int)threadIdx.x; i < n_part; i += 256) {
		const FrameAcc b = frame_load(part + i, FRAME_GRID_CAP);
		frame_merge(a, b);
	}
	frame_block_reduce(a);
	if (threadIdx.x == 0) frame_store(a, part + (size_t)FRAME_GRID_CAP * FRAME_FIELDS, 1);
}

/// double[3] per particle, in the order of a download: single domain by particle id, slabs by storage slot (holes closed).
__global__ void __launch_bounds__(256) k_export_positions(double *xyz, size_t n, size_t n_out, const PosRec *pos, const uint32_t *id, GridDims g, IngestParams ip,
                                                          int by_slot, const uint32_t *slot) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const PosRec me = pos_load(pos, i);
	const uint32_t b = me.key;
	if (b == 0xFFFFFFFFu) return;
	const size_t d = by_slot ? (slot ? (size_t)slot[i] : i) : (size_t)id[i];
	if (d >= n_out) return;  // (cannot happen: ids and slots are below the resident count; keeps the write inside the buffer regardless)
	double x[3];
	particle_world_position(g, ip, b, me.t[0], me.t[1], me.t[2], x);
#pragma unroll
	for (int k = 0; k < 3; ++k) xyz[3 * d + k] = x[k];
}

// ---------------------------------------------------------------------------------------------------- entry points
static void frame_neutral_host(struct lfa_frame_stats *out) {
	memset(out, 0, sizeof(*out));
	for (int k = 0; k < 3; ++k) {
		out->lo[k] = std::numeric_limits<double>::infinity();
		out->hi[k] = -std::numeric_limits<double>::infinity();
	}
}

extern "C" int lfa_frame_stats(lfa_sim *s, struct lfa_frame_stats *out, uint32_t *occupation) {
	if (!s) return LFA_E_INVALID;
	if (!out) return lfa_fail(s, LFA_E_INVALID, "lfa_frame_stats: out is NULL");
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before lfa_frame_stats");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_particles_materialize(s));
	if (s->np == 0) {
		frame_neutral_host(out);
		if (occupation) memset(occupation, 0, s->nc * 4);
		s->frame_timed = false;
		return LFA_OK;
	}
	if (s->dist && !s->binned)
		return lfa_fail(s, LFA_E_INVALID, "slab decomposition: call lfa_hash_particles before downloading particles");
	LFA_TRY(lfa_corr_join(s));
	if (!s->frame_part) {
		hipError_t e = hipMalloc(&s->frame_part, (size_t)FRAME_PART_DOUBLES * 8);
		if (e != hipSuccess) return lfa_fail(s, LFA_E_OOM, "hipMalloc of the frame summary's partials failed");
	}
	for (hipEvent_t &e : s->frame_ev)
		if (!e) LFA_HIP(s, hipEventCreate(&e));
	if (occupation) LFA_TRY(lfa_ensure_io(s, s->nc * 4));
	FrameParams q;
	q.ip = lfa_ingest_params(s);
	for (int k = 0; k < 3; ++k) q.g[k] = s->prm.gravity[k];
	// (slabs with holes: the records [0, np_live) include the leavers' holes - skipped by their key)
	const size_t n_rec = s->binned ? s->np_live : s->np;
	size_t blocks = (n_rec + 255) / 256;
	if (blocks > FRAME_GRID_CAP) blocks = FRAME_GRID_CAP;
	const ParticleSoA &p = s->pb[s->cur];
	s->frame_timed = false;
	LFA_HIP(s, hipEventRecord(s->frame_ev[0], s->stream));
	if (occupation) {
		LFA_HIP(s, hipMemsetAsync(s->io_buf, 0, s->nc * 4, s->stream));
		hipLaunchKernelGGL(k_frame_stats<true>, dim3((unsigned)blocks), dim3(256), 0, s->stream, n_rec, (const PosRec *)p.pos,
		                   (const float *)p.v[0], (const float *)p.v[1],
		                   (const float *)p.v[2], s->g, q, (uint32_t *)s->io_buf, s->frame_part);
	} else {
		hipLaunchKernelGGL(k_frame_stats<false>, dim3((unsigned)blocks), dim3(256), 0, s->stream, n_rec, (const PosRec *)p.pos,
		                   (const float *)p.v[0], (const float *)p.v[1],
		                   (const float *)p.v[2], s->g, q, (uint32_t *)nullptr, s->frame_part);
	}
	LFA_LAUNCH_CHECK(s);
	hipLaunchKernelGGL(k_frame_finish, dim3(1), dim3(256), 0, s->stream, (int)blocks, s->frame_part);
	LFA_LAUNCH_CHECK(s);
	LFA_HIP(s, hipEventRecord(s->frame_ev[1], s->stream));
	double r[FRAME_FIELDS];
	LFA_HIP(s, hipMemcpyAsync(r, s->frame_part + (size_t)FRAME_GRID_CAP * FRAME_FIELDS, sizeof(r), hipMemcpyDeviceToHost, s->stream));
	if (occupation) LFA_HIP(s, hipMemcpyAsync(occupation, s->io_buf, s->nc * 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	s->frame_timed = true;
	out->energy = r[0];
	out->energy_abs = r[1];
	out->max_speed2 = r[2];
	for (int k = 0; k < 3; ++k) {
		out->lo[k] = r[3 + k];
		out->hi[k] = r[6 + k];
	}
	memcpy(&out->n, &r[9], 8);
	memcpy(&out->n_in_grid, &r[10], 8);
	return LFA_OK;
}

extern "C" int lfa_frame_stats_time(lfa_sim *s, double *ms) {
	if (!s || !ms) return LFA_E_INVALID;
	if (!s->frame_timed) return lfa_fail(s, LFA_E_INVALID, "lfa_frame_stats_time: no lfa_frame_stats has run on the device");
	LFA_HIP(s, hipSetDevice(s->device));
	float f = 0.0f;
	LFA_HIP(s, hipEventElapsedTime(&f, s->frame_ev[0], s->frame_ev[1]));
	*ms = (double)f;
	return LFA_OK;
}

extern "C" int lfa_download_positions(lfa_sim *s, double *xyz, uint64_t n) {
	if (!s || (!xyz && n)) return LFA_E_INVALID;
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before lfa_download_positions");
	LFA_HIP(s, hipSetDevice(s->device));
	LFA_TRY(lfa_particles_materialize(s));
	if (n != s->np) return lfa_fail(s, LFA_E_INVALID, "download of %llu positions but %zu particles are resident",
	                                (unsigned long long)n, s->np);
	if (n == 0) return LFA_OK;
	if (s->dist && !s->binned)
		return lfa_fail(s, LFA_E_INVALID, "slab decomposition: call lfa_hash_particles before downloading particles");
	LFA_TRY(lfa_corr_join(s));
	const uint32_t *slot = nullptr;
	LFA_TRY(lfa_slab_download_slots(s, &slot));
	LFA_TRY(lfa_ensure_io(s, n * 24));
	const IngestParams ip = lfa_ingest_params(s);
	const size_t n_rec = s->binned ? s->np_live : s->np;
	const ParticleSoA &p = s->pb[s->cur];
	hipLaunchKernelGGL(k_export_positions, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s->stream, (double *)s->io_buf, n_rec,
	                   (size_t)n, (const PosRec *)p.pos,
	                   (const uint32_t *)p.id, s->g, ip, s->dist ? 1 : 0, slot);
	LFA_LAUNCH_CHECK(s);
	LFA_HIP(s, hipMemcpyAsync(xyz, s->io_buf, n * 24, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	return LFA_OK;
}
