// libfluid_amd/csrc/sample.hip -- the grid's velocity at points of the host's choosing, computed where the grid is.
//
// After a step the velocity field is tile-major fp32 u, v, w on the device, and outside the dilated tile set only implied (common.h:
// CellView). A host that wants the fluid's velocity anywhere but at a particle - the testbed's grid_vels copy (testbed/main.cpp:70-78),
// a renderer that motion-blurs the mesher's surface, foam and tracer points - had one route: lfa_download_cells (32 bytes per cell)
// and its own mac_grid::get_face_samples + trilerp. Here: 24 bytes per point up, 24 down, or nothing up at all for the mesher's vertices.
//
// Arithmetic: lfa_sample_velocity(s, x) is the velocity the reference's PIC grid-to-particle transfer gives a particle at x
// (simulation::_transfer_from_grid_pic, src/simulation.cpp:447-461, through mac_grid::get_face_samples, src/mac_grid.cpp:42-112, and
// trilerp, include/fluid/misc.h:20-36) on the grid lfa_download_cells would return: fp64, the reference's operations in its order,
// no contraction - bit for bit.
//  * cell and fraction: fi = (x - grid_offset) / cell_size, a true division; cell = trunc(fi), t = fi - cell, both fp64
//    (particle::compute_cell_index_and_position, src/simulation.cpp:17-23). NOT cell_and_fraction of common.h: its float fraction
//    is the resident particles'.
//  * inside iff fi >= 0 && fi < n on all three axes, decided on the doubles before any cast (false for NaN, +-inf, 1e300). The
//    reference never asks about other points (its advection clamps first): they get (+0, +0, +0), type 0, and are counted.
//  * the 3 x 3 x 3 block around the cell follows _clamp (:42-50): an index below 0 or at or above n - 1 - the last cell counts as
//    clamped - replicates the border cell and zeroes the component along that axis (grid_ops.hip: clamped_sample is the fp32 form).
//    tmid = t - 0.5, shifted by one cell when negative; the three trilerps with the argument order of :451-459 and
//    lerp(a, b, t) = a (1 - t) + b t.
//  * a cell's value is the rule of common.h (cell_tile_rule / cell_velocity / cell_type), the one k_export_cells applies.
//
// One lane per point; the 24 samples come straight from the tile-major fields (no binning of the points, no LDS). When the cell has
// local coordinates 1..6 in its tile and no sample is clamped, the block lies in one tile: one flag lookup, one base index, constant
// offsets. Otherwise every sample resolves its own tile, flag and clamp. The same functions produce the value on both paths.
#include "common.h"

#define SAMPLE_GRID_CAP 1024  // workgroups of the pass (frame.hip caps its own alike); beyond 256 x SAMPLE_GRID_CAP points a lane walks several

struct SampleParams {
	IngestParams ip;
	double n[3];  // grid size as doubles: the inside test compares before any cast
};

__device__ inline double lerp_ref(double a, double b, double t) { return a * (1.0 - t) + b * t; }  // include/fluid/misc.h:20-22
/// trilerp (include/fluid/misc.h:30-36) of q[4 iz + 2 iy + ix]: along ix with t3, along iy with t2, along iz with t1.
__device__ inline double trilerp_ref(const double (&q)[8], double t1, double t2, double t3) {
	const double lo = lerp_ref(lerp_ref(q[0], q[1], t3), lerp_ref(q[2], q[3], t3), t2);
	const double hi = lerp_ref(lerp_ref(q[4], q[5], t3), lerp_ref(q[6], q[7], t3), t2);
	return lerp_ref(lo, hi, t1);
}

/// Component `comp` at sample cell (x, y, z), any integers: the general path.
__device__ inline double sample_clamped(const GridDims &g, const CellView &cv, int comp, int x, int y, int z) {
	const int c[3] = {x, y, z};
	const int n[3] = {g.nx, g.ny, g.nz};
	if (c[comp] < 0 || c[comp] >= n[comp] - 1) return 0.0;
	const int xx = min(max(x, 0), g.nx - 1), yy = min(max(y, 0), g.ny - 1), zz = min(max(z, 0), g.nz - 1);
	const uint32_t b = blocked_index(g, xx, yy, zz);
	return cell_velocity(cv, cell_tile_rule(cv, b >> 9), b, comp);
}

__global__ void __launch_bounds__(256) k_sample_velocity(const double *xyz, size_t n, GridDims g, SampleParams q, CellView cv,
                                                         double *velocity, uint8_t *types, uint32_t *n_outside) {
	const int lane = threadIdx.x & 63;
	uint32_t outside_wave = 0;  // (the same number in every lane of the wave)
	// the whole wave walks the loop together: the ballot below needs every lane
	for (size_t base = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (size_t)gridDim.x * 256) {
		const size_t i = base + lane;
		const bool live = i < n;
		double fi[3] = {0.0, 0.0, 0.0};
		bool inside = live;
		if (live) {
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				fi[k] = (xyz[3 * i + k] - q.ip.off[k]) / q.ip.h;
				inside = inside && fi[k] >= 0.0 && fi[k] < q.n[k];
			}
		}
		outside_wave += (uint32_t)__popcll(__ballot(live && !inside));
		if (!live) continue;
		double vel[3] = {0.0, 0.0, 0.0};
		uint8_t type = 0;
		if (inside) {
			int c[3], d[3];
			double t[3], tmid[3];
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				c[k] = (int)fi[k];
				t[k] = fi[k] - (double)c[k];
				tmid[k] = t[k] - 0.5;
				d[k] = 1;
				if (tmid[k] < 0.0) {
					d[k] = 0;
					tmid[k] += 1.0;
				}
			}
			const uint32_t b = blocked_index(g, c[0], c[1], c[2]);
			const int rule = cell_tile_rule(cv, b >> 9);
			type = cell_type(cv, rule, b);
			// first sample cell (offset 0..1 from it) of the component along x, y, z: get_face_samples' vels[dz + iz][dy + iy][ix] etc.
			const int x0[3] = {c[0] - 1, c[0] + d[0] - 1, c[0] + d[0] - 1};
			const int y0[3] = {c[1] + d[1] - 1, c[1] - 1, c[1] + d[1] - 1};
			const int z0[3] = {c[2] + d[2] - 1, c[2] + d[2] - 1, c[2] - 1};
			const int l[3] = {c[0] & 7, c[1] & 7, c[2] & 7};
			const bool one_tile = l[0] >= 1 && l[0] <= 6 && l[1] >= 1 && l[1] <= 6 && l[2] >= 1 && l[2] <= 6 &&
			                      c[0] + 1 < g.nx - 1 && c[1] + 1 < g.ny - 1 && c[2] + 1 < g.nz - 1;
			double s[3][8];
			if (one_tile) {
				// every sample is a cell of the point's own tile, none is clamped: the tile's rule, the cell's index plus constants
#pragma unroll
				for (int comp = 0; comp < 3; ++comp) {
					const uint32_t b0 = b + (uint32_t)((x0[comp] - c[0]) + 8 * (y0[comp] - c[1]) + 64 * (z0[comp] - c[2]));
#pragma unroll
					for (int k = 0; k < 8; ++k) s[comp][k] = cell_velocity(cv, rule, b0 + (uint32_t)((k & 1) + 8 * ((k >> 1) & 1) + 64 * (k >> 2)), comp);
				}
			} else {
#pragma unroll
				for (int comp = 0; comp < 3; ++comp)
#pragma unroll
					for (int k = 0; k < 8; ++k)
						s[comp][k] = sample_clamped(g, cv, comp, x0[comp] + (k & 1), y0[comp] + ((k >> 1) & 1), z0[comp] + (k >> 2));
			}
			vel[0] = trilerp_ref(s[0], tmid[2], tmid[1], t[0]);
			vel[1] = trilerp_ref(s[1], tmid[2], t[1], tmid[0]);
			vel[2] = trilerp_ref(s[2], t[2], tmid[1], tmid[0]);
		}
#pragma unroll
		for (int k = 0; k < 3; ++k) velocity[3 * i + k] = vel[k];
		if (types) types[i] = type;
	}
	// integer adds: the total does not depend on their order
	if (lane == 0 && outside_wave) atomicAdd(n_outside, outside_wave);
}

int lfa_sample_velocity_launch(lfa_sim *s, hipStream_t stream, const double *xyz, size_t n, double *velocity, uint8_t *types,
                               uint32_t *n_outside_dev) {
	LFA_HIP(s, hipMemsetAsync(n_outside_dev, 0, 4, stream));
	if (n == 0) return LFA_OK;
	SampleParams q;
	q.ip = lfa_ingest_params(s);
	q.n[0] = (double)s->g.nx; q.n[1] = (double)s->g.ny; q.n[2] = (double)s->g.nz;
	size_t blocks = (n + 255) / 256;
	if (blocks > SAMPLE_GRID_CAP) blocks = SAMPLE_GRID_CAP;
	hipLaunchKernelGGL(k_sample_velocity, dim3((unsigned)blocks), dim3(256), 0, stream, xyz, n, s->g, q,
	                   lfa_cell_view(s, s->u, s->v, s->w, false), velocity, types, n_outside_dev);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

extern "C" int lfa_sample_velocity(lfa_sim *s, const double *xyz, uint64_t n, double *velocity, uint8_t *types, uint64_t *n_outside) {
	if (!s) return LFA_E_INVALID;
	if (s->dist) return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_sample_velocity: not on a slab decomposition (the ghost layers would make it a collective)");
	if (n >= (1ull << 32)) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity: 2^32 points or more");
	if (n && (!xyz || !velocity)) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity: xyz or velocity is NULL");
	if (n == 0) {
		if (n_outside) *n_outside = 0;
		return LFA_OK;
	}
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before lfa_sample_velocity");
	LFA_HIP(s, hipSetDevice(s->device));
	// io buffer: positions | velocities | the count word | type bytes
	const size_t np = (size_t)n;
	LFA_TRY(lfa_ensure_io(s, np * 48 + 8 + np));
	double *d_xyz = (double *)s->io_buf, *d_vel = d_xyz + 3 * np;
	uint32_t *d_count = (uint32_t *)(d_vel + 3 * np);
	uint8_t *d_types = (uint8_t *)(d_count + 2);
	for (hipEvent_t &e : s->sample_ev)
		if (!e) LFA_HIP(s, hipEventCreate(&e));
	s->sample_timed = false;
	LFA_HIP(s, hipMemcpyAsync(d_xyz, xyz, np * 24, hipMemcpyHostToDevice, s->stream));
	LFA_HIP(s, hipEventRecord(s->sample_ev[0], s->stream));
	LFA_TRY(lfa_sample_velocity_launch(s, s->stream, d_xyz, np, d_vel, types ? d_types : (uint8_t *)nullptr, d_count));
	LFA_HIP(s, hipEventRecord(s->sample_ev[1], s->stream));
	uint32_t count = 0;
	LFA_HIP(s, hipMemcpyAsync(velocity, d_vel, np * 24, hipMemcpyDeviceToHost, s->stream));
	if (types) LFA_HIP(s, hipMemcpyAsync(types, d_types, np, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	s->sample_timed = true;
	if (n_outside) *n_outside = count;
	return LFA_OK;
}

extern "C" int lfa_sample_velocity_time(lfa_sim *s, double *ms) {
	if (!s || !ms) return LFA_E_INVALID;
	if (!s->sample_timed) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity_time: no lfa_sample_velocity has run on the device");
	LFA_HIP(s, hipSetDevice(s->device));
	float f = 0.0f;
	LFA_HIP(s, hipEventElapsedTime(&f, s->sample_ev[0], s->sample_ev[1]));
	*ms = (double)f;
	return LFA_OK;
}
