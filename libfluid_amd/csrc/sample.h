// libfluid_amd/csrc/sample.h -- the ONE statement of the grid's velocity at a point (sample_classify + sample_value), shared by the
// kernels of sample.hip and of tracers.hip. The arithmetic and its references are described at the head of sample.hip.
#pragma once

#include "common.h"

#define SAMPLE_GRID_CAP 1024  // workgroups of the pass (frame.hip caps its own alike); beyond 256 x SAMPLE_GRID_CAP points a lane walks several

struct SampleParams {
	IngestParams ip;
	double n[3];  // grid size as doubles: the inside test compares before any cast
	// the cell layers [z_lo, z_hi) the call answers, as doubles: for fi_z >= 0, trunc(fi_z) lies in them iff z_lo <= fi_z < z_hi
	double z_lo, z_hi;
};

__device__ inline double lerp_ref(double a, double b, double t) { return a * (1.0 - t) + b * t; }  // include/fluid/misc.h:20-22
/// trilerp (include/fluid/misc.h:30-36) of q[4 iz + 2 iy + ix]: along ix with t3, along iy with t2, along iz with t1.
__device__ inline double trilerp_ref(const double (&q)[8], double t1, double t2, double t3) {
	const double lo = lerp_ref(lerp_ref(q[0], q[1], t3), lerp_ref(q[2], q[3], t3), t2);
	const double hi = lerp_ref(lerp_ref(q[4], q[5], t3), lerp_ref(q[6], q[7], t3), t2);
	return lerp_ref(lo, hi, t1);
}

/// Component `comp` at sample cell (x, y, z), any integers: the general path.
template <bool OWNER_RULES> __device__ inline double sample_clamped(const GridDims &g, const CellView &cv, int comp, int x, int y, int z) {
	const int c[3] = {x, y, z};
	const int n[3] = {g.nx, g.ny, g.nz};
	if (c[comp] < 0 || c[comp] >= n[comp] - 1) return 0.0;
	const int xx = min(max(x, 0), g.nx - 1), yy = min(max(y, 0), g.ny - 1), zz = min(max(z, 0), g.nz - 1);
	const uint32_t b = blocked_index(g, xx, yy, zz);
	return cell_velocity(cv, cell_tile_rule<OWNER_RULES>(cv, b >> 9), b, comp);
}

/// fi = (x - grid_offset) / cell_size of point i; true iff the point is inside the grid (decided on the doubles, false for NaN).
__device__ inline bool sample_classify(const double *xyz, size_t i, const SampleParams &q, double (&fi)[3]) {
	bool inside = true;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		fi[k] = (xyz[3 * i + k] - q.ip.off[k]) / q.ip.h;
		inside = inside && fi[k] >= 0.0 && fi[k] < q.n[k];
	}
	return inside;
}

/// Velocity and cell type at an INSIDE point with the fi of sample_classify. OWNER_RULES: slabs, the view carries the rule of every
/// tile of the own and the ghost layers as its owner states it (a compile-time switch: the single-domain kernels pay nothing for it).
template <bool OWNER_RULES> __device__ inline void sample_value(const GridDims &g, const CellView &cv, const double (&fi)[3], double (&vel)[3], uint8_t &type) {
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
	const int rule = cell_tile_rule<OWNER_RULES>(cv, b >> 9);
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
				s[comp][k] = sample_clamped<OWNER_RULES>(g, cv, comp, x0[comp] + (k & 1), y0[comp] + ((k >> 1) & 1), z0[comp] + (k >> 2));
	}
	vel[0] = trilerp_ref(s[0], tmid[2], tmid[1], t[0]);
	vel[1] = trilerp_ref(s[1], tmid[2], t[1], tmid[0]);
	vel[2] = trilerp_ref(s[2], t[2], tmid[1], tmid[0]);
}

/// Whether this call answers an inside point: its cell layer trunc(fi_z) is one of [z_lo, z_hi).
__device__ inline bool sample_answers(const double (&fi)[3], const SampleParams &q) { return fi[2] >= q.z_lo && fi[2] < q.z_hi; }

/// The parameters and the view of a sampling kernel on the handle's current grid (tile_rule: null, or what lfa_sample_refresh returned).
inline SampleParams sample_params(const lfa_sim *s, int z_lo, int z_hi) {
	SampleParams q;
	q.ip = lfa_ingest_params(s);
	q.n[0] = (double)s->g.nx; q.n[1] = (double)s->g.ny; q.n[2] = (double)s->g.nz;
	q.z_lo = (double)z_lo;
	q.z_hi = (double)z_hi;
	return q;
}
inline CellView sample_view(const lfa_sim *s, const uint32_t *tile_rule) {
	CellView cv = lfa_cell_view(s, s->u, s->v, s->w, false);
	cv.tile_rule = tile_rule;
	return cv;
}
