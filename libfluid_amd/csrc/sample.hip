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
// sample_classify and sample_value (sample.h, shared with tracers.hip) are the ONE statement of all that; every kernel below calls them.
//
// Slabs (lfa_sample_velocity_collective, lfa_mesher_vertex_velocities_collective): a rank holds its own tile layers and one ghost
// layer on each side, so it can answer for every point of its own layers once the ghost layers answer like their owners.
// lfa_sample_refresh makes them: the rule of every tile (cell_tile_rule) as its owner's view states it travels first - the ranks'
// views may differ (a rank that kept particles of a collective seeding reads tile_flag, its neighbour still grid_flag) -, then u, v,
// w and ctype of the tiles whose rule reads them, listed under THOSE rules and not under halo_tiles, which every binning rebuilds
// from tile_flag. Every rank classifies every point it is shown and keeps the ones whose cell lies in its own layers: k_sample_count
// (one ballot per 64 consecutive points: owned, outside), a scan, k_sample_write (compact, in input order, no atomics). The
// kernels named _slab are the same bodies with the owners' rules read instead of the flags (OWNER_RULES, a compile-time switch).
#include "sample.h"

/// Dense: one row per point. counts[0]: points outside the grid, counts[1]: inside points whose cell layer is not in [z_lo, z_hi)
/// (none when the range is the whole grid); both kinds get (+0, +0, +0) and type 0.
template <bool OWNER_RULES>
__device__ inline void sample_dense(const double *xyz, size_t n, const GridDims &g, const SampleParams &q, const CellView &cv, double *velocity,
                                    uint8_t *types, uint32_t *counts) {
	const int lane = threadIdx.x & 63;
	uint32_t outside_wave = 0, beyond_wave = 0;  // (the same numbers in every lane of the wave)
	// the whole wave walks the loop together: the ballots below need every lane
	for (size_t base = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (size_t)gridDim.x * 256) {
		const size_t i = base + lane;
		const bool live = i < n;
		double fi[3] = {0.0, 0.0, 0.0};
		const bool inside = live && sample_classify(xyz, i, q, fi);
		const bool answered = inside && sample_answers(fi, q);
		outside_wave += (uint32_t)__popcll(__ballot(live && !inside));
		beyond_wave += (uint32_t)__popcll(__ballot(inside && !answered));
		if (!live) continue;
		double vel[3] = {0.0, 0.0, 0.0};
		uint8_t type = 0;
		if (answered) sample_value<OWNER_RULES>(g, cv, fi, vel, type);
#pragma unroll
		for (int k = 0; k < 3; ++k) velocity[3 * i + k] = vel[k];
		if (types) types[i] = type;
	}
	// integer adds: the totals do not depend on their order
	if (lane == 0 && outside_wave) atomicAdd(counts, outside_wave);
	if (lane == 0 && beyond_wave) atomicAdd(counts + 1, beyond_wave);
}

__global__ void __launch_bounds__(256) k_sample_velocity(const double *xyz, size_t n, GridDims g, SampleParams q, CellView cv, double *velocity,
                                                         uint8_t *types, uint32_t *counts) {
	sample_dense<false>(xyz, n, g, q, cv, velocity, types, counts);
}
/// The same on a slab decomposition: the view carries the owners' rules (lfa_sample_refresh).
__global__ void __launch_bounds__(256) k_sample_velocity_slab(const double *xyz, size_t n, GridDims g, SampleParams q, CellView cv, double *velocity,
                                                              uint8_t *types, uint32_t *counts) {
	sample_dense<true>(xyz, n, g, q, cv, velocity, types, counts);
}

/// Compact, pass 1: per chunk of 64 consecutive points (chunk w: [64 w, 64 w + 64)) the points this rank owns and the points outside.
__global__ void __launch_bounds__(256) k_sample_count(const double *xyz, size_t n, SampleParams q, uint32_t *chunk_owned, uint32_t *chunk_outside) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool live = i < n;
	double fi[3] = {0.0, 0.0, 0.0};
	const bool inside = live && sample_classify(xyz, i, q, fi);
	const bool own = inside && sample_answers(fi, q);
	const unsigned long long mo = __ballot(own), mx = __ballot(live && !inside);
	if ((threadIdx.x & 63) == 0 && (i >> 6) < ((n + 63) >> 6)) {
		chunk_owned[i >> 6] = (uint32_t)__popcll(mo);
		chunk_outside[i >> 6] = (uint32_t)__popcll(mx);
	}
}

/// Compact, pass 2: the classification again; owned point i becomes row owned_off[chunk] + its rank among the chunk's owned points -
/// the rows are in input order, and no atomic decides a position.
template <bool OWNER_RULES>
__device__ inline void sample_write(const double *xyz, size_t n, const GridDims &g, const SampleParams &q, const CellView &cv, const uint32_t *owned_off,
                                    size_t total, uint32_t *index, double *velocity, uint8_t *types) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool live = i < n;
	double fi[3] = {0.0, 0.0, 0.0};
	const bool own = live && sample_classify(xyz, i, q, fi) && sample_answers(fi, q);
	const unsigned long long mo = __ballot(own);
	if (!own) return;  // (a wave that owns nothing ends here)
	const size_t j = (size_t)owned_off[i >> 6] + (size_t)__popcll(mo & ((1ull << (threadIdx.x & 63)) - 1ull));
	if (j >= total) return;  // (cannot happen: both passes classify the same points; keeps a write inside the arrays regardless)
	double vel[3];
	uint8_t type;
	sample_value<OWNER_RULES>(g, cv, fi, vel, type);
	index[j] = (uint32_t)i;
#pragma unroll
	for (int k = 0; k < 3; ++k) velocity[3 * j + k] = vel[k];
	if (types) types[j] = type;
}

__global__ void __launch_bounds__(256) k_sample_write(const double *xyz, size_t n, GridDims g, SampleParams q, CellView cv, const uint32_t *owned_off,
                                                      size_t total, uint32_t *index, double *velocity, uint8_t *types) {
	sample_write<false>(xyz, n, g, q, cv, owned_off, total, index, velocity, types);
}
__global__ void __launch_bounds__(256) k_sample_write_slab(const double *xyz, size_t n, GridDims g, SampleParams q, CellView cv, const uint32_t *owned_off,
                                                           size_t total, uint32_t *index, double *velocity, uint8_t *types) {
	sample_write<true>(xyz, n, g, q, cv, owned_off, total, index, velocity, types);
}

/// Slabs: rule[t] = 1 + cell_tile_rule of the own view for the tiles [t_lo, t_hi) - the own layers.
__global__ void k_sample_tile_rules(CellView cv, uint32_t *rule, int t_lo, int t_hi) {
	const int t = t_lo + (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (t < t_hi) rule[t] = 1u + (uint32_t)cell_tile_rule(cv, (uint32_t)t);
}
/// need[t] = 1 iff a cell of tile t reads the tile's stored fields under its rule (every rule but CELL_BG).
__global__ void k_sample_tile_needs(const uint32_t *rule, uint32_t *need, int t_lo, int t_hi) {
	const int t = t_lo + (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (t < t_hi) need[t] = (rule[t] != 0u && rule[t] != 1u + CELL_BG) ? 1u : 0u;
}

int lfa_sample_velocity_launch(lfa_sim *s, hipStream_t stream, const double *xyz, size_t n, const uint32_t *tile_rule, int z_lo, int z_hi,
                               double *velocity, uint8_t *types, uint32_t *counts_dev) {
	LFA_HIP(s, hipMemsetAsync(counts_dev, 0, 8, stream));
	if (n == 0) return LFA_OK;
	size_t blocks = (n + 255) / 256;
	if (blocks > SAMPLE_GRID_CAP) blocks = SAMPLE_GRID_CAP;
	const SampleParams q = sample_params(s, z_lo, z_hi);
	if (tile_rule)
		hipLaunchKernelGGL(k_sample_velocity_slab, dim3((unsigned)blocks), dim3(256), 0, stream, xyz, n, s->g, q, sample_view(s, tile_rule), velocity, types, counts_dev);
	else
		hipLaunchKernelGGL(k_sample_velocity, dim3((unsigned)blocks), dim3(256), 0, stream, xyz, n, s->g, q, sample_view(s, nullptr), velocity, types, counts_dev);
	LFA_LAUNCH_CHECK(s);
	return LFA_OK;
}

/// What the state of the handle alone decides - the same on every rank of a collective call, so all fail here or none does.
static int sample_state_checks(lfa_sim *s, const char *who) {
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before %s", who);
	if (s->dist && !s->binned)
		return lfa_fail(s, LFA_E_INVALID, "%s on a slab decomposition: call lfa_hash_particles (on every rank) first", who);
	return LFA_OK;
}

int lfa_sample_refresh(lfa_sim *s, const char *who, size_t room_bytes, const uint32_t **tile_rule, void **room, int *z_lo, int *z_hi) {
	LFA_TRY(sample_state_checks(s, who));
	LFA_HIP(s, hipSetDevice(s->device));
	*tile_rule = nullptr;
	*z_lo = 0;
	*z_hi = s->g.nz;
	if (!s->dist) {  // every layer is the handle's own: nothing to refresh, no rule but the view's
		LFA_TRY(lfa_ensure_io(s, room_bytes));
		*room = s->io_buf;
		return LFA_OK;
	}
	const int nt = s->g.nt, L = s->g.ntx * s->g.nty;
	// head of the io buffer: rule[nt] | need[nt] | lists[4 L]
	const size_t head = (((size_t)2 * nt + (size_t)4 * L) * 4 + 255) & ~(size_t)255;
	LFA_TRY(lfa_ensure_io(s, head + room_bytes));
	uint32_t *rule = (uint32_t *)s->io_buf, *need = rule + nt;
	int *lists = (int *)(need + nt);
	*room = (char *)s->io_buf + head;
	const int own_lo = s->slab_lo * L, own_hi = s->slab_hi * L;
	const int all_lo = lfa_has_lo(s) ? own_lo - L : own_lo, all_hi = lfa_has_hi(s) ? own_hi + L : own_hi;
	LFA_HIP(s, hipMemsetAsync(rule, 0, (size_t)2 * nt * 4, s->stream));
	hipLaunchKernelGGL(k_sample_tile_rules, dim3((unsigned)((own_hi - own_lo + 255) / 256)), dim3(256), 0, s->stream, sample_view(s, nullptr), rule,
	                   own_lo, own_hi);
	LFA_LAUNCH_CHECK(s);
	LFA_TRY(lfa_dist_exchange_tile_layers_u32(s, rule));
	hipLaunchKernelGGL(k_sample_tile_needs, dim3((unsigned)((all_hi - all_lo + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t *)rule, need,
	                   all_lo, all_hi);
	LFA_LAUNCH_CHECK(s);
	int n_halo[4];
	LFA_TRY(lfa_dist_build_halo_lists(s, need, lists, n_halo));
	void *f[4] = {s->u, s->v, s->w, s->ctype};
	const int e[4] = {4, 4, 4, 1};
	LFA_TRY(lfa_dist_exchange_fields_of(s, lists, n_halo, 4, f, e));
	*tile_rule = rule;
	*z_lo = lfa_has_lo(s) ? 8 * s->slab_lo - 7 : 0;
	*z_hi = lfa_has_hi(s) ? 8 * s->slab_hi + 7 : s->g.nz;
	if (*z_hi > s->g.nz) *z_hi = s->g.nz;
	return LFA_OK;
}

extern "C" int lfa_sample_velocity(lfa_sim *s, const double *xyz, uint64_t n, double *velocity, uint8_t *types, uint64_t *n_outside) {
	if (!s) return LFA_E_INVALID;
	if (s->dist) return lfa_fail(s, LFA_E_UNSUPPORTED, "lfa_sample_velocity: not on a slab decomposition (the ghost layers would make it a collective: lfa_sample_velocity_collective)");
	if (n >= (1ull << 32)) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity: 2^32 points or more");
	if (n && (!xyz || !velocity)) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity: xyz or velocity is NULL");
	if (n == 0) {
		if (n_outside) *n_outside = 0;
		return LFA_OK;
	}
	if (!(s->prm.cell_size > 0.0)) return lfa_fail(s, LFA_E_INVALID, "set cell_size (lfa_set_params) before lfa_sample_velocity");
	LFA_HIP(s, hipSetDevice(s->device));
	// io buffer: positions | velocities | the count words | type bytes
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
	LFA_TRY(lfa_sample_velocity_launch(s, s->stream, d_xyz, np, nullptr, 0, s->g.nz, d_vel, types ? d_types : (uint8_t *)nullptr, d_count));
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

extern "C" int lfa_sample_velocity_collective(lfa_sim *s, const double *xyz, uint64_t n, uint32_t *index, double *velocity, uint8_t *types,
                                              uint64_t capacity, uint64_t counts[3]) {
	if (!s) return LFA_E_INVALID;
	if (counts) counts[0] = counts[1] = counts[2] = 0;
	// ---- 1, 2: the handle's state, then the ghost refresh - every rank gets this far or none does
	const bool usable = n < (1ull << 32) && !(n && (!xyz || !index || !velocity));
	const size_t np = usable ? (size_t)n : 0, n_chunks = (np + 63) >> 6;
	// io buffer behind the refresh's head: positions | velocities | index | chunk words: owned + total, outside + total | type bytes
	const uint32_t *rule = nullptr;
	void *room = nullptr;
	int z_lo, z_hi;  // (the reach: the dense call's range; the owner of a point is decided by the own layers below)
	LFA_TRY(lfa_sample_refresh(s, "lfa_sample_velocity_collective", np * 48 + np * 4 + (n_chunks + 1) * 8 + np, &rule, &room, &z_lo, &z_hi));
	// ---- 3: this rank's arguments and work; a failure from here on is this rank's alone and costs its peers nothing
	if (n >= (1ull << 32)) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity_collective: 2^32 points or more");
	if (!usable) return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity_collective: xyz, index or velocity is NULL");
	if (np == 0) return LFA_OK;
	const int own_lo = s->dist ? 8 * s->slab_lo : 0, own_hi = s->dist ? 8 * s->slab_hi : s->g.nz;
	double *d_xyz = (double *)room, *d_vel = d_xyz + 3 * np;
	uint32_t *d_index = (uint32_t *)(d_vel + 3 * np), *d_owned = d_index + np, *d_outside = d_owned + n_chunks + 1;
	uint8_t *d_types = (uint8_t *)(d_outside + n_chunks + 1);
	for (hipEvent_t &e : s->sample_ev)
		if (!e) LFA_HIP(s, hipEventCreate(&e));
	s->sample_timed = false;
	const SampleParams q = sample_params(s, own_lo, own_hi);
	const dim3 grid((unsigned)((np + 255) / 256));
	LFA_HIP(s, hipMemcpyAsync(d_xyz, xyz, np * 24, hipMemcpyHostToDevice, s->stream));
	LFA_HIP(s, hipEventRecord(s->sample_ev[0], s->stream));
	hipLaunchKernelGGL(k_sample_count, grid, dim3(256), 0, s->stream, (const double *)d_xyz, np, q, d_owned, d_outside);
	LFA_LAUNCH_CHECK(s);
	LFA_TRY(lfa_exclusive_scan_u32(s, d_owned, d_owned, n_chunks, d_owned + n_chunks));
	LFA_TRY(lfa_exclusive_scan_u32(s, d_outside, d_outside, n_chunks, d_outside + n_chunks));
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + LFA_PIN_SAMPLE_OWNED, d_owned + n_chunks, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipMemcpyAsync(s->h_pinned + LFA_PIN_SAMPLE_OUTSIDE, d_outside + n_chunks, 4, hipMemcpyDeviceToHost, s->stream));
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	const size_t owned = s->h_pinned[LFA_PIN_SAMPLE_OWNED], outside = s->h_pinned[LFA_PIN_SAMPLE_OUTSIDE];
	if (counts) {
		counts[0] = owned;
		counts[1] = outside;
		counts[2] = np - owned - outside;
	}
	if (capacity < owned)
		return lfa_fail(s, LFA_E_INVALID, "lfa_sample_velocity_collective: room for %llu rows but this rank owns %zu of the points",
		                (unsigned long long)capacity, owned);
	if (owned) {
		uint8_t *const d_typ = types ? d_types : (uint8_t *)nullptr;
		if (rule)
			hipLaunchKernelGGL(k_sample_write_slab, grid, dim3(256), 0, s->stream, (const double *)d_xyz, np, s->g, q, sample_view(s, rule),
			                   (const uint32_t *)d_owned, owned, d_index, d_vel, d_typ);
		else
			hipLaunchKernelGGL(k_sample_write, grid, dim3(256), 0, s->stream, (const double *)d_xyz, np, s->g, q, sample_view(s, nullptr),
			                   (const uint32_t *)d_owned, owned, d_index, d_vel, d_typ);
		LFA_LAUNCH_CHECK(s);
	}
	LFA_HIP(s, hipEventRecord(s->sample_ev[1], s->stream));
	if (owned) {
		LFA_HIP(s, hipMemcpyAsync(index, d_index, owned * 4, hipMemcpyDeviceToHost, s->stream));
		LFA_HIP(s, hipMemcpyAsync(velocity, d_vel, owned * 24, hipMemcpyDeviceToHost, s->stream));
		if (types) LFA_HIP(s, hipMemcpyAsync(types, d_types, owned, hipMemcpyDeviceToHost, s->stream));
	}
	LFA_HIP(s, hipStreamSynchronize(s->stream));
	s->sample_timed = true;
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
