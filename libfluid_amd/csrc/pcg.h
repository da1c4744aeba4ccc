// libfluid_amd/csrc/pcg.h -- shared constants and cell / tile primitives of the pressure-solve kernels.
#pragma once
#include "common.h"

// Every reduction of the solve is deterministic: workgroup g writes one partial to partials[PART_x + g], and every
// consumer workgroup re-adds the <= PCG_MAX_GRID partials in the same fixed order. No atomics, no host round trip.
#define PCG_MAX_GRID 2048
#define PCG_WAVES 4          // waves (= tiles in flight) per workgroup
// offsets in doubles; one spare slot after the PCG_MAX_GRID workgroup partials (coarse share of sigma)
enum { PART_STRIDE = PCG_MAX_GRID + 64, PART_ZS = 0, PART_RMAX = PART_STRIDE, PART_SIG0 = 2 * PART_STRIDE,
       PART_SIG1 = 3 * PART_STRIDE, PART_B2 = 4 * PART_STRIDE, PART_TOTAL = 5 * PART_STRIDE };

/// Workgroups of the wave-per-tile kernels of the solve (each wave walks tiles slot, slot + 4 G, ...). LFA_PCG_GRID_CAP (read once,
/// process-wide: the partial-sum layout of every handle depends on it) lowers the cap for experiments.
extern int lfa_pcg_grid_cap;  // core.hip
static inline int pcg_grid(int n_ptiles) {
	int g = (n_ptiles + PCG_WAVES - 1) / PCG_WAVES;
	if (g < 1) g = 1;
	return g < lfa_pcg_grid_cap ? g : lfa_pcg_grid_cap;
}

/// The same without the tuning cap: up to PCG_MAX_GRID workgroups (kernels that run once per solve and stream).
static inline int pcg_grid_uncapped(int n_ptiles) {
	int g = (n_ptiles + PCG_WAVES - 1) / PCG_WAVES;
	if (g < 1) g = 1;
	return g < PCG_MAX_GRID ? g : PCG_MAX_GRID;
}

// ---- cell and tile primitives of the solve's kernels (pcg.hip, mg.hip). The execution forms of the V-cycle - a wave per tile, the
// finest level's pipelines, a workgroup per tile, the dataflow and launch-order forms of k_mg_coarse, the single-tile chain - must
// agree bit for bit (tested): each of them calls these, none types the arithmetic out again.
/// Index of cell (x, y, z) of a tile, each -1 .. 8, in the tile's 10^3 halo block.
/// (A macro on purpose: as a function, even one inlined at once, the compiler associates the address sums differently in twenty
/// kernels, and k_mg_solve_closed<float> goes from 168 to 178 VGPRs, from 3 to 2 waves per SIMD - tools/kernel_diff.py.)
#define halo_at(x, y, z) (((x) + 1) + 10 * ((y) + 1) + 100 * ((z) + 1))
/// The six faces of a halo block, a wave's worth: lane = (lx, ly) over the two in-face axes; v[6] = x-, x+, y-, y+, z-, z+.
/// (A macro for the same reason: as a function it costs k_pcg_a<float, true, false> 8 VGPRs, a wave per SIMD, and the fp64
/// k_mg_prolong_postsmooth five more spills.)
#define store_halo_faces(h, lx, ly, v) \
	do {                               \
		(h)[halo_at(-1, lx, ly)] = (v)[0]; \
		(h)[halo_at(8, lx, ly)] = (v)[1];  \
		(h)[halo_at(lx, -1, ly)] = (v)[2]; \
		(h)[halo_at(lx, 8, ly)] = (v)[3];  \
		(h)[halo_at(lx, ly, -1)] = (v)[4]; \
		(h)[halo_at(lx, ly, 8)] = (v)[5];  \
	} while (0)
/// Halo block of a tile-major vector: interior + the six faces of the neighbour tiles nb[0..6) (0 where there is none).
/// `ld(j)` reads element j of the vector.
template <typename real, typename Load>
__device__ inline void load_halo(real *h, Load ld, size_t base, const int (&nb)[6], int lane, int lx, int ly) {
#pragma unroll
	for (int zz = 0; zz < 8; ++zz) h[halo_at(lx, ly, zz)] = ld(base + zz * 64 + lane);
	const size_t cell[6] = {(size_t)ly * 64 + lx * 8 + 7, (size_t)ly * 64 + lx * 8, (size_t)ly * 64 + 56 + lx, (size_t)ly * 64 + lx,
	                        (size_t)7 * 64 + lane, (size_t)lane};
	real v[6];
#pragma unroll
	for (int k = 0; k < 6; ++k) v[k] = nb[k] >= 0 ? ld((size_t)nb[k] * 512 + cell[k]) : (real)0;
	store_halo_faces(h, lx, ly, v);
}
/// Row i (halo index) of the UNSCALED 7-point operator, term by term in the order of pressure_solver::_apply_a
/// (src/pressure_solver.cpp:334-362): a = the cell's A byte (non-solid neighbour count, "positive neighbour is fluid" bits).
template <typename real> __device__ inline real stencil_row(const real *H, uint32_t a, int i) {
	const real F = (a & AB_FLUID) ? (real)1 : (real)0;
	real val = (real)(a & 7) * H[i];
	val = madd01(-F, H[i - 1], val);
	val = madd01(-F, H[i - 10], val);
	val = madd01(-F, H[i - 100], val);
	val = madd01(-(real)((a >> 3) & 1), H[i + 1], val);
	val = madd01(-(real)((a >> 4) & 1), H[i + 10], val);
	val = madd01(-(real)((a >> 5) & 1), H[i + 100], val);
	return val;
}
/// Residual b - A x of an unknown (unscaled operator), 0 for every other cell.
template <typename real> __device__ inline real residual_cell(const real *H, uint32_t a, real b, int i) {
	real r = (real)0;
	if (a & AB_UNKNOWN) r = b - stencil_row<real>(H, a, i);
	return r;
}
/// Maximum that keeps a NaN.
__device__ inline double nan_max(double x, double y) { return (x != x || y != y) ? NAN : (y > x ? y : x); }
/// The stopping rule of pressure_solver::solve (src/pressure_solver.cpp:54-58) on rmax, the signed maximum of the residual of
/// iteration `slot`: a NaN or rmax < tol ends the solve with iteration count slot + 1.
__device__ inline bool verdict_stops(double rmax, double tol) { return rmax != rmax || rmax < tol; }
/// ... recorded, by ONE thread: the history entry always; when the solve ends the NaN word, the residual beside the state words (the
/// host reads it with them: no read-back of its own) and the iteration count, which the kernels queued behind see and return.
__device__ inline void record_verdict(int *state, double *hist, int slot, double rmax, bool stops) {
	hist[slot] = rmax;
	if (stops) {
		if (rmax != rmax) state[LFA_DW_NAN] = 1;
		*(double *)(state + LFA_DW_RESIDUAL) = rmax;
		state[LFA_DW_DONE] = slot + 1;
	}
}

int lfa_build_rhs(lfa_sim *s, double dt);
int lfa_p2g_run(lfa_sim *s, bool fuse_gravity, double dt);
int lfa_dist_refresh_grid(lfa_sim *s, bool with_topology);

// multigrid preconditioner (mg.hip)
int lfa_mg_setup(lfa_sim *s);                       // hierarchy for the current unknown set (after lfa_build_rhs)
int lfa_mg_apply(lfa_sim *s, double *part_sigma);   // vz = V(vr) / scale (vq is scratch), partials of dot(z, r)
/// Single domain: the residual maxima of iteration `iter` (one per workgroup of the AXPY kernel) that the V-cycle's first kernel
/// tests against the stopping rule (mg.hip: MgStop). part_rmax == nullptr: no test.
struct lfa_mg_stop {
	const double *part_rmax = nullptr;
	int n_part = 0, iter = 0;
};
// the AXPYs of a PCG iteration fused with the pre-smoothing of the finest level, then the rest of the V-cycle (float and double)
template <typename real>
int lfa_mg_axpy_apply(lfa_sim *s, const void *sdir, const double *part_sigma, int n_sigma, const double *part_qs, int n_qs,
                      double *part_rmax, double *part_sigma_new, const lfa_mg_stop &stop);
// slab runs: the single-reduction form (gamma = z.r, delta = (A z).z and max r in one collective; mg.hip: k_mg_axpy_presmooth_cg)
template <typename real>
int lfa_mg_axpy_apply_cg(lfa_sim *s, const double *gamma, int n_gamma, const double *gamma_old, int n_gamma_old, const double *delta,
                         int n_delta, const double *rmax_prev, int n_rmax, int iter, double *alpha_io, double *part_rmax,
                         double *part_sigma_new);
int lfa_mg_bench_part(lfa_sim *s, int part);
int lfa_mg_level0(const lfa_sim *s, const int **tiles, const int **slot);  // the tiles the PCG iterates over (closed ones left out)
int lfa_mg_solve_closed(lfa_sim *s, void *out = nullptr);                  // the closed tiles' own solves of A x = vr (lfa_sim::tile_closed) -> out (null: the pressure)
void lfa_mg_free(lfa_sim *s);
void lfa_mg_stats(const lfa_sim *s, uint64_t *launches_per_cycle, uint64_t *levels, uint64_t *first_co);
