/* libfluid_amd.h -- C ABI of the MI355X-native PIC/FLIP/APIC hot path (drop-in for lukedan/libfluid's per-step path).
 *
 * The reference has no FFI: its boundary is the C++ class fluid::simulation (include/fluid/simulation.h:21-280) used
 * identically by the testbed (testbed/main.cpp:91-99,189) and the Maya GridNode (plugins/maya/nodes/grid_node.cpp:
 * 256-274,351-357). This header is the thin layer the north star asks for *beneath* a class with that surface
 * (libfluid_amd/host/simulation.h): plain pointers and sizes, host layouts exactly as the reference holds them.
 *
 *   particles : simulation::particle, 152-B fp64 AoS {position, velocity, cx, cy, cz, old_position, raw_cell_index}
 *               (include/fluid/simulation.h:24-34)
 *   cells     : mac_grid::cell, 32-B AoS {vec3d velocities_posface, u8 type{air=1,fluid=2,solid=4}, pad}, x fastest
 *               (include/fluid/mac_grid.h:15-27, include/fluid/data_structures/grid.h:11-12)
 *   solids    : flat int[3k] (x,y,z) triples as the Maya plugin passes them (plugins/maya/nodes/grid_node.cpp:330-339)
 *   pressure  : double[n] in the reference's unknown order = ascending raw cell index of occupied cells
 *               (src/simulation.cpp:83-94, include/fluid/simulation.h:166)
 *
 * Every function returns LFA_OK (0) or a negative LFA_E_* code; lfa_last_error() gives the text. The library never
 * keeps a host pointer past the call. One host thread per handle; different handles are independent.
 * There is no CPU fallback: without a usable HIP device lfa_create fails with LFA_E_NO_DEVICE.
 */
#ifndef LIBFLUID_AMD_H
#define LIBFLUID_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lfa_sim lfa_sim;

enum {
	LFA_OK = 0,
	LFA_E_INVALID = -1,      /* bad argument / size / state */
	LFA_E_NO_DEVICE = -2,    /* no HIP device or device init failed */
	LFA_E_HIP = -3,          /* a HIP runtime call failed */
	LFA_E_OOM = -4,          /* device allocation failed */
	LFA_E_NAN = -5,          /* NaN/Inf detected in the pressure solve */
	LFA_E_UNSUPPORTED = -6,  /* parameter combination not implemented on the device path */
	LFA_W_PCG_NOT_CONVERGED = 1 /* warning: PCG stopped at max_iterations (reference is silent: pressure_solver.cpp:45) */
};

/* simulation::method, include/fluid/simulation.h:44-48 */
enum { LFA_PIC = 0, LFA_FLIP_BLEND = 1, LFA_APIC = 2 };
/* P2G scatter variant (BASELINE config 2: "P2G atomics vs LDS-binned") */
enum { LFA_P2G_LDS_BINNED = 0, LFA_P2G_GLOBAL_ATOMIC = 1 };
/* MIC(0) schedule. EXACT = hyperplane order over tiles: the same recurrence as pressure_solver.cpp:244-332, hence the
 * same iteration counts as the reference. TILED = MIC(0) restricted to 8x8x8 tiles (couplings across tile faces
 * dropped from the preconditioner only): one launch per application, more iterations, same converged pressure. */
enum { LFA_PRECOND_MIC0_TILED = 0, LFA_PRECOND_MIC0_EXACT = 1,
       /* MULTILEVEL = TILED + additive coarse-space correction: one piecewise-constant unknown per 8^3 tile (Galerkin
        * operator, block MIC(0) again on 8^3 blocks of tiles) and a dense solve of the 64^3-cell aggregates on top.
        * Restores mesh-independent-ish convergence at one launch per level. */
       LFA_PRECOND_MULTILEVEL = 2,
       /* MULTIGRID = geometric multigrid V-cycle (levels of 2x coarser cells down to one tile, rediscretised operators,
        * red-black Gauss-Seidel inside tiles / Jacobi across tile faces, piecewise-constant transfers): the work per
        * iteration stays O(unknowns) and the iteration count barely grows with the grid (about 20 at 512^3 where MIC(0)
        * needs 180). Runs on a slab decomposition too (finest levels distributed, coarser ones replicated, see the slab
        * section below). Same converged pressure, same stopping rule. The default. */
       LFA_PRECOND_MULTIGRID = 3 };
/* arithmetic type of the PCG vectors */
enum { LFA_PCG_F32 = 0, LFA_PCG_F64 = 1 };

/* Public fields of fluid::simulation (include/fluid/simulation.h:179-190) and fluid::pressure_solver
 * (include/fluid/pressure_solver.h:38-42), same names and defaults, plus device-path selectors. */
typedef struct lfa_params {
	double grid_offset[3];
	double gravity[3];
	double cell_size;             /* reference default NaN: must be set */
	double blending_factor;       /* 1.0 */
	double density;               /* 1.0 */
	double boundary_skin_width;   /* 0.1 (used by the "next" rows only) */
	double correction_stiffness;  /* 5.0 (used by the "next" rows only) */
	double cfl_number;            /* 3.0 */
	uint64_t velocity_extrapolation_iterations; /* 1; device path supports 0..8 */
	int32_t simulation_method;    /* LFA_APIC */
	double tau, sigma, tolerance; /* 0.97, 0.25, 1e-6 */
	uint64_t max_iterations;      /* 200 */
	int32_t p2g_variant;          /* LFA_P2G_LDS_BINNED */
	int32_t precond;              /* LFA_PRECOND_MULTIGRID (single domain and slabs) */
	int32_t pcg_dtype;            /* LFA_PCG_F32 */
	int32_t apic_unscaled_kernel; /* 1 (default) = keep the reference quirk simulation.cpp:367-369: the APIC P2G hat is
	                                 evaluated on world-space distances (only differs when cell_size != 1: narrower hat for
	                                 cell_size > 1, wider - truncated by the 27-cell gather - for cell_size < 1);
	                                 0 = divide by cell_size like the PIC transfer does */
	int32_t pcg_fused;            /* 1 = two launches per PCG iteration (k_pcg_a: search direction + A s, k_pcg_b: AXPYs +
	                                 MIC(0) sweeps) where the schedule allows it (single domain, tile-local MIC(0));
	                                 0 = one launch per vector operation. Same arithmetic either way. */
	int32_t pcg_warm_start;       /* 0 (default) = every solve starts from p = 0 like the reference (src/pressure_solver.cpp:36).
	                                 1 = the PCG starts from the pressure of the previous solve where a tile was solved then
	                                 (r = b - A p): same system, same stopping rule, fewer iterations when consecutive steps
	                                 resemble each other (a settling pool; in the violent phase of the C4 dam break 16 -> 15).
	                                 Never with LFA_PRECOND_MIC0_EXACT (the reference-parity schedule) or slabs. */
} lfa_params;

/* -- lifetime ------------------------------------------------------------------------------------------------ */
void lfa_default_params(lfa_params *p);
/* simulation::resize (include/fluid/simulation.h:57) + device selection. device < 0 => current device. */
int lfa_create(lfa_sim **out, uint64_t nx, uint64_t ny, uint64_t nz, int device);
void lfa_destroy(lfa_sim *s);
const char *lfa_last_error(const lfa_sim *s); /* s may be NULL: error of the last failed lfa_create on this thread */
int lfa_set_params(lfa_sim *s, const lfa_params *p);
int lfa_get_params(const lfa_sim *s, lfa_params *p);
int lfa_synchronize(lfa_sim *s);
/* HIP stream all kernels of this handle are launched on (hipStream_t as void*), for external timing/graphs. */
void *lfa_stream(lfa_sim *s);

/* -- data in / out (reference host layouts) ------------------------------------------------------------------ */
/* Replaces the particle set (simulation::particles(), include/fluid/simulation.h:142). Converts to the device layout
 * (fp32 SoA, cell-relative positions) and computes the clamped cell key of src/simulation.cpp:251-261 in fp64. */
int lfa_upload_particles(lfa_sim *s, const void *aos152, uint64_t n);
/* Writes velocity, cx, cy, cz and raw_cell_index (x-fastest raw index, as the reference stores it) of every particle
 * back into the caller's array, in upload order (particle i of the upload is element i).
 * flags: LFA_DL_POSITIONS also writes position/old_position (reconstructed from the device's cell-relative
 * representation); LFA_DL_KEEP_RAW leaves raw_cell_index untouched (the reference's value is the one of the last
 * hash, src/simulation.cpp:62, not the one of the final position). */
enum { LFA_DL_POSITIONS = 1, LFA_DL_KEEP_RAW = 2 };
int lfa_download_particles(lfa_sim *s, void *aos152, uint64_t n, int flags);
uint64_t lfa_num_particles(const lfa_sim *s);
/* With a slab decomposition particles migrate between ranks: lfa_num_particles is the number resident on this rank
 * after the last lfa_hash_particles, lfa_download_particles writes them in storage order, and this call returns the
 * global id of each record (upload index / index in the seeded block). Single domain: ids[i] = i. */
int lfa_download_particle_ids(lfa_sim *s, uint32_t *ids, uint64_t n);
/* -- frame summary: what the hosts read from the particles after every step, without moving the particles ----------------------
 * The testbed's update_simulation (testbed/main.cpp:50-88) copies simulation::particles(), sums 0.5 |v|^2 - g . x into its "total
 * energy" (:54-58) and counts the particles of every cell into an occupation grid (:61-67); its
 * post_grid_to_particle_transfer_callback (:117-123) takes the largest |v|^2. Through lfa_download_particles each of these moves
 * 152 bytes per particle to the device and 152 back. lfa_frame_stats computes all of them in one pass over the resident key, t and
 * v arrays (csrc/frame.hip), from the positions and velocities an LFA_DL_POSITIONS download would report, term by term in the
 * callers' fp64 arithmetic (squared_length: vx vx, += vy vy, += vz vz; dot: gx x, += gy y, += gz z; term = 0.5 sq - dot).
 *   occupation : NULL, or nx ny nz counts, x fastest (grid3's order), overwritten. Cell of a particle:
 *                vec3s(vec3i((position - grid_offset) / cell_size)) - a true fp64 division truncated toward zero, counted iff all
 *                three indices are inside the grid. That is NOT always the cell the particle is binned in (raw_cell_index): the
 *                reconstructed position off + c h, divided by h again, often lands one cell lower, and the hosts' loop sees that.
 *   n, n_in_grid, max_speed2, lo, hi and the grid are exactly what the caller's loop over an LFA_DL_POSITIONS download gives.
 *   energy, energy_abs are sums in a fixed order of the same terms: reproducible (two calls on the same resident state return the
 *   same bits; no floating-point atomics) and within 2 n 2^-53 energy_abs of any other summation order.
 * Works in every state lfa_download_particles works in (unbinned, binned, a correction on its second stream, between lfa_advect and
 * lfa_collide: the moved positions) and changes nothing a later step reads. No particles: LFA_OK, the neutral values below, a
 * zeroed grid. LFA_E_INVALID, nothing written: cell_size unset, out NULL.
 * Slab decomposition: local, no message; covers the records this rank owns (never a ghost copy); needs a binned handle like the
 * download (LFA_E_INVALID otherwise). The ranks' particle sets are a partition, so a job combines the ranks' results itself:
 * n, n_in_grid, energy, energy_abs and the occupation grids ADD; max_speed2 and hi take the MAXIMUM; lo takes the MINIMUM - the
 * integer results, the maximum and the box then equal the single domain's exactly.
 * (The struct has a tag and no typedef: in C a typedef would collide with the function of the same name. Write
 * `struct lfa_frame_stats st;`.) */
struct lfa_frame_stats {
	uint64_t n;            /* resident particles summed over (this rank's own on slabs)            */
	uint64_t n_in_grid;    /* particles counted by the occupation rule = sum of the occupation grid */
	double   energy;       /* sum_i (0.5 |v_i|^2 - g . x_i), fp64, g = the handle's gravity parameter */
	double   energy_abs;   /* sum_i (0.5 |v_i|^2 + |g . x_i|): the condition of that sum            */
	double   max_speed2;   /* max_i |v_i|^2 (0 for no particles; a NaN speed is skipped, as std::max(maxv, nan) skips it) */
	double   lo[3], hi[3]; /* bounding box of the positions (+inf / -inf for no particles)          */
};
int lfa_frame_stats(lfa_sim *s, struct lfa_frame_stats *out, uint32_t *occupation);
/* Device milliseconds of the last lfa_frame_stats of this handle (HIP events around the zeroing of the grid, the pass and the final
 * sum; not the read-back). LFA_E_INVALID when none has run on the device (no call yet, or one with no particles). */
int lfa_frame_stats_time(lfa_sim *s, double *ms);
/* The Maya GridNode's cache loop (plugins/maya/nodes/grid_node.cpp:356-364: position of every particle into an MPointArray after
 * update): double[3 n], n = lfa_num_particles, in the order of lfa_download_particles (single domain: record i = particle i;
 * slabs: storage order, holes closed) and equal to `position` of an LFA_DL_POSITIONS download bit for bit. 24 bytes per particle
 * device to host, nothing host to device. LFA_E_INVALID, nothing written: n is not the resident count, cell_size unset, an
 * unbinned slab handle. */
int lfa_download_positions(lfa_sim *s, double *xyz, uint64_t n);
/* -- grid velocity at points of the caller's choosing -------------------------------------------------------------------------
 * lfa_sample_velocity(s, x) is the velocity the reference's PIC grid-to-particle transfer gives a particle at world position x, on
 * the grid that lfa_download_cells(s) would return at that moment, computed in fp64 with the reference's operations in the
 * reference's order, so it equals the oracle on that download bit for bit (simulation::_transfer_from_grid_pic,
 * src/simulation.cpp:447-461, through mac_grid::get_face_samples, src/mac_grid.cpp:42-112, and trilerp,
 * include/fluid/misc.h:20-36). What it replaces: the download of every cell (32 bytes each) and the host's own copy of those
 * loops - the testbed's grid_vels (testbed/main.cpp:70-78), velocities for motion blur, foam and tracer points.
 *   cell, fraction : fi = (x - grid_offset) / cell_size per axis, a true fp64 division; cell = trunc(fi), t = fi - cell, fp64
 *                    (particle::compute_cell_index_and_position, src/simulation.cpp:17-23).
 *   inside         : fi >= 0 && fi < n on all three axes, decided before any cast: false for NaN, +-inf and huge values. The
 *                    reference never asks about other points (its advection clamps them first); here they get velocity
 *                    (+0.0, +0.0, +0.0) and type 0, and *n_outside counts them.
 *   samples        : the 3 x 3 x 3 block around the cell under _clamp's rule (src/mac_grid.cpp:42-50): an index below 0 or at or
 *                    above n - 1 - the last cell counts as clamped - replicates the border cell and zeroes the component along
 *                    that axis; tmid = t - 0.5, shifted by one cell when negative; the three trilerps with the argument order of
 *                    src/simulation.cpp:451-459 and lerp(a, b, t) = a (1 - t) + b t.
 *   xyz            : double[3 n] world positions (host memory), staged through the handle's io buffer; n < 2^32.
 *   velocity       : double[3 n].     types: NULL, or uint8[n]: the type lfa_download_cells reports for the point's cell.
 *   n_outside      : NULL, or the number of points outside the grid.
 * Reads grid arrays only: particles, binning, pressure system, background and the position correction's state are untouched, so a
 * call between any two stage calls is legal, in every state lfa_download_cells works in (fresh handle, uploaded grid, after
 * lfa_p2g, after lfa_time_step). Two calls on the same state write the same bytes. n == 0: LFA_OK, nothing written but
 * *n_outside = 0. LFA_E_INVALID: n >= 2^32, a NULL array with n > 0, cell_size unset. LFA_E_UNSUPPORTED, before anything is touched,
 * on a slab decomposition (the freshness of the ghost layers makes the call a collective: lfa_sample_velocity_collective). */
int lfa_sample_velocity(lfa_sim *s, const double *xyz, uint64_t n, double *velocity, uint8_t *types, uint64_t *n_outside);
/* The same on a slab decomposition. COLLECTIVE: every rank of the job makes the call, a rank with n == 0 too; the lists may differ
 * from rank to rank (all the same list, each its own, an empty one). A sample block reaches one cell beyond the point's cell, so a
 * rank answers for the points of its own tile layers once its ghost layers answer like their owners - the call makes them (below).
 *   owner    : by cell: c = trunc((x - grid_offset) / cell_size), the division above; the rank whose tile layers hold c_z >> 3.
 *              The inside points are partitioned over the ranks; an outside point belongs to nobody and every rank counts it.
 *   output   : COMPACT and in input order: index[k] = position in xyz of the k-th point this rank owns (ascending),
 *              velocity[3 k ..] and types[k] (or NULL) its values. No row is written for a point the rank does not own; capacity =
 *              the rows index, velocity and types have room for, capacity >= n always suffices. 28 (29) bytes come down per OWNED
 *              point, 24 go up per point shown.
 *   counts   : [0] points this rank answered, [1] points outside the grid, [2] inside points that belong to other ranks;
 *              [0] + [1] + [2] == n.
 *   value    : what lfa_sample_velocity returns on a single-domain handle whose lfa_download_cells is the ranks' downloads
 *              stitched by owned z-range, bit for bit, types included. Two calls on the same state write the same bytes.
 * Order inside the call:
 *   1. the handle's state, the same on every rank by construction: cell_size set, and binned by a collective lfa_hash_particles;
 *      otherwise LFA_E_INVALID (the message names lfa_hash_particles) on every rank, and no message is sent.
 *   2. the ghost refresh, two transport calls: the rule a cell's value follows, per tile of the boundary layers, as its OWNER's
 *      state gives it (stored / stored base plus background / background alone: the ranks' states can differ, e.g. after a
 *      collective seeding that left particles on some ranks only), then u, v, w and the cell types of the tiles whose rule reads
 *      them. What stays the caller's: solid cells and the background are the same on every rank, and after lfa_upload_cells the
 *      ghost layers' base values equal their owners' if every rank uploaded the same whole grid.
 *   3. this rank's arguments and work. LFA_E_INVALID here - a NULL xyz / index / velocity with n > 0, n >= 2^32, capacity below
 *      counts[0] - is this rank's alone: counts is filled (zeros when the list itself is unusable), nothing else is written, the
 *      peers' calls complete unharmed, and a repeat is a NEW collective call that every rank has to make again.
 * On a single domain the call is local (no message, every layer owned): index lists the inside points, so one host code serves 1 and
 * N ranks. lfa_sample_velocity_time then reports the device time from the count pass to the write pass (the read-back of the two
 * totals between them included, the refresh and the copies not). */
int lfa_sample_velocity_collective(lfa_sim *s, const double *xyz, uint64_t n, uint32_t *index, double *velocity, uint8_t *types,
                                   uint64_t capacity, uint64_t counts[3]);
/* Device milliseconds of the kernel of the last lfa_sample_velocity (HIP events on the handle's stream; not the copies).
 * LFA_E_INVALID when none has run on the device. */
int lfa_sample_velocity_time(lfa_sim *s, double *ms);
/* -- tracers: massless markers on the device ------------------------------------------------------------------------------------
 * A tracer has an fp64 world position, an fp64 velocity and the cell type at its position. It moves as a PIC particle of the
 * reference does and is seen by no grid stage (P2G, pressure solve, position correction): dye, debris, foam seeds, streak lines.
 * What it replaces: per step one lfa_sample_velocity (24 bytes per point up, 24 down), the move on the host, and - to stop a
 * point at an obstacle - lfa_download_cells (32 bytes per cell) with the host's own copy of _detect_collisions. Step n of the
 * tracers follows lfa_time_step number n with the same dt:
 *   1. move     : _advect_particles (src/simulation.cpp:240-248): position += velocity * dt, clamped to [grid_offset + skin,
 *                 cell_size * size + grid_offset - skin], skin = boundary_skin_width.
 *   2. collide  : _detect_collisions (:612-683) with grid::march_cells (include/fluid/data_structures/grid.h:140-209): from = the
 *                 position before the move, up to three bounces, the bounce update in world units, then the skin push-out (:654-681).
 *   3. transfer : _transfer_from_grid_pic (:447-461): velocity and type = lfa_sample_velocity at the new position.
 * 1 and 2 read the stored velocity and the solid cells, 3 the grid the step's G2P read, so the result is what a placement inside
 * the step would give. fp64, the reference's operations in its order: positions and velocities equal the oracle's advect,
 * detect_collisions and PIC transfer bit for bit. Two deliberate differences, invisible on finite inputs: the march of a bounce
 * takes at most nx + ny + nz + 3 face crossings, and a tracer whose moved position is not finite in every coordinate (a NaN
 * velocity) is FROZEN: it keeps its position, is counted, and still takes a new velocity in 3.
 * The eight calls below are the single domain's. On a handle with a slab decomposition lfa_tracers_add, _advect_collide, _transfer
 * and _step return LFA_E_UNSUPPORTED before anything is touched (counts and arrays included) - the _collective calls further down
 * take their place -, and lfa_dist_init_* refuses a handle that holds tracers; _count, _clear, _time and _download are local and work
 * there (the rank's own tracers, in storage order).
 *   lfa_tracers_add            : appends n tracers in order; a tracer's index is its rank over all adds since the last clear. xyz
 *                                double[3 n] (host), velocity double[3 n] or NULL: zeros. The total stays below 2^32. A non-finite
 *                                position is LFA_E_INVALID, the message names the first bad index; checked on the host before
 *                                anything is queued: nothing is added. Velocities may be anything. Positions outside the grid are
 *                                accepted: their transfer gives +0.0 and type 0, the first move clamps them in. The type of a new
 *                                tracer is 0 until its first transfer. A handle that never adds a tracer allocates nothing.
 *   lfa_tracers_clear          : no tracers (the arrays are kept for the next add).     lfa_tracers_count: how many there are.
 *   lfa_tracers_advect_collide : steps 1 + 2.     lfa_tracers_transfer: step 3.     lfa_tracers_step: 1 + 2 + 3 in one kernel, the
 *                                same bits as the two stage calls. counts (or NULL: nothing is read back, the call does not wait):
 *                                [0] tracers a march stopped at a solid cell or a wall, [1] tracers frozen.
 *                                The three are queued on the handle's stream behind everything already there and write nothing but
 *                                the tracer arrays. No tracers: LFA_OK, nothing launched. LFA_E_INVALID: dt not finite, cell_size unset.
 *   lfa_tracers_download       : xyz double[3 n], velocity double[3 n], types uint8[n], each or NULL; n = lfa_tracers_count
 *                                (LFA_E_INVALID otherwise).
 *   lfa_tracers_time           : device milliseconds of the last tracer kernel (HIP events on the handle's stream). LFA_E_INVALID
 *                                when none has run since the last clear. */
int lfa_tracers_add(lfa_sim *s, const double *xyz, const double *velocity, uint64_t n);
int lfa_tracers_clear(lfa_sim *s);
int lfa_tracers_count(const lfa_sim *s, uint64_t *n);
int lfa_tracers_advect_collide(lfa_sim *s, double dt);
int lfa_tracers_transfer(lfa_sim *s);
int lfa_tracers_step(lfa_sim *s, double dt, uint64_t counts[2]);
int lfa_tracers_download(lfa_sim *s, double *xyz, double *velocity, uint8_t *types, uint64_t n);
int lfa_tracers_time(lfa_sim *s, double *ms);
/* -- tracers on a slab decomposition ----------------------------------------------------------------------------------------------
 * COLLECTIVE: every rank of the job makes each of these calls, a rank that holds no tracer too. Between calls the job holds a
 * PARTITION of the single domain's tracers: gathered by id, the ranks' positions, velocities and type bytes after k collective steps
 * are the bytes lfa_tracers_download gives on a single-domain handle after k plain steps on the ranks' grids stitched by owned
 * z-range - the move and the collision handling read the solid cells alone, which every rank holds whole, and the transfer is
 * lfa_sample_velocity_collective's: the ghost refresh, then sample_value under the owners' tile rules.
 *   id       : a tracer's index over all adds of the JOB since the last clear, a uint32_t. On a slab handle it is stored beside the
 *              record and travels with it; a single-domain handle stores none (there the id is the storage index).
 *   owner    : the rank whose tile layers hold cz >> 3, cz = floor((z - grid_offset_z) / cell_size) with lfa_sample_velocity's fp64
 *              division, clamped to [0, nz - 1] on the double before any cast. x and y play no part, so a tracer added outside the
 *              grid has an owner too, and its first move clamps it in as on a single domain.
 *   far moves: a tracer's first velocity is the caller's and the move is only clamped to the box, so one step can carry a tracer
 *              across several slabs. Unlike the particle migration, which refuses such a move (and with it the job), the tracers are
 *              FORWARDED hop by hop: after the move every rank finds the lowest and the highest destination layer of the tracers
 *              it no longer owns, maps them to a hop distance through the layer bounds given at init, and ONE max all-reduce makes
 *              it the job's round count R. R rounds follow, each a count exchange and a payload exchange with z-1 / z+1 (56 bytes per
 *              record: six doubles, id and type); a round sends every record a rank holds and does not own, arrivals of the round
 *              before included, down or up by the owner's side. R == 0 - nothing crosses anywhere - costs the all-reduce alone.
 *   placement: deterministic, no atomic decides a position. After a call a rank's arrays are compact: the stayers first, in their
 *              previous order, then the arrivals from below, then those from above, each in the sender's order. Two runs of a job
 *              write the same bytes in the same order on every rank. Arrivals beyond the capacity grow the arrays (everything new
 *              is allocated before anything old is released); a rank that cannot (LFA_E_OOM) closes the transport, so that its
 *              peers' calls fail at once instead of waiting.
 * Order inside every call, as in lfa_sample_velocity_collective: 1. what the handle's state decides and is the same on every rank
 * - dt finite, cell_size set, for the transfer: binned by a collective lfa_hash_particles -, otherwise LFA_E_INVALID on every rank
 * and no message is sent; 2. the transport calls; 3. this rank's own work.
 * On a SINGLE DOMAIN each call is local, sends no message and equals the plain call it replaces, so one host code serves 1 and N
 * ranks.
 *   lfa_tracers_add_collective            : replaces lfa_tracers_add. Every rank passes the SAME list; the rank keeps the tracers it
 *                                           owns, in list order, with id = first_id + index in the list. first_id advances by n on
 *                                           every rank, also on one that keeps nothing. counts (or NULL): [0] kept here, [1] the
 *                                           first_id of this call. The host checks of lfa_tracers_add run on every rank alike before
 *                                           anything is queued (non-finite position; 2^32 tracers or more in the JOB). No message.
 *   lfa_tracers_advect_collide_collective : replaces lfa_tracers_advect_collide: its kernel on the resident tracers, then the
 *                                           migration above. counts (or NULL): [0] stopped, [1] frozen - both of the tracers
 *                                           resident before the move; a frozen tracer keeps its position and so its rank -,
 *                                           [2] records handed down, [3] handed up, [4] records received (a forwarded record counts
 *                                           on every rank it passes: over the job, sum of [2] + [3] == sum of [4]), [5] the rounds R.
 *   lfa_tracers_transfer_collective       : replaces lfa_tracers_transfer: the ghost refresh of lfa_sample_velocity_collective (two
 *                                           transport calls, also on a rank with no tracers), then the transfer of the resident ones.
 *   lfa_tracers_step_collective           : replaces lfa_tracers_step: the two calls above in sequence, with the state checks of both
 *                                           in front, and the same bits. NOT one kernel on slabs - the migration sits between the
 *                                           stages (on a single domain it is lfa_tracers_step's fused kernel).
 *   lfa_tracers_download_ids              : local. lfa_tracers_download with ids uint32[n] (or NULL) in front: the rank's rows in
 *                                           storage order and their ids; on a single domain 0 .. n - 1. n = lfa_tracers_count.
 * lfa_tracers_clear on a slab handle also resets first_id, so EVERY rank has to call it; lfa_tracers_time then covers the move and
 * the rank's share of the migration (or the transfer kernel). */
int lfa_tracers_add_collective(lfa_sim *s, const double *xyz, const double *velocity, uint64_t n, uint64_t counts[2]);
int lfa_tracers_advect_collide_collective(lfa_sim *s, double dt, uint64_t counts[6]);
int lfa_tracers_transfer_collective(lfa_sim *s);
int lfa_tracers_step_collective(lfa_sim *s, double dt, uint64_t counts[6]);
int lfa_tracers_download_ids(lfa_sim *s, uint32_t *ids, double *xyz, double *velocity, uint8_t *types, uint64_t n);
/* Synthetic dam-break block [lo,hi) in cells, 8 jittered particles per cell, generated on the device; bit-identical
 * to libfluid_amd/scenes.py:seed_block. */
int lfa_seed_block(lfa_sim *s, const int64_t lo[3], const int64_t hi[3], uint64_t seed);
/* simulation::seed_box / seed_sphere (src/simulation.cpp:153-181, seed_func include/fluid/simulation.h:80-115) on the device: the
 * particles the reference's loop seeds from a pcg32 in state *rng_state, bit for bit and in its order, APPENDED behind the
 * resident particles (velocity as given, C = 0, ids continuing). Candidate sub-cell i of the loop nest starts at draw 6 i -
 * three doubles of two 32-bit draws each, as libstdc++'s uniform_real_distribution<double> takes them (generate_canonical:
 * first draw = low word) - so every candidate is evaluated by its own thread after a jump-ahead of the generator, in the host
 * loop's fp64 arithmetic, and a compaction in candidate order gives the reference's list (csrc/seed.hip).
 *   rng_state : raw 64-bit state of the pcg32 (XSH-RR 64/32, multiplier 6364136223846793005, increment 1442695040888963407) on
 *               entry; on success the state after all 6 x candidates draws, as the host loop leaves it (an empty cell range draws
 *               nothing). Unchanged on failure.
 *   flags     : LFA_SEED_DRAW_LTR - the three doubles of a candidate are x, y, z in drawing order (a reference built with a
 *               compiler that evaluates `vec3d(dist(random), dist(random), dist(random))`, simulation.h:101, left to right);
 *               default: z, y, x, what g++ does.
 *   n_seeded  : particles appended (may be NULL)
 *   positions : NULL, or room for positions_capacity particles: receives the exact fp64 world positions double[3 n_seeded] in
 *               seeding order (the device keeps an fp32 in-cell fraction: a later download cannot return them).
 * LFA_E_INVALID, and nothing appended: cell_size unset, density 0 or above 16, positions_capacity below the count, 2^32
 * particles or more in all, a NULL pointer.
 *
 * Slab decomposition: LFA_E_UNSUPPORTED, and nothing changed, unless flags carry LFA_SEED_COLLECTIVE. With it the call is
 * COLLECTIVE in that every rank of the job must make it, with the same arguments and the same *rng_state; no message is sent.
 * Every rank evaluates every candidate and appends, in candidate order, the accepted ones whose clamped cell - the one the
 * particle's key holds - lies in its own tile layers: the ranks' lists are a partition of the single-domain list.
 *   - the id of a particle is its index in the single-domain list, counted on from the job's numbering before the call
 *     (lfa_download_particle_ids); ids are unique across ranks;
 *   - n_seeded, positions and positions_capacity speak of the particles THIS rank keeps (it allocates room for those alone);
 *   - *rng_state advances by 6 x candidates on every rank, also on one that keeps nothing, and the job's numbering by the
 *     job-wide count; the 2^32 limit is tested against that count, so every rank decides alike;
 *   - the resident records may be in any state lfa_time_step or lfa_hash_particles leaves them in: records that a hand-over to
 *     a neighbour rank has left as holes are closed up by the call itself. Like on a single domain the particles are unbinned
 *     afterwards: lfa_hash_particles (collective) before a download.
 * What the arguments decide fails on every rank alike, before anything changes. A failure of one rank alone (a short positions
 * buffer, no memory) leaves THAT handle as it was while the others have seeded: the job must not go on seeding with handles
 * that disagree - it ends, or starts over from lfa_upload_particles.
 * On a single domain LFA_SEED_COLLECTIVE changes nothing, so one host code serves 1 and N ranks. */
enum { LFA_SEED_DRAW_LTR = 1, LFA_SEED_COLLECTIVE = 2 };
int lfa_seed_box(lfa_sim *s, const double start[3], const double size[3], const double velocity[3], uint64_t density,
                 uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions, uint64_t positions_capacity);
int lfa_seed_sphere(lfa_sim *s, const double centre[3], double radius, const double velocity[3], uint64_t density,
                    uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions, uint64_t positions_capacity);
/* The last successful lfa_seed_box / lfa_seed_sphere of this handle: out[0] candidates drawn, out[1] particles accepted in the
 * WHOLE job (single domain: n_seeded), out[2] id of the first of them. All zero before the first call. */
int lfa_seed_last(const lfa_sim *s, uint64_t out[3]);
/* Marks cells solid (flat int[3k] triples). lfa_clear_solid_cells resets every cell to non-solid. */
int lfa_set_solid_cells(lfa_sim *s, const int32_t *xyz, uint64_t k);
int lfa_clear_solid_cells(lfa_sim *s);
/* Whole MAC grid in the reference layout (32-B AoS, x fastest). upload takes velocities and solid flags. */
int lfa_upload_cells(lfa_sim *s, const void *aos32);
int lfa_download_cells(lfa_sim *s, void *aos32);
int lfa_download_old_cells(lfa_sim *s, void *aos32); /* FLIP's _old_grid (src/simulation.cpp:340-344) */

/* -- hot-path stages, individually callable for parity tests ---------------------------------- */
/* a2: bins particles by 8x8x8 tile and counts particles per cell (src/simulation.cpp:251-291). */
int lfa_hash_particles(lfa_sim *s);
uint64_t lfa_num_fluid_cells(lfa_sim *s);
/* _fluid_cells: ascending raw indices of cells holding particles (include/fluid/simulation.h:209). */
int lfa_download_fluid_cells(lfa_sim *s, uint64_t *raw, uint64_t n);
/* per-cell particle counts (the `count` half of _space_hash, include/fluid/simulation.h:193-197,207), x fastest. */
int lfa_download_cell_counts(lfa_sim *s, uint32_t *count);
/* a4-a6: simulation::_transfer_to_grid (src/simulation.cpp:400-412).
 * RANGE (p2g_variant = LFA_P2G_LDS_BINNED, the default): the scatter accumulates in 64-bit fixed point, and the conversion of one
 * contribution w (v + C (face - p)), w <= 1, is valid below 2^15. A host stays inside it with
 *     |v| + |C| * cell_size < 32768      for every particle, in the world units of one step
 * (PIC / FLIP: |v| alone). Beyond it the face velocities are wrong without any error being reported. LFA_P2G_GLOBAL_ATOMIC
 * accumulates in fp32 and has no such limit. */
int lfa_p2g(lfa_sim *s);
/* a7: gravity loop (src/simulation.cpp:72-78). */
int lfa_add_gravity(lfa_sim *s, double dt);
/* a8-a12: unknown set, A bits, divergence rhs, MIC(0) factor (src/pressure_solver.cpp:19-25,150-294). */
int lfa_build_system(lfa_sim *s, double dt);
int lfa_download_abits(lfa_sim *s, uint8_t *bits, uint64_t n);   /* bits0-2 nonsolid, 3 xpos, 4 ypos, 5 zpos */
int lfa_download_rhs(lfa_sim *s, double *b, uint64_t n);
int lfa_download_precon(lfa_sim *s, double *precon, uint64_t n);
/* a13/a14 in isolation (vectors in the reference's unknown order). */
int lfa_apply_preconditioner(lfa_sim *s, const double *r, double *z, uint64_t n);
int lfa_apply_a(lfa_sim *s, const double *v, double *out, uint64_t n);
/* a16: pressure_solver::solve (src/pressure_solver.cpp:19-71); includes lfa_build_system like the reference's solve().
 * Returns LFA_W_PCG_NOT_CONVERGED if it stopped at max_iterations. */
int lfa_pcg_solve(lfa_sim *s, double dt, double *residual, uint64_t *iterations);
int lfa_download_pressure(lfa_sim *s, double *p, uint64_t n);
int lfa_upload_pressure(lfa_sim *s, const double *p, uint64_t n); /* a host callback may edit it (simulation.h:166) */
/* a17: pressure_solver::apply_pressure (src/pressure_solver.cpp:73-148). */
int lfa_apply_pressure(lfa_sim *s, double dt);
/* a18: simulation::_extrapolate_velocities (src/simulation.cpp:685-754). */
int lfa_extrapolate(lfa_sim *s);
/* a19-a20: simulation::_transfer_from_grid (src/simulation.cpp:548-560). Works on the particle order of the last
 * lfa_hash_particles: particles that lfa_correct_collide has since moved out of their tile are transferred by a gather
 * kernel (the new cell must still lie in the processed tiles, i.e. within a tile of the P2G-time particles), so no second
 * binning is needed before it (lfa_time_step relies on this). */
int lfa_g2p(lfa_sim *s);
/* a21: simulation::cfl (src/simulation.cpp:199-205); +inf when every velocity is zero. */
int lfa_cfl(lfa_sim *s, double *out);

/* One pass of the hot path, device resident, no host synchronisation except the PCG convergence polls:
 * hash -> P2G -> gravity -> build+PCG -> apply pressure -> extrapolate -> G2P  (src/simulation.cpp:62-66,72-78,
 * 83-104,119-121). residual/iterations may be NULL. */
int lfa_step_hot(lfa_sim *s, double dt, double *residual, uint64_t *iterations);

/* -- the per-step particle stages around the hot path, device resident ----------------------------
 * lfa_advect_collide : simulation::_advect_particles (src/simulation.cpp:226-249, with the sources' velocity coercion) fused with the
 *                      _detect_collisions that follows it (:612-683, grid::march_cells grid.h:140-209; from = old position)
 * lfa_correct_collide: simulation::_correct_positions (:562-610) fused with the _detect_collisions after it (:114-117);
 *                      needs lfa_hash_particles of the current positions
 * lfa_time_step      : simulation::time_step(dt) (:43-125) entirely on the device: advect+collide, hash, P2G, gravity,
 *                      pressure solve, pressure gradient, correct+collide, extrapolate, hash, G2P; sources included, no callbacks
 *                      (the host class falls back to stage calls when it needs them).
 * With a slab decomposition both move stages end with the particle migration: particles whose cell left the owned tile
 * layers are packed (68 B records) and handed to the neighbour rank, arrivals are appended; lfa_correct_collide first
 * fetches ghost copies (key + fraction) of the neighbours' adjacent tile layers, so pairs across a slab face interact. */
/* Fluid sources: simulation::sources (include/fluid/simulation.h:179; include/fluid/data_structures/source.h:12-22) as the
 * hosts fill them (testbed/main.cpp:141-165, plugins/maya/nodes/grid_node.cpp:295-303: flat int[3k] cell triples).
 *   lfa_clear_sources / lfa_add_source : replace the list (sources keep their order: a later coercing source wins a cell, a
 *                        later seeding source tops a cell up beyond an earlier one's target, exactly as the sequential
 *                        loops of src/simulation.cpp:227-238 and :756-765 do)
 *   lfa_update_sources : simulation::_update_sources (:756-765) + the hash_particles that follows it (:64): every cell of an
 *                        active source is topped up to target_density_cubic_root^3 particles (seed_cell, :136-151: uniformly
 *                        random positions inside the cell, the source's velocity, C = 0), counted by the last
 *                        lfa_hash_particles. By default the positions come from a counter-based generator: parity is the
 *                        particle count per cell and every non-random field. lfa_update_sources_rng / lfa_set_source_rng
 *                        (below) draw them from the simulation's pcg32 instead, bit for bit the reference's particles.
 *                        New particles get the next ids (download order).
 * lfa_advect_collide applies the velocity coercion of _advect_particles (:227-238: velocity = the source's, C = 0 for every
 * particle inside a cell of an active coercing source) before it moves the particles; lfa_time_step runs the seeding
 * between its two binnings when a source is active. Slab decompositions: every rank is handed the whole list (like the solid
 * cells) and tops up the cells of its own tile layers; lfa_update_sources is a collective then (every rank calls it). */
int lfa_clear_sources(lfa_sim *s);
int lfa_add_source(lfa_sim *s, const int32_t *xyz, uint64_t k, const double velocity[3], uint64_t target_density_cubic_root,
                   int active, int coerce_velocity);
int lfa_update_sources(lfa_sim *s, uint64_t *n_seeded);
/* lfa_update_sources with the reference's own draws: simulation::_update_sources (src/simulation.cpp:756-765) walks the active
 * sources in order and their cells in list order and calls seed_cell (:136-151), which creates target - count particles at
 *     position = (grid_offset + vec3d(cell) * cell_size) + vec3d(dist(random), dist(random), dist(random)),
 * dist = uniform_real_distribution<double>(0, cell_size): six 32-bit draws of the simulation's pcg32 per particle, as libstdc++
 * takes them. New particle k of a call, counted over all cells in that order, therefore starts at draw 6 k from the state on
 * entry - k is the exclusive scan of the entries' needs that lfa_update_sources computes anyway -, so every entry jumps there and
 * draws its own particles (csrc/seed.hip: k_source_write). Inactive sources and full cells draw nothing. Velocity = (float)
 * of the source's, C = 0, ids continue in draw order; the call ends with the re-binning, like lfa_update_sources.
 *   rng_state : raw pcg32 state (see lfa_seed_box) on entry; on success the state after 6 x n_seeded draws. Unchanged on failure.
 *   flags     : 0 - z gets the first pair of draws, then y, then x (g++'s right-to-left evaluation of :145) - or LFA_SEED_DRAW_LTR.
 *   positions : NULL, or room for positions_capacity particles: the exact fp64 world positions double[3 n_seeded] in draw order.
 * What the device stores is what lfa_upload_particles would store for the reference's record: key and fp32 fraction per axis come
 * from the POSITION, by the upload's rule, not from the source cell. The two differ only when offset + draw rounds up onto the far
 * face of the source cell: the reference keeps such a particle in the source cell's hash entry (raw_cell_index = the source cell,
 * :147) for the rest of that one step - its next update_and_hash_particles moves it -, the device bins it in the neighbouring
 * cell at once. That is the only deviation, and it is the one every uploaded particle is subject to.
 * LFA_E_INVALID, records and state untouched: no lfa_hash_particles since the particles last changed, cell_size unset, a NULL
 * rng_state, positions_capacity below the count, 2^32 particles or more in all, a flag other than the two named here.
 * LFA_E_UNSUPPORTED, and nothing changed, on a slab decomposition without LFA_SEED_COLLECTIVE.
 *
 * Slab decomposition, flags | LFA_SEED_COLLECTIVE: the call is a COLLECTIVE. Every rank makes it with the same *rng_state and
 * flags after the same lfa_add_source list (every rank is handed the whole list anyway). The draw number of an entry is its offset
 * among the new particles of ALL ranks in source order, and that order interleaves the ranks' entries: the ranks' needs are summed
 * into one vector over the job-wide entry list and scanned on every rank. That is ONE transport call per seeding call (an
 * all-reduce of one float per entry; none when no active source lists a cell), beside those of the re-binning that ends the call.
 * The ranks' new particles are a partition of the single-domain call's:
 *   - a particle belongs to the rank whose tile layers hold its KEY - the clamped cell of its fp64 position, not the source cell
 *     (the ownership rule of the collective lfa_seed_box): a position that rounds onto the far z face of a slab's top cell layer
 *     is created on the rank above;
 *   - the id of a particle is the job's numbering before the call plus its index in the single-domain draw order; ids are unique
 *     across ranks, and each rank's records and positions follow that order;
 *   - n_seeded, positions and positions_capacity speak of the particles THIS rank keeps;
 *   - *rng_state advances by 6 x the job-wide count on every rank, also on one that keeps nothing, and the job's numbering by
 *     the job-wide count; the 2^32 limit is tested against that count, so every rank decides alike;
 *   - the call ends with the re-binning on every rank, or - nothing to create anywhere - on none.
 * What the arguments and the job-wide count decide fails on every rank alike, before anything changes. A failure of one rank
 * alone (a short positions buffer, no memory) leaves THAT handle as it was; its peers have seeded, and their re-binning - which
 * needs every rank - fails with LFA_E_HIP (the in-process transport reports the lost peer at once, the others when their wait
 * runs out). As for lfa_seed_box the job must not go on with handles that disagree: it ends, or starts over from
 * lfa_upload_particles. On a single domain LFA_SEED_COLLECTIVE changes nothing, so one host code serves 1 and N ranks.
 *
 * lfa_set_source_rng(on = 1) makes this the behaviour of the plain lfa_update_sources and of the seeding inside lfa_time_step:
 * they draw from the state kept in the handle and advance it (the host class carries `pcg32 random`, include/fluid/simulation.h:177,
 * through a step this way); lfa_get_source_rng reads the mode and the state back. on = 0, the default, restores the counter-based
 * generator exactly as before, its sequence included (on slabs: ids in rank order). flags as above; with LFA_SEED_COLLECTIVE the
 * mode is accepted on a handle with a transport - every rank switches it on with the same state - and stays valid when a transport
 * is attached later. LFA_E_UNSUPPORTED: on = 1 without LFA_SEED_COLLECTIVE on a handle with a transport; when a transport is
 * attached after the mode was switched on without it, lfa_update_sources and lfa_time_step refuse instead, before they change
 * anything.
 *
 * lfa_source_last: the last successful source seeding of this handle that drew from the pcg32 (a call that created nothing drew
 * nothing and leaves it alone): out[0] particles created in the WHOLE job, out[1] particles kept by this handle (single domain:
 * the same), out[2] id of the first of them. All zero before the first such call. */
int lfa_update_sources_rng(lfa_sim *s, uint64_t *rng_state, int flags, uint64_t *n_seeded, double *positions,
                           uint64_t positions_capacity);
int lfa_set_source_rng(lfa_sim *s, int on, uint64_t rng_state, int flags);
int lfa_get_source_rng(const lfa_sim *s, int *on, uint64_t *rng_state);
int lfa_source_last(const lfa_sim *s, uint64_t out[3]);
int lfa_advect_collide(lfa_sim *s, double dt);
int lfa_correct_collide(lfa_sim *s, double dt);
/* The same two stages with the collision handling split off, for hosts that install post_advection_callback or
 * post_correction_callback: simulation::time_step runs _advect_particles -> callback -> _detect_collisions
 * (src/simulation.cpp:50-59) and _correct_positions -> callback -> _detect_collisions (:111-117). lfa_advect / lfa_correct move
 * the particles and keep the positions of before on the device; a download in between reports them as old_position;
 * lfa_collide runs _detect_collisions (:612-683) from there to the current positions. After an upload in between lfa_collide
 * starts from the uploaded positions (from = to: the skin push-out alone). Slab decompositions: the particles change rank in
 * lfa_collide, once they have their final positions (a collective: every rank calls it).
 * Every stage that hands particles over (lfa_advect_collide, lfa_collide, lfa_correct_collide, lfa_time_step) hands them to the
 * adjacent rank: a particle that ends in a tile layer the adjacent rank does not own makes its rank return LFA_E_UNSUPPORTED
 * before anything is handed over and closes the transport (the peers' next exchange fails); the job's handles are unusable then. */
int lfa_advect(lfa_sim *s, double dt);
int lfa_correct(lfa_sim *s, double dt);
int lfa_collide(lfa_sim *s);
int lfa_time_step(lfa_sim *s, double dt, double *residual, uint64_t *iterations);
/* Device time of the stages of the last lfa_time_step in milliseconds (timing enabled), HIP events on the handle's stream:
 * [0] advect+collide  [1] binning  [2] P2G (scatter + finalize + gravity)  [3] P2G scatter kernel alone
 * [4] pressure system + preconditioner set-up  [5] PCG loop  [6] pressure gradient  [7] cell index of the position
 * correction (k_build_fine_index)  [8] LDS-tiled correction kernel alone  [9] correct+collide as a whole (7 + 8 + fallback)
 * [10] extrapolation  [11] G2P  [12] whole step  [13] PCG iterations of the step (a count, not a time)
 * [14] mean PCG iteration ([5] / [13])  [15] 1 if the correction ran beside the solve (lfa_set_step_overlap), else 0.
 * Overlapped, [7] [8] [9] are spans on the correction's own stream and [4] [5] [6] [10] spans on the main one: each is
 * stretched by the other side's kernels sharing the device, and they no longer add up to [12]. */
#define LFA_NUM_STEP_TIMERS 16
enum { /* index of each entry, in the order above */
	LFA_STEP_TIMER_ADVECT_COLLIDE,
	LFA_STEP_TIMER_BIN,
	LFA_STEP_TIMER_P2G,
	LFA_STEP_TIMER_P2G_SCATTER_KERNEL,
	LFA_STEP_TIMER_BUILD_SYSTEM,
	LFA_STEP_TIMER_PCG_LOOP,
	LFA_STEP_TIMER_APPLY_PRESSURE,
	LFA_STEP_TIMER_CORRECT_CELL_INDEX,
	LFA_STEP_TIMER_CORRECT_TILED_KERNEL,
	LFA_STEP_TIMER_CORRECT_COLLIDE,
	LFA_STEP_TIMER_EXTRAPOLATE,
	LFA_STEP_TIMER_G2P,
	LFA_STEP_TIMER_TIME_STEP,
	LFA_STEP_TIMER_PCG_ITERATIONS,     /* a count, not a time */
	LFA_STEP_TIMER_PCG_ITERATION_MEAN, /* a mean of times: PCG loop / iterations */
	LFA_STEP_TIMER_OVERLAPPED          /* a flag, not a time */
};
int lfa_get_step_timings(lfa_sim *s, double ms[LFA_NUM_STEP_TIMERS]);
/* lfa_time_step on a single domain runs the position correction (particle arrays only; simulation.cpp:99-106) on a second HIP
 * stream beside the pressure solve, the pressure gradient and the extrapolation (grid arrays only; :82-97, :119): forked after
 * the P2G, joined before the G2P. Results are identical either way; on = 0 runs the stages back to back (stage attribution).
 * Default: on. A slab decomposition overlaps the same way: the ghost-particle exchange happens on the main stream before the fork,
 * the migration after the join - no communication is issued from the correction's stream. */
int lfa_set_step_overlap(lfa_sim *s, int on);
/* The same fork / join for a host that calls the stages one by one (libfluid_amd/host/simulation.h with stage callbacks):
 * _begin enqueues lfa_correct_collide on the second stream behind everything enqueued so far and returns; until _end the
 * particle arrays and the solid mask are the correction's - grid-only calls (lfa_add_gravity, lfa_build_system, lfa_pcg_solve,
 * lfa_download/upload_pressure, lfa_apply_pressure, lfa_extrapolate, lfa_download_cells) run beside it, every other entry
 * point joins first (as if _end had been called). _end makes the main stream wait for it (no-op if nothing is in flight).
 * _undo (only between _begin and _end) joins and puts back the positions of before the correction - exactly: the correction
 * keeps its inputs - for a host whose callback asks for particles(), or changes the solid mask, at a point of the reference's
 * step order that lies before the correction (simulation.cpp:82-99); it then calls lfa_correct_collide where the reference does.
 * Single domain only (LFA_E_UNSUPPORTED on a slab decomposition). */
int lfa_correct_collide_begin(lfa_sim *s, double dt);
int lfa_correct_collide_end(lfa_sim *s);
int lfa_correct_collide_undo(lfa_sim *s);

/* -- multi-GPU: z-slab domain decomposition ---------------------------------------------------------
 * One handle per GPU/process, every handle created with the GLOBAL grid size. Rank r owns the tile layers
 * [bounds[r], bounds[r+1]) (a tile layer = 8 cells in z) and the particles inside them; one ghost tile layer on each side
 * is refreshed by nearest-neighbour exchanges (tile flags, P2G boundary planes, u/v/w/type halos, one z-slice of the PCG
 * search vector per iteration) and two scalar collectives per PCG iteration. The multigrid preconditioner runs the same
 * V-cycle as on a single domain: its finest levels (while no tile layer straddles a slab face: pick layer_bounds that are
 * multiples of 8 tile layers to keep four levels distributed) exchange one z-slice per face and smoothing step, the
 * coarser levels are replicated through one sum all-reduce of the restricted residual per V-cycle. The reference has no
 * distributed mode; this replaces nothing in it.
 *   lfa_dist_unique_id  : rank 0 fills a 128-byte RCCL id, the caller broadcasts it (e.g. torch.distributed)
 *   lfa_dist_init_rccl  : ncclCommInitRank on this handle's device; send/recv to z+-1 and all-reduce run on the
 *                         handle's stream over xGMI
 *   lfa_dist_local_*    : the same protocol between handles of ONE process (one host thread per handle), device-to-device
 *                         copies instead of RCCL: how the slab logic is tested on a single GPU ("virtual slabs")
 *   lfa_dist_init_shm   : one PROCESS per rank, messages staged through the POSIX shared-memory segment `name` ("/..."; rank 0
 *                         creates it, every rank of the job passes the same name; LFA_SHM_SLOT_MB = per-rank slot, default 32;
 *                         LFA_SHM_TIMEOUT_S = how long a rank waits for its peers before the call fails, default 60).
 *                         No RCCL and no peer access, ranks may share a GPU: the functional fallback when the communicator
 *                         cannot be created, and the way N processes are exercised on a 1-GPU box. Two PCIe crossings per
 *                         message: not a transport to quote throughput on. */
int lfa_dist_unique_id(void *id128);
int lfa_dist_init_rccl(lfa_sim *s, int rank, int nranks, const void *id128, const int32_t *layer_bounds);
typedef struct lfa_hub lfa_hub;
lfa_hub *lfa_dist_local_hub_create(int nranks);
void lfa_dist_local_hub_destroy(lfa_hub *h);
int lfa_dist_init_local(lfa_sim *s, lfa_hub *h, int rank, const int32_t *layer_bounds);
int lfa_dist_init_shm(lfa_sim *s, const char *name, int rank, int nranks, const int32_t *layer_bounds);
/* Owned tile layers of this handle ([0, ntz) without a decomposition). */
int lfa_dist_get_slab(const lfa_sim *s, int32_t *lo, int32_t *hi);
/* Marks the handle's transport as given up by the job (a PEER failed to create its communicator, a rank died): lfa_destroy then
 * releases it without waiting for the peers (ncclCommAbort). A healthy handle is not marked: its communicator is drained and
 * destroyed. Nothing in the reference (it is single-process). */
int lfa_dist_abandon(lfa_sim *s);

/* -- solid-boundary voxelizer ----------------------------------------------------------------
 * Replaces fluid::voxelizer (include/fluid/voxelizer.h:14-74, src/voxelizer.cpp:12-136) as the Maya VoxelizerNode
 * drives it (plugins/maya/nodes/voxelizer_node.cpp:255-343; fluid::obstacle, src/data_structures/obstacle.cpp:9-29, runs
 * the same sequence). Cell classification is bit-exact (fp64, the reference's operation
 * order). Host layouts: positions = double[3 nv]; indices = uint32 or uint64 triples (mesh<..., int|size_t, ...>);
 * voxel types = one byte per cell, x fastest (grid3<cell_type>); cell lists = int32 (x,y,z) triples in grid3::for_each
 * order, as the plugin passes them on to lfa_set_solid_cells (grid_node.cpp:330-339).
 *   lfa_voxels_create            : grid3<cell_type>(size, interior) at a given offset  (resize_reposition_grid*)
 *   lfa_voxels_voxelize_triangles: voxelizer::voxelize_mesh_surface (voxelizer.h:55-63)
 *   lfa_voxels_mark_exterior     : voxelizer::mark_exterior (voxelizer.cpp:83-124)
 *   lfa_voxelize_mesh            : get_bounding_box + resize_reposition_grid_constrained + the two above, i.e. the whole
 *                                  sequence of obstacle.cpp:12-18 / voxelizer_node.cpp:255-268
 *   lfa_voxels_cells             : ref_grid_size == NULL: voxel-grid coordinates of the selected types ("cells",
 *                                  voxelizer_node.cpp:285-323); otherwise reference-grid coordinates clipped to the
 *                                  reference grid ("cells_ref" :325-343). obstacle.cpp:20-28 means the same list
 *                                  (interior only) but bounds its walk over the voxel grid with a corner in
 *                                  reference-grid coordinates, which is out of range for positive offsets; that
 *                                  defect is not reproduced
 *   lfa_set_solid_from_voxels    : the same selection marked solid in a simulation grid without leaving the device */
typedef struct lfa_voxels lfa_voxels;
enum { LFA_VOX_INTERIOR = 0, LFA_VOX_EXTERIOR = 1, LFA_VOX_SURFACE = 2 }; /* voxelizer::cell_type, voxelizer.h:17-21 */
int lfa_voxels_create(lfa_voxels **out, const uint64_t size[3], const double grid_offset[3], double cell_size, int device);
void lfa_voxels_destroy(lfa_voxels *v);
const char *lfa_voxels_last_error(const lfa_voxels *v);
int lfa_voxels_info(const lfa_voxels *v, int32_t grid_min[3], uint64_t size[3], double grid_offset[3], double *cell_size);
int lfa_voxels_upload(lfa_voxels *v, const uint8_t *types);
int lfa_voxels_download(lfa_voxels *v, uint8_t *types);
int lfa_voxels_voxelize_triangles(lfa_voxels *v, const double *positions, uint64_t n_vertices, const void *indices,
                                  int index_bytes, uint64_t n_indices);
int lfa_voxels_mark_exterior(lfa_voxels *v);
int lfa_voxelize_mesh(lfa_voxels **out, const double *positions, uint64_t n_vertices, const void *indices, int index_bytes,
                      uint64_t n_indices, double cell_size, const double ref_grid_offset[3], int device);
int lfa_voxels_count(lfa_voxels *v, int include_interior, int include_surface, const int64_t *ref_grid_size, uint64_t *count);
int lfa_voxels_cells(lfa_voxels *v, int include_interior, int include_surface, const int64_t *ref_grid_size, int32_t *xyz,
                     uint64_t capacity, uint64_t *count);
int lfa_set_solid_from_voxels(lfa_sim *s, lfa_voxels *v, int include_interior, int include_surface);

/* -- surface mesher ---------------------------------------------------------------------------
 * Replaces fluid::mesher (include/fluid/mesher.h:14-46, src/mesher.cpp:320-515): implicit surface function sampled from
 * particle positions + marching cubes with shared vertices. Bit-exact: sampled values, vertex positions, vertex order
 * and index list equal the reference's (fp64, its summation order and its vertex numbering).
 * Host layouts: particle positions = double[3 n] (std::vector<vec3d>); values = double per grid point, x fastest,
 * (size + 1)^3 of them (grid3<double> _surface_function); mesh = double[3 nv] positions + uint64 indices (mesh_t).
 *   lfa_mesher_create          : mesher::resize(size) + the public fields grid_offset, cell_size, particle_extent,
 *                                cell_radius (mesher.h:28-32)
 *   lfa_mesher_sample          : mesher::_sample_surface_function(particles, r) (mesher.cpp:333-376)
 *   lfa_mesher_marching_cubes  : mesher::_marching_cubes() (mesher.cpp:400-515); the two together = generate_mesh (:325)
 *   lfa_mesher_upload_values / download_values : the sampled function, for stage-level parity tests */
/* A z-window of the grid (slab decompositions, BASELINE configs[4] on 8 GPUs): the handle stores, samples and meshes only the
 * cell layers [zlo, zhi) of the whole grid `size` - plus what it needs around them: the point planes zlo - 1 .. zhi and the
 * cells cell_radius beyond those. All arithmetic uses the whole grid's coordinates, so N windows that partition [0, size[2])
 * produce, concatenated in z order, exactly the single-grid mesh: the same vertex positions in the same order, and the same
 * index list once every window's indices have been shifted by the number of vertices of all windows below it
 * (lfa_mesher_rebase; the vertices on the plane between two windows belong to the lower one, the upper one refers to them).
 * The only thing the windows have to tell each other is a vertex count: an exclusive scan over the ranks.
 *   lfa_mesher_create_window : as lfa_mesher_create for the layers [zlo, zhi)
 *   lfa_mesher_window        : first stored point plane, number of stored planes (what lfa_mesher_download_values returns),
 *                              first and one-past-last own cell layer
 *   lfa_mesher_sample_ids    : lfa_mesher_sample with an order key per particle: inside a cell the reference visits the newest
 *                              particle first (space_hashing.h:55-62), i.e. descending index in the host's array; a rank that
 *                              holds its particles in some other order passes their global indices
 *   lfa_mesher_rebase        : adds `vertices_below` to every index of the mesh just extracted
 * lfa_mesher_sample_sim works on a handle with a slab decomposition too: the rank's own particles plus the ghost copies of its
 * neighbours' adjacent tile layers, ordered by global id (the window must not need more than those 8 cells beyond the slab). */
typedef struct lfa_mesher lfa_mesher;
int lfa_mesher_create_window(lfa_mesher **out, const uint64_t size[3], const double grid_offset[3], double cell_size,
                             double particle_extent, uint64_t cell_radius, uint64_t zlo, uint64_t zhi, int device);
int lfa_mesher_window(const lfa_mesher *m, uint64_t *z0, uint64_t *n_planes, uint64_t *own_lo, uint64_t *own_hi);
int lfa_mesher_sample_ids(lfa_mesher *m, const double *positions, const uint32_t *ids, uint64_t n, double r);
int lfa_mesher_rebase(lfa_mesher *m, uint64_t vertices_below);
int lfa_mesher_create(lfa_mesher **out, const uint64_t size[3], const double grid_offset[3], double cell_size,
                      double particle_extent, uint64_t cell_radius, int device);
void lfa_mesher_destroy(lfa_mesher *m);
const char *lfa_mesher_last_error(const lfa_mesher *m);
int lfa_mesher_sample(lfa_mesher *m, const double *positions, uint64_t n, double r);
/* the same from the particles resident in a simulation handle (upload order, the positions LFA_DL_POSITIONS reports):
 * what testbed/main.cpp:52-61,101-113 does through a host copy, without the PCIe round trip */
int lfa_mesher_sample_sim(lfa_mesher *m, lfa_sim *s, double r);
int lfa_mesher_download_values(lfa_mesher *m, double *values);
int lfa_mesher_upload_values(lfa_mesher *m, const double *values);
int lfa_mesher_marching_cubes(lfa_mesher *m, uint64_t *n_vertices, uint64_t *n_indices);
int lfa_mesher_download_mesh(lfa_mesher *m, double *positions, uint64_t *indices);
/* Vertex normals of the mesh just extracted: mesh::generate_normals() (include/fluid/data_structures/mesh.h:38-53 with
 * NormalT = double; cross product and normalized_checked of include/fluid/math/vec.h:355-398,546-548), which every caller runs
 * right after generate_mesh (testbed/main.cpp:224-225). Bit-exact and reproducible: no atomics - every vertex gathers the face
 * vectors of its triangles in ascending triangle index, the order of the reference's loop, which the vertex numbering gives
 * without a sort (mesher.hip). A vertex whose sum is not longer than 1e-6 gets (1, 0, 0); a NaN sum stays NaN.
 *   lfa_mesher_normals          : computes them on the device. LFA_E_INVALID unless lfa_mesher_marching_cubes has succeeded on
 *                                 this handle since the values were last sampled or uploaded (never stale normals).
 *                                 LFA_E_UNSUPPORTED on a z-window that is not the whole grid: the vertices on a window's upper
 *                                 plane have triangles in the window above. An empty mesh is LFA_OK. Indices that
 *                                 lfa_mesher_rebase has shifted give the same normals: the shift is remembered.
 *   lfa_mesher_download_normals : double[3 nv] in the vertex order of lfa_mesher_download_mesh; LFA_E_INVALID without a preceding
 *                                 lfa_mesher_normals for the current mesh; an empty mesh writes nothing.
 *   lfa_mesher_normals_time     : device time of the last lfa_mesher_normals (HIP events on the mesher's stream, milliseconds)
 * The buffers (24 B per vertex, 24 B per triangle) exist from the first lfa_mesher_normals on; a handle that never asks
 * allocates and launches nothing more. */
int lfa_mesher_normals(lfa_mesher *m);
int lfa_mesher_download_normals(lfa_mesher *m, double *normals);
int lfa_mesher_normals_time(lfa_mesher *m, double *ms);
/* The same on z-windows, for a slab run: what replaces downloading every rank's mesh, concatenating them and running the serial
 * mesh::generate_normals() (mesh.h:38-53) on the host. The windows' normals, concatenated in z order, are the single grid's bit
 * for bit. A vertex on a window's upper plane has triangles in the first cell layer of the window above; they are the last
 * terms of its ordered sum, so the lower window continues its sum with that layer's face vectors. These, with the layer's case
 * bytes, are the upper window's BOUNDARY: uint8 case per cell of its layer own_lo (nx ny, x fastest) and double[3] per triangle of
 * that layer in triangle order (a prefix of its triangle list). The caller moves it to the window below; the windows need nothing
 * else from each other (the vertices of the plane below a window are recomputed from its own samples, mesher.cpp:378-392).
 *   lfa_mesher_boundary_size       : cells (nx ny) and triangles of the boundary of the current mesh. LFA_E_INVALID without a
 *                                    current mesh or on a window that starts at layer 0.
 *   lfa_mesher_download_boundary   : the boundary into host memory (cases[n_cells], face[3 n_triangles]); the face vectors are
 *                                    computed on the first request for the current mesh.
 *   lfa_mesher_window_normals      : mesh::generate_normals() for the vertices this window owns, kept on the device for
 *                                    lfa_mesher_download_normals / lfa_mesher_normals_time. cases_above / face_above /
 *                                    n_triangles_above: the boundary of the window directly above; NULL / NULL / 0 exactly when the
 *                                    window reaches the top of the grid (on the whole grid this is lfa_mesher_normals).
 *                                    LFA_E_INVALID, and no normals, when a boundary is missing or surplus, when n_triangles_above
 *                                    is not what cases_above imply, or when the boundary contradicts this window's mesh: the
 *                                    bottom corners of every imported cell are the top corners of the own cell below it and must
 *                                    lie on the same side of the surface (a stale boundary, or one of another window; the message
 *                                    names the first such cell).
 *   lfa_mesher_window_normals_from : the same with the boundary taken from the handle of the window directly above (same grid,
 *                                    above->own_lo == own_hi, else LFA_E_INVALID): device to device on one GPU, staged through the
 *                                    host otherwise.
 * lfa_mesher_rebase on either handle, before or after, changes nothing. Normals and boundary go stale like lfa_mesher_normals'
 * results. The buffers (boundary in and out, the recomputed vertices) exist from the first request on. */
int lfa_mesher_boundary_size(lfa_mesher *m, uint64_t *n_cells, uint64_t *n_triangles);
int lfa_mesher_download_boundary(lfa_mesher *m, uint8_t *cases, double *face);
int lfa_mesher_window_normals(lfa_mesher *m, const uint8_t *cases_above, const double *face_above, uint64_t n_triangles_above);
int lfa_mesher_window_normals_from(lfa_mesher *m, lfa_mesher *above);
/* One velocity per vertex of the mesh just extracted: lfa_sample_velocity (above: simulation::_transfer_from_grid_pic,
 * src/simulation.cpp:447-461; mac_grid::get_face_samples, src/mac_grid.cpp:42-112; trilerp, include/fluid/misc.h:20-36) of the
 * simulation `s` at the fp64 vertex positions this handle holds on the device - what a renderer needs to motion-blur the surface.
 * No position crosses PCIe; the result equals lfa_sample_velocity on the positions of lfa_mesher_download_mesh bit for bit.
 *   lfa_mesher_vertex_velocities   : computes them into a per-vertex buffer kept for the download; *n_outside (or NULL): vertices
 *                                    outside the simulation's box (the mesher's grid may be larger), which get zeros. Ordered
 *                                    after everything queued on the simulation's stream, like lfa_mesher_sample_sim. Needs a
 *                                    current mesh (LFA_E_INVALID unless lfa_mesher_marching_cubes has succeeded since the values
 *                                    were last sampled or uploaded); an empty mesh is LFA_OK. LFA_E_INVALID when the handles live
 *                                    on different devices; LFA_E_UNSUPPORTED, nothing touched, when `s` is a slab decomposition (below).
 *                                    On a z-window: the vertices the window owns; the windows' results, concatenated in z order,
 *                                    are the whole grid's. lfa_mesher_rebase changes nothing.
 *   lfa_mesher_vertex_velocities_collective : the same when `s` is a slab decomposition. COLLECTIVE in `s`: every rank makes the
 *                                    call, with the state checks and the ghost refresh of lfa_sample_velocity_collective first
 *                                    (steps 1 and 2 there); what follows - the mesher's own checks above included - is the rank's
 *                                    alone. The result stays dense, one row per vertex. A window's vertices on its top plane lie
 *                                    in the cell layer of the rank above, so a rank answers by REACH, not by ownership: every
 *                                    vertex whose cell z lies in [max(0, 8 lo - 7), min(nz, 8 hi + 7)) for the rank's tile layers
 *                                    [lo, hi) - the sample block of such a cell stays inside the own and the ghost layers.
 *                                    counts: [0] vertices outside the simulation's box, [1] vertices inside it but beyond this
 *                                    rank's reach; both kinds get +0.0. With the windows [8 lo, min(8 hi, nz)) on the
 *                                    simulation's own grid counts[1] == 0 on every rank, and the windows' results, concatenated
 *                                    in z order, are the job's. On a single domain it equals lfa_mesher_vertex_velocities.
 *   lfa_mesher_download_velocities : double[3 nv] in the vertex order of lfa_mesher_download_mesh; LFA_E_INVALID without a
 *                                    preceding lfa_mesher_vertex_velocities for the current mesh (the velocities go stale exactly
 *                                    where the normals do); an empty mesh writes nothing.
 *   lfa_mesher_velocities_time     : device time of the last lfa_mesher_vertex_velocities (HIP events, milliseconds)
 * The buffer (24 B per vertex) exists from the first request on. */
int lfa_mesher_vertex_velocities(lfa_mesher *m, lfa_sim *s, uint64_t *n_outside);
int lfa_mesher_vertex_velocities_collective(lfa_mesher *m, lfa_sim *s, uint64_t counts[2]);
int lfa_mesher_download_velocities(lfa_mesher *m, double *velocity);
int lfa_mesher_velocities_time(lfa_mesher *m, double *ms);

/* -- measurement --------------------------------------------------------------------------------------------- */
/* Per-stage device time of the last lfa_step_hot, measured with HIP events on the handle's stream (milliseconds):
 * [0] hash/bin [1] P2G [2] gravity [3] build system [4] PCG loop [5] apply pressure [6] extrapolate [7] G2P
 * [8] P2G scatter kernel alone [9] mean PCG iteration (PCG loop / iterations). Enabled by lfa_enable_timing(s,1). */
#define LFA_NUM_TIMERS 10
enum { /* index of each entry, in the order above */
	LFA_TIMER_BIN,
	LFA_TIMER_P2G,
	LFA_TIMER_GRAVITY,
	LFA_TIMER_BUILD_SYSTEM,
	LFA_TIMER_PCG_LOOP,
	LFA_TIMER_APPLY_PRESSURE,
	LFA_TIMER_EXTRAPOLATE,
	LFA_TIMER_G2P,
	LFA_TIMER_P2G_SCATTER_KERNEL,
	LFA_TIMER_PCG_ITERATION_MEAN /* a mean of times: PCG loop / iterations */
};
int lfa_enable_timing(lfa_sim *s, int on);
int lfa_get_timings(lfa_sim *s, double ms[LFA_NUM_TIMERS]);
/* counts of the last step: [0] particles [1] unknowns (fluid cells) [2] tiles holding particles [3] tiles processed
 * by grid kernels (dilated set) [4] padded cell count */
int lfa_get_counts(lfa_sim *s, uint64_t counts[5]);
/* The last pressure solve, per PCG iteration (no member of the reference corresponds: pressure_solver::solve,
 * src/pressure_solver.cpp:45-69, is one host loop): [0] kernel launches of one iteration [1] transport calls (neighbour
 * exchanges + all-reduces; 0 on a single domain) of one iteration [2] levels of the multigrid hierarchy (0: another
 * preconditioner) [3] first level that runs inside the single coarse-level launch [4] iterations of the solve
 * [5] transport calls of the whole solve [6] not a figure of the solve: how many LDS-binned scatters of lfa_p2g on this handle so far read v and C
 * through the source index of a deferred binning (the slot of the one-launch solve of small systems, which left the library in
 * round 5; read-only, for tests of that path) [7] device-side waits given up on this handle so far (0 in a healthy run; after the first one the handle keeps
 * to the launch-per-phase path, and the solve that met it was repeated there). */
#define LFA_NUM_SOLVER_STATS 8
int lfa_get_solver_stats(lfa_sim *s, uint64_t stats[LFA_NUM_SOLVER_STATS]);
/* Active tiles (8^3 cells of the level) per level of the last multigrid hierarchy, finest first; levels beyond the hierarchy
 * are 0. Diagnostic (sparse scenes: a kernel of the V-cycle pays per tile); no member of the reference corresponds. */
#define LFA_MAX_MG_LEVELS 12
int lfa_get_mg_level_tiles(lfa_sim *s, uint64_t tiles[LFA_MAX_MG_LEVELS]);
/* The last position correction: [0] half tiles handled by the LDS-tiled kernel's fallback (a thread per particle gathering from
 * global memory: crowded blocks of more than 12288 staged particles) [1] half tiles in all. Joins a correction in
 * flight. A large [0] / [1] means the scene is far denser than 8 particles per cell and the correction runs slowly.
 * _ex adds [2]: half tiles that took the tiled kernel's second pass (more than 5632 staged particles: one workgroup per CU). */
int lfa_get_correction_stats(lfa_sim *s, uint64_t stats[2]);
int lfa_get_correction_stats_ex(lfa_sim *s, uint64_t stats[3]);

/* Times `reps` back-to-back launches of one hot-path kernel on the state left by the last lfa_step_hot, with HIP
 * events on the handle's stream; returns the mean launch duration in milliseconds. For bench.py's roofline object. */
enum {
	LFA_K_SPMV_DOT = 0,    /* z = A s, dot(z,s)                         algorithmic 17 n bytes */
	LFA_K_AXPY_MAX = 1,    /* p += a s, r -= a z, max r                 algorithmic 28 n bytes */
	LFA_K_MIC_APPLY = 2,   /* z = M^-1 r (fwd+bwd), dot(z,r)            algorithmic 34 n bytes */
	LFA_K_UPDATE_S = 3,    /* s = z + b s                               algorithmic 12 n bytes */
	LFA_K_P2G_SCATTER = 4, /* particles -> per-tile (sum wv, sum w)     algorithmic 60 Np (APIC) / 24 Np bytes */
	LFA_K_P2G_FINALIZE = 5,/* normalise + type + gravity                algorithmic 14 Nc bytes (+12 Nc FLIP) */
	LFA_K_G2P = 6,         /* grid -> particles                         algorithmic 60 Np + 12 Nc (APIC) */
	LFA_K_BIN = 7,         /* tile binning (count + scatter)            algorithmic 2*68 Np + 8 Np bytes */
	LFA_K_MIC_FINE = 8,    /* the tile-level sweep kernel of LFA_K_MIC_APPLY alone (k_mic_apply) */
	LFA_K_COARSE = 9,      /* the coarse levels of the multilevel preconditioner alone (side stream in the solve) */
	LFA_K_PCG_A = 10,      /* fused: s = z + beta s, q = A s, dot(q,s)   algorithmic 12 n + 17 n bytes */
	LFA_K_PCG_B = 11,      /* fused: p += a s, r -= a q, max r, z = M^-1 r, dot(z,r)   algorithmic 28 n + 34 n bytes */
	/* LFA_PRECOND_MULTIGRID: the parts of one iteration besides LFA_K_PCG_A */
	LFA_K_MG_AXPY_PRESMOOTH = 12, /* p += a s, r -= a q, max r + red-black pre-smoothing of the finest level  28 n + 5 n */
	LFA_K_MG_DOWN0 = 13,          /* finest level: residual + restriction                                     9.5 n */
	LFA_K_MG_COARSE = 14,         /* all coarser levels: down, single-workgroup tail, up (latency bound)          */
	LFA_K_MG_UP0 = 15             /* finest level: prolongation + post-smoothing + dot(z, r)                   21 n */
};
int lfa_bench_kernel(lfa_sim *s, int which, int reps, double *mean_ms);
/* Measured HBM ceilings of this device beside the 8 TB/s spec peak (SURVEY.md 8d "report both"): a float4 grid-stride device
 * copy of `bytes` (read + write counted) and a read-only pass over the same buffer, GB/s, mean of `reps` launches. */
int lfa_bench_stream(lfa_sim *s, uint64_t bytes, int reps, double *copy_gbs, double *read_gbs);
/* Handle re-creation is cheap (fluid::simulation::resize() per Maya evaluation, plugins/maya/nodes/grid_node.cpp:256-274): device
 * blocks, streams, events and the pinned page of destroyed handles are cached process-wide and adopted by the next lfa_create /
 * allocation of the same size. lfa_pool_trim releases the cache to the driver (shutdown, memory pressure; LFA_POOL_MAX_BYTES
 * bounds it, default a quarter of the device memory). lfa_pool_stats: [0] cached bytes [1] cached blocks [2] allocations served
 * from the cache [3] allocations that went to the driver. */
void lfa_pool_trim(void);
void lfa_pool_stats(uint64_t stats[4]);
/* Which copy kernel gave the figure of the last lfa_bench_stream (a static string; "" before the first call). */
const char *lfa_bench_stream_variant(void);

#ifdef __cplusplus
}
#endif
#endif
