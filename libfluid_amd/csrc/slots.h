// The layout of the handle's small shared arrays: every word of pcg_state, h_pinned, dist_red and pcg_hist and every event of
// ev[] has its name and its owner here and nowhere else. Plain enums - `s->pcg_state + LFA_DW_N_LEAVERS` is the word it always
// was, plus a name - and the static_asserts that keep the claims apart. A new claim is a new line in this file.
#pragma once

#include "../../include/libfluid_amd.h"  // LFA_MAX_MG_LEVELS

// ---------------------------------------------------------------------------------------------------- lfa_sim::pcg_state
// Device ints: despite the member's name the whole library's device scalar block. Kernels take it as `int *state`.
enum {
	LFA_DW_DONE = 0,           // solver: < 0 while iterating, else the iteration count (k_pcg_a, k_check_converged, k_check_rhs, mg_stop)
	LFA_DW_NAN = 1,            // solver: a NaN was met
	LFA_DW_GAVE_UP = 2,        // solver: a device-side wait was given up (mg.hip: co_wait, co_get; dist.hip: k_pack_triple)
	LFA_DW_RHS = 3,            // solver: k_check_rhs' verdict - 1: zero right-hand side, 2: NaN in it
	LFA_DW_SOLVER_WORDS = 4,   // [0, 4): what the start of every solve resets to {-1, 0, 0, 0}
	LFA_DW_COARSE_TICKET = 4,  // pcg.hip: the multilevel coarse solve's ticket (coarse_args)
	LFA_DW_SCAN_TOTAL = 5,     // core.hip: resident records (lfa_slab_download_slots, lfa_particles_close_holes)
	LFA_DW_N_LEAVERS = 6,      // grid_ops.hip: the G2P's leaver count
	LFA_DW_VMAX2_BITS = 7,     // grid_ops.hip: max |v|^2 as float bits, for lfa_cfl (lfa_sim::vmax2_valid)
	LFA_DW_N_PTILES = 8,       // core.hip, binning of a single domain: particle tiles ...
	LFA_DW_N_DTILES = 9,       // ... and processed tiles (one 8-byte read-back)
	LFA_DW_N_UNKNOWNS = 10,    // core.hip: lfa_number_unknowns
	LFA_DW_SLAB_MARKS = 12,    // core.hip, binning of a slab: the four layer marks k_gather_u32 reads [12, 16)
	LFA_DW_SLAB_MARKS_END = 16,
	LFA_DW_RESIDUAL = 16,      // solver: the final residual, a double [16, 18) (mg_stop, k_check_rhs)
	LFA_DW_GAVE_UP_REASON = 18,  // solver: why the wait was given up (0x100 a co_wait | 0x400 a co_get, | the waiter's XCC id)
	LFA_DW_READBACK_WORDS = 20,  // [0, 20): what a solve reads back in one copy
	LFA_DW_SLAB = 20,          // core.hip, binning of a slab: its totals, LFA_SLAB_* below [20, 30)
	LFA_DW_ALLOC = 32,         // words allocated
};
// Words of the slab binning's block, from LFA_DW_SLAB on the device and from LFA_PIN_SLAB on the host
enum {
	LFA_SLAB_N_PTILES = 0,   // particle tiles of the own and the ghost layers
	LFA_SLAB_MARK_SCAN = 1,  // the tile scan at the four layer marks [1, 5)
	LFA_SLAB_N_DTILES = 5,   // processed tiles
	LFA_SLAB_N_HALO = 6,     // the four halo lists [6, 10); lfa_dist_build_halo_lists counts its own lists in the same four
	LFA_SLAB_WORDS = 10,
};
enum { LFA_DW_COUNT = LFA_DW_SLAB + LFA_SLAB_WORDS };
static_assert(LFA_DW_COUNT <= LFA_DW_ALLOC, "pcg_state: a claim lies beyond the allocation");
static_assert(LFA_DW_RESIDUAL % 2 == 0, "pcg_state: the residual is a double and needs 8-byte alignment");
static_assert(LFA_DW_GAVE_UP_REASON < LFA_DW_READBACK_WORDS && LFA_DW_RESIDUAL + 2 <= LFA_DW_READBACK_WORDS,
              "pcg_state: the read-back must cover the residual and the give-up reason");
static_assert(LFA_DW_DONE == 0 && LFA_DW_NAN == 1 && LFA_DW_GAVE_UP == 2 && LFA_DW_RHS == 3 && LFA_DW_SOLVER_WORDS == 4,
              "pcg_state: the reset covers exactly the four solver words");
static_assert(LFA_DW_N_DTILES == LFA_DW_N_PTILES + 1, "pcg_state: the two tile counts are read back as one block");
static_assert(LFA_DW_N_UNKNOWNS < LFA_DW_SLAB_MARKS && LFA_DW_SLAB_MARKS + 4 == LFA_DW_SLAB_MARKS_END &&
                  LFA_DW_SLAB_MARKS_END <= LFA_DW_RESIDUAL && LFA_DW_READBACK_WORDS <= LFA_DW_SLAB,
              "pcg_state: the layer marks and the slab block overlap another claim");
static_assert(LFA_SLAB_MARK_SCAN + 4 == LFA_SLAB_N_DTILES && LFA_SLAB_N_HALO + 4 == LFA_SLAB_WORDS, "slab block: four marks, four lists");

// ---------------------------------------------------------------------------------------------------- lfa_sim::h_pinned
// Pinned host words (uint32) that device scalars are read back through; host-only, so no two claims share a word.
enum {
	LFA_PIN_STATE = 0,               // pcg.hip: the LFA_DW_READBACK_WORDS state words of a solve [0, 20)
	LFA_PIN_SLAB = 20,               // core.hip: the slab binning's LFA_SLAB_WORDS totals [20, 30)
	LFA_PIN_N_UNKNOWNS = 32,         // core.hip: lfa_number_unknowns
	LFA_PIN_LAST_RESIDUAL = 34,      // pcg.hip: the residual of a capped solve, a double [34, 36)
	LFA_PIN_NP_LIVE = 36,            // core.hip, binning: live particles
	LFA_PIN_N_PTILES = 37,           // core.hip, binning of a single domain: particle tiles ...
	LFA_PIN_N_DTILES = 38,           // ... and processed tiles (one 8-byte copy)
	LFA_PIN_MG_COUNTS = 64,          // mg.hip: tiles per level, LFA_MAX_MG_LEVELS words [64, 76)
	LFA_PIN_SOURCE_TOTAL = 96,       // lfa_update_sources: particles the own entries create
	LFA_PIN_SEED_ACCEPTED = 97,      // lfa_seed_box / _sphere: accepted candidates of the whole job ...
	LFA_PIN_SEED_OWNED = 98,         // ... and those of them this rank keeps
	LFA_PIN_RESIDENT = 99,           // lfa_particles_close_holes: resident records
	LFA_PIN_VMAX2_BITS = 100,        // grid_ops.hip -> lfa_cfl: max |v|^2 as float bits
	LFA_PIN_SOURCE_TOTAL_ALL = 104,  // collective lfa_update_sources_rng: particles the whole job creates ...
	LFA_PIN_SOURCE_KEPT = 105,       // ... and those of them this rank keeps
	LFA_PIN_SAMPLE_OWNED = 106,      // lfa_sample_velocity_collective: points this rank owns ...
	LFA_PIN_SAMPLE_OUTSIDE = 107,    // ... and points outside the grid
	LFA_PIN_TRACER_COUNTS = 108,     // lfa_tracers_step: tracers stopped in the march, and (109) tracers frozen
	LFA_PIN_TRACER_KEPT = 110,       // lfa_tracers_add_collective: tracers of the list this rank keeps
	LFA_PIN_TRACER_MIGRATE = 112,    // tracers.hip, a round of the slab migration: leaving down / up, staying, arriving from
	                                 // below / above, lowest / highest destination layer (int32) [112, 119)
	LFA_PIN_TRACER_ROUNDS = 120,     // ... and the job's round count, a double [120, 122)
	LFA_PIN_COUNT = 122,
	LFA_PIN_BYTES = 4096,            // the allocation
};
static_assert(LFA_PIN_STATE + LFA_DW_READBACK_WORDS <= LFA_PIN_SLAB && LFA_PIN_SLAB + LFA_SLAB_WORDS <= LFA_PIN_N_UNKNOWNS,
              "h_pinned: the state and slab blocks overlap the next claim");
static_assert(LFA_PIN_LAST_RESIDUAL % 2 == 0 && LFA_PIN_LAST_RESIDUAL + 2 <= LFA_PIN_NP_LIVE, "h_pinned: the residual is an aligned double");
static_assert(LFA_PIN_N_DTILES == LFA_PIN_N_PTILES + 1, "h_pinned: the two tile counts arrive as one block");
static_assert(LFA_PIN_MG_COUNTS + LFA_MAX_MG_LEVELS <= LFA_PIN_SOURCE_TOTAL, "h_pinned: the level counts run into the next claim");
static_assert(LFA_PIN_TRACER_KEPT >= LFA_PIN_TRACER_COUNTS + 2 && LFA_PIN_TRACER_MIGRATE + 7 <= LFA_PIN_TRACER_ROUNDS &&
                  LFA_PIN_TRACER_ROUNDS % 2 == 0 && LFA_PIN_TRACER_ROUNDS + 2 <= LFA_PIN_COUNT,
              "h_pinned: the tracer migration's words overlap, or its round count is no aligned double");
static_assert(LFA_PIN_COUNT * 4 <= LFA_PIN_BYTES, "h_pinned: a claim lies beyond the allocation");

// ---------------------------------------------------------------------------------------------------- lfa_sim::dist_red
// Device doubles of a slab run (dist.hip). (LFA_RED_* are the reduce types.)
enum {
	LFA_DR_MAX_RANKS = 32,
	LFA_DR_B2 = 0,              // solver: sum b^2
	LFA_DR_ZS = 1,              // solver: q . s
	LFA_DR_RMAX = 2,            // solver: max |r|
	LFA_DR_SIGMA = 3,           // solver: sigma, + parity [3, 5)
	LFA_DR_SOURCE_TOTALS = 16,  // particles.hip, lfa_update_sources: one slot per rank. Beyond 16 ranks it runs into the two claims
	                            // below; each of the three is written, reduced and read back inside one call
	LFA_DR_MIGRATE_COUNTS = 32,  // dist.hip, lfa_dist_migrate: five uint32 - leaving lo / hi, arriving from lo / hi, beyond reach
	LFA_DR_GHOST_TOTALS = 40,   // dist.hip, ghost particles: two uint32 - arriving from below / above
	LFA_DR_TRACER_ROUNDS = 42,  // tracers.hip, lfa_tracers_advect_collide_collective: the job's round count (max over the ranks' hop
	                            // distances) and, behind it, this rank's own [42, 44)
	LFA_DR_GATHER = 64,         // two gather buffers (parity), each [max | sum | sum2 per rank | given up]: lfa_dist_gather_buf
	LFA_DR_GATHER_LEN = 3 * LFA_DR_MAX_RANKS + 1,
	LFA_DR_ALPHA = LFA_DR_GATHER + 2 * LFA_DR_GATHER_LEN,  // alpha of the single-reduction CG (2) and room behind it
	LFA_DR_COUNT = LFA_DR_ALPHA + 8,
};
static_assert(LFA_DR_SIGMA + 2 <= LFA_DR_SOURCE_TOTALS && LFA_DR_GHOST_TOTALS + 1 <= LFA_DR_GATHER, "dist_red: scalars overlap");
static_assert(LFA_DR_GHOST_TOTALS + 1 <= LFA_DR_TRACER_ROUNDS && LFA_DR_TRACER_ROUNDS + 2 <= LFA_DR_GATHER && LFA_DR_GATHER <= LFA_DR_COUNT,
              "dist_red: the tracer round count overlaps another claim or lies beyond the allocation");

// ---------------------------------------------------------------------------------------------------- lfa_sim::pcg_hist
enum {
	LFA_HIST_LEN = 4096,         // [0, 4096): the residual of every iteration
	LFA_HIST_BENCH_SINK = 4095,  // lfa_bench_kernel: where its launch of k_pcg_a leaves its residual
	LFA_HIST_COARSE = 6144,      // pcg.hip: the coarse solve's r2 hand-off (coarse_args)
	LFA_HIST_COUNT = 8192,       // doubles allocated
};
static_assert(LFA_HIST_BENCH_SINK < LFA_HIST_LEN && LFA_HIST_LEN <= LFA_HIST_COARSE && LFA_HIST_COARSE < LFA_HIST_COUNT, "pcg_hist layout");

// ---------------------------------------------------------------------------------------------------- lfa_sim::ev
// Timing events (lfa_enable_timing creates them; lfa_stream_set parks them between handles).
enum {
	// boundaries of lfa_step_hot, in stream order
	LFA_EV_HOT_START = 0, LFA_EV_HOT_BIN, LFA_EV_HOT_P2G, LFA_EV_HOT_GRAVITY, LFA_EV_HOT_ALLOC, LFA_EV_HOT_SOLVE, LFA_EV_HOT_APPLY,
	LFA_EV_HOT_EXTRAP, LFA_EV_HOT_G2P,
	// recorded inside the stages, read by both step drivers
	LFA_EV_SCATTER_BEGIN = 16, LFA_EV_SCATTER_END,  // p2g.hip: around the scatter kernel
	LFA_EV_SYSTEM_BUILT,                            // pcg.hip: end of the system build, inside a non-trivial solve
	LFA_EV_BENCH_BEGIN = 20, LFA_EV_BENCH_END,      // lfa_bench_kernel
	// boundaries of lfa_time_step; LFA_EV_STEP_CORRECT is also the end of a correction on its own stream (correct_begin)
	LFA_EV_STEP_START = 24, LFA_EV_STEP_ADVECT, LFA_EV_STEP_BIN, LFA_EV_STEP_P2G, LFA_EV_STEP_SOLVE, LFA_EV_STEP_APPLY,
	LFA_EV_STEP_CORRECT, LFA_EV_STEP_EXTRAP, LFA_EV_STEP_G2P, LFA_EV_STEP_JOIN,
	// the position correction, on whichever stream it runs: start | cell index built | tiled kernel done
	LFA_EV_CORR_BEGIN = 40, LFA_EV_CORR_INDEXED, LFA_EV_CORR_TILED,
	LFA_EV_COUNT = 48,
};
static_assert(LFA_EV_HOT_G2P < LFA_EV_SCATTER_BEGIN && LFA_EV_SYSTEM_BUILT < LFA_EV_BENCH_BEGIN && LFA_EV_BENCH_END < LFA_EV_STEP_START &&
                  LFA_EV_STEP_JOIN < LFA_EV_CORR_BEGIN && LFA_EV_CORR_TILED < LFA_EV_COUNT,
              "ev: two groups of events overlap");

// ---------------------------------------------------------------------------------------------------- lfa_sim::ms, ms_next
// The timer indices are public (include/libfluid_amd.h: LFA_TIMER_*, LFA_STEP_TIMER_*)
static_assert(LFA_TIMER_PCG_ITERATION_MEAN + 1 == LFA_NUM_TIMERS && LFA_STEP_TIMER_OVERLAPPED + 1 == LFA_NUM_STEP_TIMERS,
              "the timer enums and their counts differ");
