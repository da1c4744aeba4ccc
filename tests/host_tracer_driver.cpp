// Test driver for the tracers of the C++ host class (libfluid_amd/host/simulation.h): the grid of tests/sample_cases.py (40 x 24 x 17,
// cell size 0.3, offset (0.69, -0.35, 15.3)) with a seeded box and the tracers the test hands in takes three time_step(dt)s with a
// fixed dt; the tracers' state is then read BEFORE grid() is downloaded. Three runs: "fused" (no callbacks: a step is one
// lfa_time_step and one lfa_tracers_step), "staged" (a post_gravity_callback that does nothing: the stages one by one, the tracers
// after the G2P) and "off" (advance_tracers = false: the tracers stay where they were added).
// Built and run by tests/test_host_tracers.py, which compares what is written here.
//   usage: host_tracer_driver outdir      (reads outdir/tracers.bin: double[3 n] positions, then double[3 n] velocities)
//   writes, for <tag> = fused, staged, off:
//     outdir/<tag>_pos.bin, outdir/<tag>_vel.bin  double[3 n]     outdir/<tag>_types.bin  u8[n]
//     outdir/<tag>_grid.bin  grid() (32-byte cells, x fastest)    outdir/<tag>_calls.bin  u64: times the callback ran
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../libfluid_amd/host/simulation.h"

using fluid_amd::mac_grid;
using fluid_amd::simulation;
using fluid_amd::vec3d;
using fluid_amd::vec3s;

static bool put(const std::string &path, const void *data, std::size_t bytes) {
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const bool ok = bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes;
	std::fclose(f);
	return ok;
}

static bool get_tracers(const std::string &path, std::vector<vec3d> &pos, std::vector<vec3d> &vel) {
	FILE *f = std::fopen(path.c_str(), "rb");
	if (!f) return false;
	std::vector<vec3d> all;
	vec3d p;
	while (std::fread(&p, sizeof(p), 1, f) == 1) all.push_back(p);
	std::fclose(f);
	if (all.empty() || all.size() % 2) return false;
	pos.assign(all.begin(), all.begin() + static_cast<std::ptrdiff_t>(all.size() / 2));
	vel.assign(all.begin() + static_cast<std::ptrdiff_t>(all.size() / 2), all.end());
	return true;
}

static int run(const std::string &outdir, const std::string &tag, const std::vector<vec3d> &pos0, const std::vector<vec3d> &vel0, bool staged,
               bool advance) {
	const double h = 0.3, dt = 0.005;
	simulation sim;
	sim.resize(vec3s(40, 24, 17));
	sim.grid_offset = vec3d(0.69, -0.35, 15.3);
	sim.cell_size = h;
	sim.gravity = vec3d(0.3, -981.0, 0.1);
	if (sim.last_status() < 0) {
		std::printf("no device: %s\n", sim.last_error().c_str());
		return 1;
	}
	std::uint64_t calls = 0;
	if (staged) sim.post_gravity_callback = [&calls](double) { ++calls; };
	sim.advance_tracers = advance;
	sim.particles().clear();
	sim.seed_box(sim.grid_offset + vec3d(2, 2, 2) * h, vec3d(9, 7, 6) * h);
	sim.reset_space_hash();
	// in two batches: the second one grows the arrays with the first one alive
	const std::size_t half = pos0.size() / 2;
	const std::vector<vec3d> pa(pos0.begin(), pos0.begin() + static_cast<std::ptrdiff_t>(half)), pb(pos0.begin() + static_cast<std::ptrdiff_t>(half), pos0.end());
	const std::vector<vec3d> va(vel0.begin(), vel0.begin() + static_cast<std::ptrdiff_t>(half)), vb(vel0.begin() + static_cast<std::ptrdiff_t>(half), vel0.end());
	sim.add_tracers(pa, &va);
	sim.add_tracers(pb, &vb);
	if (sim.last_status() < 0 || sim.tracer_count() != pos0.size()) {
		std::printf("%s: add_tracers failed: %s\n", tag.c_str(), sim.last_error().c_str());
		return 2;
	}
	for (int step = 1; step <= 3; ++step) {
		sim.time_step(dt);
		if (sim.last_status() < 0) {
			std::printf("%s: step %d failed: %s\n", tag.c_str(), step, sim.last_error().c_str());
			return 3;
		}
	}
	std::vector<vec3d> pos, vel;
	std::vector<unsigned char> types;
	sim.tracers(pos, &vel, &types);
	if (sim.last_status() < 0 || pos.size() != pos0.size() || vel.size() != pos0.size() || types.size() != pos0.size()) {
		std::printf("%s: tracers() failed: %s\n", tag.c_str(), sim.last_error().c_str());
		return 4;
	}
	const simulation &csim = sim;
	const fluid_amd::grid3<mac_grid::cell> &g = csim.grid().grid();
	static_assert(sizeof(mac_grid::cell) == 32, "cells are the reference's 32-byte records");
	const vec3s n = g.get_size();
	const std::string base = outdir + "/" + tag;
	if (!put(base + "_pos.bin", pos.data(), sizeof(vec3d) * pos.size()) || !put(base + "_vel.bin", vel.data(), sizeof(vec3d) * vel.size()) ||
	    !put(base + "_types.bin", types.data(), types.size()) || !put(base + "_grid.bin", &g[0], sizeof(mac_grid::cell) * n.x * n.y * n.z) ||
	    !put(base + "_calls.bin", &calls, 8))
		return 5;
	sim.clear_tracers();
	return sim.tracer_count() == 0 ? 0 : 6;
}

int main(int argc, char **argv) {
	if (argc < 2) return 64;
	const std::string outdir = argv[1];
	std::vector<vec3d> pos, vel;
	if (!get_tracers(outdir + "/tracers.bin", pos, vel)) return 65;
	if (int rc = run(outdir, "fused", pos, vel, false, true)) return rc;
	if (int rc = run(outdir, "staged", pos, vel, true, true)) return 10 + rc;
	if (int rc = run(outdir, "off", pos, vel, false, false)) return 20 + rc;
	return 0;
}
