// Test driver for frame_stats() / positions() of the C++ host class (libfluid_amd/host/simulation.h): the testbed's scene 3
// (testbed/main.cpp:163-165, scaled to a 24^3 grid) takes three time_step()s; after each one the device summary is taken FIRST,
// then particles() is downloaded and the testbed's own loops (update_simulation, testbed/main.cpp:50-88; the maximum of
// :117-123) run over it. Then one particle is moved through particles(), and the summary has to see the edit.
// Built and run by tests/test_host_frame.py, which compares what is written here.
//   usage: host_frame_driver outdir
//   writes, for <tag> = step1, step2, step3, edit:
//     outdir/<tag>_stats.bin      struct lfa_frame_stats          outdir/<tag>_occupation.bin  u64[nx ny nz] of frame_stats()
//     outdir/<tag>_positions.bin  double[3 n] of positions()      outdir/<tag>_particles.bin   particles() (152-byte records)
//     outdir/<tag>_host.bin       double energy, double max |v|^2, then u64[nx ny nz]: the loops over particles()
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../libfluid_amd/host/simulation.h"

using fluid_amd::simulation;
using fluid_amd::vec3d;
using fluid_amd::vec3i;
using fluid_amd::vec3s;

static bool put(const std::string &path, const void *data, std::size_t bytes) {
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const bool ok = bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes;
	std::fclose(f);
	return ok;
}

static bool record(simulation &sim, const std::string &outdir, const std::string &tag) {
	const std::string base = outdir + "/" + tag;
	const simulation::frame_summary device = sim.frame_stats();
	std::vector<vec3d> points;
	sim.positions(points);
	if (sim.last_status() < 0) {
		std::printf("%s failed: %s\n", tag.c_str(), sim.last_error().c_str());
		return false;
	}
	const struct lfa_frame_stats &st = device;
	std::vector<std::uint64_t> occ;
	const vec3s n = device.occupation.get_size();
	for (std::size_t i = 0; i < n.x * n.y * n.z; ++i) occ.push_back(device.occupation[i]);
	if (!put(base + "_stats.bin", &st, sizeof(st)) || !put(base + "_occupation.bin", occ.data(), 8 * occ.size()) ||
	    !put(base + "_positions.bin", points.data(), sizeof(vec3d) * points.size()))
		return false;

	// ---- what the testbed does instead
	const simulation &csim = sim;
	const std::vector<simulation::particle> &particles = csim.particles();
	double energy = 0.0, fastest = 0.0;
	for (const simulation::particle &p : particles) {
		energy += 0.5 * p.velocity.squared_length();
		energy -= fluid_amd::vec_ops::dot(sim.gravity, p.position);
		fastest = std::max(fastest, p.velocity.squared_length());
	}
	fluid_amd::grid3<std::size_t> grid(csim.grid().grid().get_size(), 0);
	for (const simulation::particle &p : particles) {
		vec3s cell(vec3i((p.position - sim.grid_offset) / sim.cell_size));
		if (cell.x < grid.get_size().x && cell.y < grid.get_size().y && cell.z < grid.get_size().z) ++grid(cell);
	}
	std::vector<std::uint64_t> host(2 + n.x * n.y * n.z);
	static_assert(sizeof(double) == sizeof(std::uint64_t), "doubles are stored beside the counts");
	std::memcpy(&host[0], &energy, 8);
	std::memcpy(&host[1], &fastest, 8);
	for (std::size_t i = 0; i < n.x * n.y * n.z; ++i) host[2 + i] = grid[i];
	return put(base + "_host.bin", host.data(), 8 * host.size()) &&
	       put(base + "_particles.bin", particles.data(), sizeof(simulation::particle) * particles.size());
}

int main(int argc, char **argv) {
	if (argc < 2) return 64;
	const std::string outdir = argv[1];
	const double s = 24.0 / 50.0;  // the testbed's coordinates are for 50^3
	simulation sim;
	sim.resize(vec3s(24, 24, 24));
	sim.grid_offset = vec3d();
	sim.cell_size = 1.0;
	sim.gravity = vec3d(0.0, -981.0, 0.0);
	if (sim.last_status() < 0) {
		std::printf("no device: %s\n", sim.last_error().c_str());
		return 1;
	}
	sim.particles().clear();
	sim.seed_box(vec3d(0, 0, 0), vec3d(10, 50, 50) * s);
	sim.reset_space_hash();
	for (int step = 1; step <= 3; ++step) {
		sim.time_step();
		if (sim.last_status() < 0) {
			std::printf("step %d failed: %s\n", step, sim.last_error().c_str());
			return 1;
		}
		if (!record(sim, outdir, "step" + std::to_string(step))) return 2;
	}
	// an edit through particles() reaches the device before the summary is taken
	sim.particles()[0].position = vec3d(20.5, 21.5, 22.5);
	sim.particles()[0].old_position = sim.particles()[0].position;
	if (!record(sim, outdir, "edit")) return 2;
	return 0;
}
