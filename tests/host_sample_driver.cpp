// Test driver for sample_velocity() of the C++ host class (libfluid_amd/host/simulation.h) and vertex_velocities() of the mesher
// (libfluid_amd/host/mesher.h): the grid of tests/sample_cases.py (40 x 24 x 17, cell size 0.3, offset (0.69, -0.35, 15.3)) with a
// seeded box takes three time_step()s; the grid's velocity is then sampled at the points the test hands in, BEFORE grid() is
// downloaded. Then one cell is edited through grid() and the sample is taken again without a step: it has to see the edit. Last,
// the surface is meshed from the resident particles and every vertex gets its velocity on the device.
// Built and run by tests/test_host_sample.py, which compares what is written here.
//   usage: host_sample_driver outdir      (reads outdir/points.bin: double[3 n])
//   writes, for <tag> = step3, edit:
//     outdir/<tag>_velocity.bin  double[3 n] of sample_velocity()     outdir/<tag>_types.bin  u8[n]
//     outdir/<tag>_outside.bin   u64 n_outside                        outdir/<tag>_grid.bin   grid() (32-byte cells, x fastest)
//   and outdir/mesh_positions.bin, mesh_vertex_velocities.bin, mesh_sampled.bin (double[3 nv] each), mesh_outside.bin (u64, u64)
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../libfluid_amd/host/mesher.h"
#include "../libfluid_amd/host/simulation.h"

using fluid_amd::mac_grid;
using fluid_amd::mesher;
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

static bool get_points(const std::string &path, std::vector<vec3d> &out) {
	FILE *f = std::fopen(path.c_str(), "rb");
	if (!f) return false;
	vec3d p;
	while (std::fread(&p, sizeof(p), 1, f) == 1) out.push_back(p);
	std::fclose(f);
	return !out.empty();
}

static bool record(simulation &sim, const std::vector<vec3d> &points, const std::string &outdir, const std::string &tag) {
	const std::string base = outdir + "/" + tag;
	std::vector<unsigned char> types;
	std::size_t outside = 0;
	const std::vector<vec3d> velocity = sim.sample_velocity(points, &types, &outside);
	if (sim.last_status() < 0 || velocity.size() != points.size() || types.size() != points.size()) {
		std::printf("%s failed: %s\n", tag.c_str(), sim.last_error().c_str());
		return false;
	}
	const std::uint64_t n_outside = outside;
	// ---- what a host does instead: the whole grid
	const simulation &csim = sim;
	const fluid_amd::grid3<mac_grid::cell> &g = csim.grid().grid();
	static_assert(sizeof(mac_grid::cell) == 32, "cells are the reference's 32-byte records");
	const vec3s n = g.get_size();
	return put(base + "_velocity.bin", velocity.data(), sizeof(vec3d) * velocity.size()) &&
	       put(base + "_types.bin", types.data(), types.size()) && put(base + "_outside.bin", &n_outside, 8) &&
	       put(base + "_grid.bin", &g[0], sizeof(mac_grid::cell) * n.x * n.y * n.z);
}

int main(int argc, char **argv) {
	if (argc < 2) return 64;
	const std::string outdir = argv[1];
	std::vector<vec3d> points;
	if (!get_points(outdir + "/points.bin", points)) return 65;
	const double h = 0.3;
	simulation sim;
	sim.resize(vec3s(40, 24, 17));
	sim.grid_offset = vec3d(0.69, -0.35, 15.3);
	sim.cell_size = h;
	sim.gravity = vec3d(0.3, -981.0, 0.1);
	if (sim.last_status() < 0) {
		std::printf("no device: %s\n", sim.last_error().c_str());
		return 1;
	}
	sim.particles().clear();
	sim.seed_box(sim.grid_offset + vec3d(2, 2, 2) * h, vec3d(9, 7, 6) * h);
	sim.reset_space_hash();
	for (int step = 1; step <= 3; ++step) {
		sim.time_step(0.005);
		if (sim.last_status() < 0) {
			std::printf("step %d failed: %s\n", step, sim.last_error().c_str());
			return 1;
		}
	}
	if (!record(sim, points, outdir, "step3")) return 2;
	// an edit through grid() reaches the device before the next sample, without a step in between
	sim.grid().grid()(vec3s(8, 8, 8)).velocities_posface = vec3d(1.25, -2.5, 3.75);
	if (!record(sim, points, outdir, "edit")) return 2;

	// ---- one velocity per vertex of the surface
	mesher m;
	m.resize(vec3s(44, 28, 21));
	m.cell_size = h;
	m.grid_offset = sim.grid_offset - vec3d(2, 2, 2) * h;  // (two cells larger than the simulation's box on every side)
	m.particle_extent = 2.0 * h;
	m.cell_radius = 3;
	const mesher::mesh_t mesh = m.generate_mesh(sim, 0.5 * h);
	std::size_t outside = 0, outside_sampled = 0;
	const std::vector<vec3d> on_device = m.vertex_velocities(sim, &outside);
	if (m.last_status() < 0 || on_device.size() != mesh.positions.size()) {
		std::printf("vertex_velocities failed: %s\n", m.last_error().c_str());
		return 3;
	}
	const std::vector<vec3d> sampled = sim.sample_velocity(mesh.positions, nullptr, &outside_sampled);
	if (sim.last_status() < 0) return 3;
	const std::uint64_t counts[2] = {outside, outside_sampled};
	if (!put(outdir + "/mesh_positions.bin", mesh.positions.data(), sizeof(vec3d) * mesh.positions.size()) ||
	    !put(outdir + "/mesh_vertex_velocities.bin", on_device.data(), sizeof(vec3d) * on_device.size()) ||
	    !put(outdir + "/mesh_sampled.bin", sampled.data(), sizeof(vec3d) * sampled.size()) || !put(outdir + "/mesh_outside.bin", counts, 16))
		return 3;
	return 0;
}
