// Test driver for fluid_amd::mesher::generate_mesh_with_normals (libfluid_amd/host/mesher.h): what testbed/main.cpp:224-225 does
// in two calls (generate_mesh, mesh.generate_normals()) in one, with the normals computed on the device. Built and run by
// tests/test_host_mesher_normals.py, against the standalone value types and against the reference's own (fluid::mesh).
//   usage: host_normals_driver particles.bin nx ny nz ox oy oz cell_size extent radius r mesh_out.bin
//          host_normals_driver sim n r mesh_out.bin       (a block of fluid in an n^3 simulation, two steps, mesher cells n/2)
//   particles.bin = double[3 n]; mesh_out.bin = u64 nv, u64 ni, double[3 nv] positions, u64[ni], double[3 nv] normals
// Exit code 5: the device's normals are not byte-identical to mesh_t::generate_normals() of the same mesh (NaN beside NaN
// counts as identical: a NaN's sign and payload differ between processors and are no part of the contract).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../libfluid_amd/host/mesher.h"

using namespace fluid_amd;

static int check_and_write(mesher &m, const mesher::mesh_t &mesh, const mesher::mesh_t &plain, const char *path) {
	if (m.last_status() != LFA_OK) {
		std::fprintf(stderr, "mesher failed: %s\n", m.last_error().c_str());
		return 3;
	}
	// generate_mesh itself is untouched: the same mesh, no normals
	if (!plain.normals.empty() || plain.indices != mesh.indices || plain.positions.size() != mesh.positions.size() ||
	    std::memcmp(plain.positions.data(), mesh.positions.data(), 24 * mesh.positions.size()) != 0) return 4;
	if (mesh.normals.size() != mesh.positions.size()) return 6;
	mesher::mesh_t host = mesh;
	host.generate_normals();
	const double *a = reinterpret_cast<const double *>(host.normals.data()), *b = reinterpret_cast<const double *>(mesh.normals.data());
	for (std::size_t i = 0; i < 3 * mesh.normals.size(); ++i)
		if (std::memcmp(a + i, b + i, 8) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return 5;

	std::ofstream out(path, std::ios::binary);
	const std::uint64_t nv = mesh.positions.size(), ni = mesh.indices.size();
	out.write(reinterpret_cast<const char *>(&nv), 8);
	out.write(reinterpret_cast<const char *>(&ni), 8);
	out.write(reinterpret_cast<const char *>(mesh.positions.data()), 24 * nv);
	for (std::size_t i : mesh.indices) {
		const std::uint64_t v = i;
		out.write(reinterpret_cast<const char *>(&v), 8);
	}
	out.write(reinterpret_cast<const char *>(mesh.normals.data()), 24 * nv);
	return out.good() ? 0 : 7;
}

int main(int argc, char **argv) {
	if (argc >= 5 && std::string(argv[1]) == "sim") {
		const std::size_t n = static_cast<std::size_t>(std::atoi(argv[2]));
		simulation sim;
		sim.resize(vec3s(n, n, n));
		sim.grid_offset = vec3d();
		sim.cell_size = 1.0;
		sim.seed_box(vec3d(2.0, 1.0, 3.0), vec3d(0.4 * n, 0.45 * n, 0.35 * n));
		for (int k = 0; k < 2; ++k) sim.time_step(0.01);
		if (sim.last_status() != LFA_OK) {
			std::fprintf(stderr, "simulation failed: %s\n", sim.last_error().c_str());
			return 3;
		}
		mesher m;  // testbed/main.cpp:101-107: mesher cells half a simulation cell
		m.resize(vec3s(2 * n, 2 * n, 2 * n));
		m.grid_offset = vec3d();
		m.cell_size = 0.5;
		m.particle_extent = 1.0;
		m.cell_radius = 3;
		const double r = std::atof(argv[3]);
		mesher::mesh_t mesh = m.generate_mesh_with_normals(sim, r);
		mesher::mesh_t plain = m.generate_mesh(sim, r);
		return check_and_write(m, mesh, plain, argv[4]);
	}
	if (argc < 13) return 2;
	std::ifstream in(argv[1], std::ios::binary);
	std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	const double *d = reinterpret_cast<const double *>(raw.data());
	std::vector<vec3d> pts(raw.size() / 24);
	for (std::size_t i = 0; i < pts.size(); ++i) pts[i] = vec3d(d[3 * i], d[3 * i + 1], d[3 * i + 2]);

	mesher m;
	m.resize(vec3s(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
	m.grid_offset = vec3d(std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7]));
	m.cell_size = std::atof(argv[8]);
	m.particle_extent = std::atof(argv[9]);
	m.cell_radius = static_cast<std::size_t>(std::atoi(argv[10]));
	const double r = std::atof(argv[11]);
	mesher::mesh_t mesh = m.generate_mesh_with_normals(pts, r);
	mesher::mesh_t plain = m.generate_mesh(pts, r);
	return check_and_write(m, mesh, plain, argv[12]);
}
