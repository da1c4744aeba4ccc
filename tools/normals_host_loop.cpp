// Times fluid_amd::mesh::generate_normals() (libfluid_amd/host/mesh.h: the serial host loop, one thread as it is written) on
// a mesh file; the comparison leg of tools/normals_probe.py, which builds it with g++ -O2 like the tests build host code.
//   usage: normals_host_loop mesh.bin warmups reps [normals_out.bin]
//   mesh.bin = u64 nv, u64 ni, double[3 nv] positions, u64[ni] indices; prints the wall time of every repetition in ms
#define LFA_HOST_OWN_TYPES 1
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../libfluid_amd/host/mesh.h"

int main(int argc, char **argv) {
	if (argc < 4) return 2;
	std::ifstream in(argv[1], std::ios::binary);
	std::uint64_t nv = 0, ni = 0;
	in.read(reinterpret_cast<char *>(&nv), 8);
	in.read(reinterpret_cast<char *>(&ni), 8);
	fluid_amd::mesh<double, std::size_t, double, double, fluid_amd::vec3d> mesh;
	mesh.positions.resize(nv);
	in.read(reinterpret_cast<char *>(mesh.positions.data()), 24 * nv);
	std::vector<std::uint64_t> idx(ni);
	in.read(reinterpret_cast<char *>(idx.data()), 8 * ni);
	if (!in) return 3;
	mesh.indices.assign(idx.begin(), idx.end());
	const int warmups = std::atoi(argv[2]), reps = std::atoi(argv[3]);
	for (int k = 0; k < warmups + reps; ++k) {
		const auto t0 = std::chrono::steady_clock::now();
		mesh.generate_normals();
		const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		if (k >= warmups) std::printf("%.6f\n", ms);
	}
	if (argc > 4) {
		std::ofstream out(argv[4], std::ios::binary);
		out.write(reinterpret_cast<const char *>(mesh.normals.data()), 24 * nv);
	}
	return 0;
}
