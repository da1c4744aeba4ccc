// Test driver for seed_on_device of the C++ host class (libfluid_amd/host/simulation.h): the same scene - a sphere, then a box,
// the shape of the testbed's scene 2 (testbed/main.cpp:150-153) - seeded twice, by the host loop and on the device
// (lfa_seed_sphere / lfa_seed_box). Built and run by tests/test_host_seed.py, which compares what is written here.
//   usage: host_seed_driver outdir
//   writes  outdir/first_{host,device}.bin   particles() after the sphere and the box
//           outdir/second_{host,device}.bin  particles() after particles().clear() and one more seed_box
//   prints  "<which> draws <a> <b> <c>"      the next three draws of `random` after the first two seeding calls
//           "<which> update <last_status> <particles before> <particles after>"   one update(1/60) on the second set
#include <cstdio>
#include <string>
#include <vector>

#include "../libfluid_amd/host/simulation.h"

using fluid_amd::simulation;
using fluid_amd::vec3d;
using fluid_amd::vec3s;

static bool dump(const std::string &path, const std::vector<simulation::particle> &p) {
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const bool ok = p.empty() || std::fwrite(p.data(), sizeof(simulation::particle), p.size(), f) == p.size();
	std::fclose(f);
	return ok;
}

static int run(const std::string &outdir, const char *which, bool on_device) {
	simulation sim;
	sim.resize(vec3s(24, 24, 24));
	sim.cell_size = 0.5;
	sim.grid_offset = vec3d(0.25, -0.5, 1.0);
	sim.gravity = vec3d(0.0, -981.0, 0.0);
	sim.seed_on_device = on_device;
	if (sim.last_status() < 0) {
		std::printf("%s no device: %s\n", which, sim.last_error().c_str());
		return 1;
	}
	sim.particles().clear();  // the testbed's scene reset
	sim.seed_sphere(sim.grid_offset + vec3d(6.0, 10.4, 6.0), 1.3, vec3d(0.5, -2.0, 0.25));
	sim.seed_box(sim.grid_offset, vec3d(12.0, 3.6, 12.0), vec3d(-1.0, 0.0, 3.0), 2);
	if (sim.last_status() < 0) {
		std::printf("%s seeding failed: %s\n", which, sim.last_error().c_str());
		return 1;
	}
	const std::uint32_t a = sim.random(), b = sim.random(), c = sim.random();
	std::printf("%s draws %u %u %u\n", which, a, b, c);
	if (!dump(outdir + "/first_" + which + ".bin", sim.particles())) return 2;

	sim.particles().clear();
	sim.seed_box(sim.grid_offset + vec3d(1.1, 0.3, 2.2), vec3d(4.7, 5.2, 3.9), vec3d(0.0, 1.0, 0.0), 3);
	const std::vector<simulation::particle> second = static_cast<const simulation &>(sim).particles();
	if (!dump(outdir + "/second_" + which + ".bin", second)) return 2;
	sim.update(1.0 / 60.0);
	std::printf("%s update %d %zu %zu\n", which, sim.last_status(), second.size(), static_cast<const simulation &>(sim).particles().size());
	if (sim.last_status() < 0) std::printf("%s error: %s\n", which, sim.last_error().c_str());
	return 0;
}

int main(int argc, char **argv) {
	if (argc < 2) return 64;
	const int rc = run(argv[1], "host", false);
	return rc ? rc : run(argv[1], "device", true);
}
