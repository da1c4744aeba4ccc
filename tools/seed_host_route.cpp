// The route a scene took to the device before lfa_seed_box existed, timed: the host loop of fluid_amd::simulation::seed_box
// (a sequential pcg32, one 152-byte record per particle) and lfa_upload_particles of its records. Wall time; the upload ends in a
// device synchronise. Built and run by tools/seed_probe.py.
//   usage: seed_host_route nx ny nz bx by bz density       (cell size 1, the box [0, b) in world units)
//   prints one line: particles host_loop_ms upload_ms generator_state_after
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../libfluid_amd/host/simulation.h"

int main(int argc, char **argv) {
	if (argc < 8) return 64;
	using clk = std::chrono::steady_clock;
	auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
	fluid_amd::simulation sim;
	sim.resize(fluid_amd::vec3s(std::strtoull(argv[1], nullptr, 10), std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10)));
	sim.cell_size = 1.0;
	if (sim.last_status() < 0 || !sim.device_handle()) {
		std::fprintf(stderr, "no device: %s\n", sim.last_error().c_str());
		return 1;
	}
	lfa_params p;
	lfa_default_params(&p);
	p.cell_size = sim.cell_size;
	if (lfa_set_params(sim.device_handle(), &p) < 0) return 1;
	const auto t0 = clk::now();
	sim.seed_box(fluid_amd::vec3d(), fluid_amd::vec3d(std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6])), fluid_amd::vec3d(),
	             std::strtoull(argv[7], nullptr, 10));
	const auto t1 = clk::now();
	const auto &parts = static_cast<const fluid_amd::simulation &>(sim).particles();
	if (lfa_upload_particles(sim.device_handle(), parts.data(), parts.size()) < 0 || lfa_synchronize(sim.device_handle()) < 0) {
		std::fprintf(stderr, "upload failed: %s\n", lfa_last_error(sim.device_handle()));
		return 1;
	}
	const auto t2 = clk::now();
	std::printf("%zu %.3f %.3f %llu\n", parts.size(), ms(t0, t1), ms(t1, t2), (unsigned long long)sim.random.state());
	return 0;
}
