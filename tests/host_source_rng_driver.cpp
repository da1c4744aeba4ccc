// Test driver for sources_draw_from_random of the C++ host class (libfluid_amd/host/simulation.h): seed_box, two time_steps with
// a fluid source far above the box, seed_box again - once with the whole step in one device call, once with a callback installed
// (the staged step, whose callback also records the particles right after the seeding). Built and run by
// tests/test_host_source_rng.py, which compares what is written here with tests/source_model.py.
//   usage: host_source_rng_driver outdir
//   writes  outdir/<which>_box1.bin    particles() after the first seed_box
//           outdir/staged_seeded.bin   particles() inside post_particle_to_grid_transfer_callback of the first step
//           outdir/<which>_final.bin   particles() after the second seed_box
//   prints  "<which> state <after> <random.state()> <particles>"   after box1, step1, step2, box2
//           "off state <random.state() before> <after>"            one step with the flag off
#include <cstdio>
#include <memory>
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

static void report(const char *which, const char *after, const simulation &sim) {
	std::printf("%s state %s %llu %zu\n", which, after, (unsigned long long)sim.random.state(), sim.particles().size());
}

static int run(const std::string &outdir, const char *which, bool staged, bool draw) {
	simulation sim;
	sim.resize(vec3s(24, 24, 24));
	sim.cell_size = 0.5;
	sim.grid_offset = vec3d(0.25, -0.5, 1.0);
	sim.gravity = vec3d(0.0, -981.0, 0.0);
	sim.seed_on_device = true;
	sim.sources_draw_from_random = draw;
	if (sim.last_status() < 0) {
		std::printf("%s no device: %s\n", which, sim.last_error().c_str());
		return 1;
	}
	auto src = std::make_unique<fluid_amd::source>();
	for (std::size_t z = 8; z < 14; ++z)
		for (std::size_t x = 8; x < 14; ++x) src->cells.emplace_back(vec3s(x, 20, z));
	src->velocity = vec3d(0.0, -2.0, 0.0);
	src->target_density_cubic_root = 2;
	sim.sources.emplace_back(std::move(src));

	sim.particles().clear();
	sim.seed_box(sim.grid_offset + vec3d(1.1, 0.3, 2.2), vec3d(4.7, 2.2, 3.9), vec3d(0.0, 0.0, 0.0), 2);
	if (!draw) {  // the flag off: a step's sources leave `random` alone
		const unsigned long long before = sim.random.state();
		sim.time_step(0.005);
		std::printf("off state %llu %llu\n", before, (unsigned long long)sim.random.state());
		return sim.last_status() < 0 ? 3 : 0;
	}
	report(which, "box1", sim);
	if (!dump(outdir + "/" + which + "_box1.bin", static_cast<const simulation &>(sim).particles())) return 2;
	int step = 0;
	bool dumped = true;
	if (staged)
		sim.post_particle_to_grid_transfer_callback = [&](double) {
			if (step == 0) dumped = dump(outdir + "/staged_seeded.bin", static_cast<const simulation &>(sim).particles());
		};
	sim.time_step(0.005);
	report(which, "step1", sim);
	++step;
	sim.time_step(0.005);
	report(which, "step2", sim);
	sim.seed_box(sim.grid_offset + vec3d(7.0, 4.0, 7.0), vec3d(2.0, 1.5, 2.0), vec3d(0.0, 1.0, 0.0), 3);
	report(which, "box2", sim);
	if (sim.last_status() < 0) {
		std::printf("%s error: %s\n", which, sim.last_error().c_str());
		return 3;
	}
	if (!dumped || !dump(outdir + "/" + which + "_final.bin", static_cast<const simulation &>(sim).particles())) return 2;
	return 0;
}

int main(int argc, char **argv) {
	if (argc < 2) return 64;
	int rc = run(argv[1], "single", false, true);
	rc = rc ? rc : run(argv[1], "staged", true, true);
	return rc ? rc : run(argv[1], "off", false, false);
}
