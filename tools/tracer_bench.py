"""The tracer step against the route it replaces. Not bench.py: a measurement of two calls, on the lfa_seed_block block of the C2
configuration (libfluid_amd/scenes.py) after --steps lfa_time_steps, with --tracers tracers seeded from particle positions.

  device   lfa_tracers_time (HIP events around k_tracer_step) of lfa_tracers_step, median of --reps readings after one warm-up
           step; every reading follows a lfa_time_step, as in use. The kernel's achieved bytes - 97 per tracer (48 read, 49
           written) plus the grid reads, 24 fp32 samples per tracer, counted at 4 bytes each - as a fraction of the copy ceiling
           that lfa_bench_stream reports. The samples of neighbouring tracers share cache lines: the figure counts what the
           kernel asks for, not what reaches HBM.
  route    on the same points, what a host does today: the wall time of one lfa_sample_velocity call (24 bytes per point up, the
           kernel, 24 down; host clock around a call that ends in a synchronise), and lfa_sample_velocity_time, the kernel alone.
           The host's own move and collision handling, and the lfa_download_cells it needs for the obstacles, come on top and are
           not timed here.
The child process runs under a time limit; a failure ends the measurement. One JSON line.

    python tools/tracer_bench.py [--config C2] [--steps 20] [--tracers 1048576] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = {"C1": 120, "C2": 300, "C3": 500, "C4": 900}


def child(name, steps, n_tracers, reps):
    import numpy as np
    import libfluid_amd as lfa
    from libfluid_amd import scenes
    cfg = scenes.CONFIGS[name]
    size, (lo, hi) = cfg["size"], cfg["block"]
    sim = lfa.Sim(size, method=cfg["method"], blending=cfg["blending"], gravity=(0.0, -981.0, 0.0))
    sim.seed_block(lo, hi)

    def step():
        dt = min(3.0 * sim.cfl(), 0.004)
        assert sim.time_step(dt)[2] >= 0
        return dt

    for _ in range(steps):
        step()
    pos = sim.positions()
    rng = np.random.default_rng(20261020)
    pts = np.ascontiguousarray(pos[rng.choice(len(pos), size=n_tracers, replace=len(pos) < n_tracers)])
    sim.add_tracers(pts)
    sim.tracers_transfer()
    sim.tracers_step(step())  # warm-up: the code object is loaded
    tracer_ms, stopped = [], 0
    for _ in range(reps):
        dt = step()
        stopped += sim.tracers_step(dt)[0]
        tracer_ms.append(sim.tracers_ms())
    # the route this replaces, on the tracers' current positions
    pts = sim.tracers()[0]
    sim.sample_velocity(pts)  # warm-up: the staging buffer is allocated
    route_wall, route_kernel = [], []
    for _ in range(reps):
        sim.synchronize()
        t0 = time.perf_counter()
        vel, _ = sim.sample_velocity(pts)
        route_wall.append(1e3 * (time.perf_counter() - t0))
        route_kernel.append(sim.sample_velocity_ms())
    same = bool(np.array_equal(vel, sim.tracers()[1]))  # the tracers' velocities are that sample, bit for bit
    copy_gbs, read_gbs = sim.bench_stream()
    sim.close()
    med = statistics.median
    n = len(pts)
    asked = (97.0 + 24 * 4.0) * n
    out = {"config": name, "grid": list(size), "particles": len(pos), "tracers": n, "steps": steps, "reps": reps,
           "tracer_step_device_ms": med(tracer_ms), "tracer_step_device_ms_min_max": [min(tracer_ms), max(tracer_ms)],
           "stopped_per_step": stopped / reps,
           "bytes_per_tracer": 97, "grid_bytes_per_tracer_asked": 96, "copy_ceiling_gbs": copy_gbs, "read_ceiling_gbs": read_gbs,
           "achieved_gbs_tracer_arrays": 97.0 * n / (med(tracer_ms) * 1e-3) / 1e9,
           "fraction_of_copy_ceiling_tracer_arrays": 97.0 * n / (med(tracer_ms) * 1e-3) / (copy_gbs * 1e9),
           "fraction_of_copy_ceiling_with_grid_reads": asked / (med(tracer_ms) * 1e-3) / (copy_gbs * 1e9),
           "route_sample_velocity_wall_ms": med(route_wall), "route_sample_velocity_wall_ms_min_max": [min(route_wall), max(route_wall)],
           "route_sample_velocity_kernel_ms": med(route_kernel), "same_velocities": same}
    print(json.dumps(out), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tracers", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.tracers, args.reps)
    cmd = ["timeout", "-k", "10", str(LIMIT_S[args.config]), sys.executable, os.path.abspath(__file__), "--child", args.config, "--steps",
           str(args.steps), "--tracers", str(args.tracers), "--reps", str(args.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode == 0 and args.out:
        with open(args.out, "a") as f:
            f.write(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
