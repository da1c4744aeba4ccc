"""The grid's velocity at points of the host's choosing: lfa_sample_velocity and lfa_mesher_vertex_velocities against the only route
there was before them - lfa_download_cells (32 bytes per cell) and a host loop over the points (here: the oracle's PIC transfer, one
thread of C). Not bench.py: a measurement of two calls, on the lfa_seed_block blocks of the C2 and C4 configurations
(libfluid_amd/scenes.py) after a few lfa_time_steps.

  device   lfa_sample_velocity_time (HIP events around the kernel) for --points uniform points in the box, and
           lfa_mesher_velocities_time for the vertices of that state's surface; warmed, median and spread of --reps calls; and what
           fraction of the measured copy ceiling (lfa_bench_stream) the floor of 48 bytes per point (24 read, 24 written) amounts
           to. The samples themselves are gathers from the grid on top of that floor.
  wall     lfa_sample_velocity including its two copies (24 bytes per point each way); today's route: lfa_download_cells, then the
           host loop (measured on at most 2^20 of the points and scaled to all of them).
The device and today's route must agree byte for byte on the points the host loop ran on. Every configuration runs in a child
process of its own under a time limit; a failure ends the probe. One JSON line per configuration and point count.

    python tools/sample_probe.py [--configs C2,C4] [--points 1048576,16777216] [--steps 3] [--reps 5] [--out FILE]
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
LIMIT_S = {"C1": 120, "C2": 300, "C3": 500, "C4": 1000}
HOST_LOOP_POINTS = 1 << 20


def child(name, steps, reps, counts):
    import numpy as np
    import libfluid_amd as lfa
    from libfluid_amd import scenes
    from oracle import loader as orc
    cfg = scenes.CONFIGS[name]
    size, (lo, hi) = cfg["size"], cfg["block"]
    sim = lfa.Sim(size, method=cfg["method"], blending=cfg["blending"])
    sim.seed_block(lo, hi)
    for _ in range(steps):
        dt = min(3.0 * sim.cfl(), 0.004)
        assert sim.time_step(dt)[2] >= 0
    sim.synchronize()
    med = statistics.median

    def timed(fn):
        sim.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return out, 1e3 * (time.perf_counter() - t0)

    copy_gbs, read_gbs = sim.bench_stream()
    cells, download_wall = timed(sim.cells)
    ok = True
    for n in counts:
        rng = np.random.default_rng(n)
        pts = rng.random((n, 3)) * np.array(size, dtype=np.float64)
        dev_ms, wall_ms = [], []
        for _ in range(1 + reps):
            (vel, n_out), w = timed(lambda: sim.sample_velocity(pts))
            dev_ms.append(sim.sample_velocity_ms())
            wall_ms.append(w)
        k = min(n, HOST_LOOP_POINTS)
        cpu = orc.CpuSim(size, method=orc.PIC)
        cpu.set_cells(cells)
        parts = np.zeros(k, dtype=lfa.PARTICLE_DTYPE)
        parts["pos"] = pts[:k]
        cpu.set_particles(parts)
        t0 = time.perf_counter()
        cpu.g2p()
        loop_ms = 1e3 * (time.perf_counter() - t0)
        same = bool(cpu.particles()["vel"].tobytes() == vel[:k].tobytes() and n_out == 0)
        cpu.close()
        ok = ok and same
        floor_bytes = 48.0 * n
        print(json.dumps({
            "config": name, "grid": list(size), "what": "points", "points": n, "steps": steps, "reps": reps,
            "device_ms": med(dev_ms[1:]), "device_ms_min_max": [min(dev_ms[1:]), max(dev_ms[1:])], "device_first_call_ms": dev_ms[0],
            "floor_bytes": floor_bytes, "copy_ceiling_gbs": copy_gbs, "read_ceiling_gbs": read_gbs,
            "fraction_of_copy_ceiling": floor_bytes / (med(dev_ms[1:]) * 1e-3) / (copy_gbs * 1e9),
            "wall_ms": med(wall_ms[1:]), "wall_first_call_ms": wall_ms[0],
            "today_download_cells_wall_ms": download_wall, "today_host_loop_points": k, "today_host_loop_wall_ms": loop_ms,
            "today_route_wall_ms_scaled": download_wall + loop_ms * (n / k), "same_results": same}), flush=True)
    # the vertices of this state's surface
    m = lfa.Mesher(size, particle_extent=2.0, cell_radius=3)  # (the testbed's mesher parameters)
    m.sample_sim(sim, 0.5)
    pos, idx = m.marching_cubes()
    dev_ms = []
    for _ in range(1 + reps):
        vvel, v_out = m.vertex_velocities(sim)
        dev_ms.append(m.velocities_ms())
    same = bool(vvel.tobytes() == sim.sample_velocity(pos)[0].tobytes() and np.isfinite(pos).all() and v_out == 0)
    ok = ok and same
    floor_bytes = 48.0 * len(pos)
    print(json.dumps({
        "config": name, "grid": list(size), "what": "mesh vertices", "points": len(pos), "outside": v_out, "steps": steps, "reps": reps,
        "device_ms": med(dev_ms[1:]), "device_ms_min_max": [min(dev_ms[1:]), max(dev_ms[1:])], "device_first_call_ms": dev_ms[0],
        "floor_bytes": floor_bytes, "copy_ceiling_gbs": copy_gbs,
        "fraction_of_copy_ceiling": floor_bytes / (max(med(dev_ms[1:]), 1e-6) * 1e-3) / (copy_gbs * 1e9), "same_results": same}), flush=True)
    m.close()
    sim.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--points", default="1048576,16777216")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.reps, [int(x) for x in args.points.split(",")])
    for name in args.configs.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps),
               "--reps", str(args.reps), "--points", args.points]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-4000:])
        if args.out and r.stdout:
            with open(args.out, "a") as f:
                f.write(r.stdout)
        if r.returncode != 0:  # nothing more is started on the device after a failure
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
