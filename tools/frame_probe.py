"""The per-frame read-out: lfa_frame_stats and lfa_download_positions against the route they replace - lfa_download_particles with
LFA_DL_POSITIONS and the hosts' loops over the records (here: tests/frame_model.py, numpy). Not bench.py: a measurement of three
calls, on the lfa_seed_block blocks of the C2 and C4 configurations (libfluid_amd/scenes.py) after a few lfa_time_steps.

  device   lfa_frame_stats_time (HIP events around the zeroing of the grid, the pass and the final sum) with and without the
           occupation grid, median of --reps calls, and what fraction of the measured copy ceiling (lfa_bench_stream) the 28 bytes
           per particle the pass reads amount to.
  wall     lfa_frame_stats including its read-backs (the scalars, the nx ny nz grid); lfa_download_positions (24 bytes per particle
           to the host); today's route: the 152-byte records to the device and back, then the loops. The first call of each of the
           two new ones allocates its staging buffer and is reported on its own.
The summary and the route it replaces must agree as tests/test_gpu_frame.py asks. Every configuration runs in a child process of
its own under a time limit; a failure ends the probe. One JSON line per configuration.

    python tools/frame_probe.py [--configs C2,C4] [--steps 3] [--reps 5] [--out FILE]
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
LIMIT_S = {"C1": 120, "C2": 240, "C3": 400, "C4": 900}


def child(name, steps, reps):
    import numpy as np
    import libfluid_amd as lfa
    from libfluid_amd import scenes
    from tests import frame_model as fm
    cfg = scenes.CONFIGS[name]
    size, (lo, hi) = cfg["size"], cfg["block"]
    gravity = (0.0, -981.0, 0.0)
    sim = lfa.Sim(size, method=cfg["method"], blending=cfg["blending"], gravity=gravity)
    sim.seed_block(lo, hi)
    for _ in range(steps):
        dt = min(3.0 * sim.cfl(), 0.004)
        assert sim.time_step(dt)[2] >= 0
    sim.synchronize()
    n = sim.num_particles
    med = statistics.median

    def timed(fn):
        sim.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return out, 1e3 * (time.perf_counter() - t0)

    grid_ms, grid_wall, nogrid_ms, nogrid_wall, pos_wall = [], [], [], [], []
    for _ in range(1 + reps):
        (st, occ), w = timed(sim.frame_stats)
        grid_ms.append(sim.frame_stats_ms())
        grid_wall.append(w)
        (st0, _), w = timed(lambda: sim.frame_stats(occupation=False))
        nogrid_ms.append(sim.frame_stats_ms())
        nogrid_wall.append(w)
        pos, w = timed(sim.positions)
        pos_wall.append(w)
    into = np.zeros(n, dtype=lfa.PARTICLE_DTYPE)
    d, today_download = timed(lambda: sim.download_particles(into=into, write_positions=True))
    t0 = time.perf_counter()
    m = fm.summary(d, size, (0.0, 0.0, 0.0), 1.0, gravity)
    today_loops = 1e3 * (time.perf_counter() - t0)
    bound = fm.energy_bound(n, m["energy_abs"])
    same = bool(st.n == m["n"] and st.n_in_grid == m["n_in_grid"] and np.array_equal(occ, m["occupation"]) and
                st.max_speed2 == m["max_speed2"] and np.array_equal(np.array(st.lo), m["lo"]) and np.array_equal(np.array(st.hi), m["hi"]) and
                abs(st.energy - m["energy"]) <= bound and abs(st.energy_abs - m["energy_abs"]) <= bound and
                bytes(memoryview(st)) == bytes(memoryview(st0)) and pos.tobytes() == np.ascontiguousarray(d["pos"]).tobytes())
    copy_gbs, read_gbs = sim.bench_stream()
    sim.close()
    read_bytes = 28.0 * n
    out = {"config": name, "grid": list(size), "particles": n, "steps": steps, "reps": reps,
           "device_ms_with_grid": med(grid_ms[1:]), "device_ms_with_grid_min_max": [min(grid_ms[1:]), max(grid_ms[1:])],
           "device_ms_without_grid": med(nogrid_ms[1:]), "device_ms_without_grid_min_max": [min(nogrid_ms[1:]), max(nogrid_ms[1:])],
           "bytes_read": read_bytes, "copy_ceiling_gbs": copy_gbs, "read_ceiling_gbs": read_gbs,
           "fraction_of_copy_ceiling_with_grid": read_bytes / (med(grid_ms[1:]) * 1e-3) / (copy_gbs * 1e9),
           "fraction_of_copy_ceiling_without_grid": read_bytes / (med(nogrid_ms[1:]) * 1e-3) / (copy_gbs * 1e9),
           "frame_stats_wall_ms": med(grid_wall[1:]), "frame_stats_first_call_wall_ms": grid_wall[0],
           "frame_stats_without_grid_wall_ms": med(nogrid_wall[1:]),
           "download_positions_wall_ms": med(pos_wall[1:]), "download_positions_first_call_wall_ms": pos_wall[0],
           "today_download_wall_ms": today_download, "today_loops_wall_ms": today_loops,
           "today_route_wall_ms": today_download + today_loops,
           "energy_difference": abs(st.energy - m["energy"]), "energy_bound": bound, "same_results": same}
    print(json.dumps(out), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.reps)
    for name in args.configs.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps),
               "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        sys.stderr.write(r.stderr[-4000:])
        if r.returncode != 0:  # nothing more is started on the device after a failure
            return r.returncode
        if args.out:
            with open(args.out, "a") as f:
                f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
