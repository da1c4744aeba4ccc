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
  slabs    --slabs 2,4,8: lfa_sample_velocity_collective on N virtual slabs of one GPU (in-process transport, one host thread per
           rank, the tile layers split evenly), every rank passing the same points: per rank the device time of its two passes
           (lfa_sample_velocity_time: every rank classifies every point), the points it owns, the wall time of the call and the wall
           time of a call with an empty list - the ghost refresh alone; beside them the single-domain collective call and the plain
           one. The ranks' rows must partition the points and agree with the single-domain run within the solver's fp32
           summation-order differences (tests/test_gpu_sample_slabs.py holds the bit-exact comparison, against the stitched grid).
The device and today's route must agree byte for byte on the points the host loop ran on. Every configuration runs in a child
process of its own under a time limit; a failure ends the probe. One JSON line per configuration and point count.

    python tools/sample_probe.py [--configs C2,C4] [--points 1048576,16777216] [--steps 3] [--reps 5] [--slabs 2,4,8] [--out FILE]
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


def on_ranks(sims, fn):
    """fn(rank, sim) on one host thread per rank (a collective call waits for its peers); the results in rank order."""
    import threading
    out, errors = [None] * len(sims), []

    def worker(r):
        try:
            out[r] = fn(r, sims[r])
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(len(sims))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise RuntimeError(str(errors))
    return out


def slab_child(name, steps, reps, counts, slabs):
    """The collective call on virtual slabs of configuration `name`: one JSON line per slab count and point count."""
    import numpy as np
    import libfluid_amd as lfa
    from libfluid_amd import scenes
    cfg = scenes.CONFIGS[name]
    size, (lo, hi) = cfg["size"], cfg["block"]
    layers = (size[2] + 7) // 8
    med = statistics.median
    dt = 0.002  # (a fixed step: the ranks of a job have to agree on it)

    def measure(sims, pts):
        """(per-rank median device ms, per-rank median wall ms, per-rank median wall ms of the empty call, owned, the last results)"""
        dev, wall, empty, res = [], [], [], None
        none = np.zeros((0, 3))

        def call(p):
            def fn(r, s):
                s.synchronize()
                t0 = time.perf_counter()
                out = s.sample_velocity_collective(p)
                return out, 1e3 * (time.perf_counter() - t0), (s.sample_velocity_ms() if len(p) else 0.0)
            return on_ranks(sims, fn)

        for _ in range(1 + reps):
            got = call(pts)
            res = [g[0] for g in got]
            wall.append([g[1] for g in got])
            dev.append([g[2] for g in got])
            empty.append([g[1] for g in call(none)])
        per_rank = lambda rows: [med(col) for col in zip(*rows[1:])]  # noqa: E731
        return per_rank(dev), per_rank(wall), per_rank(empty), [int(r[2][0]) for r in res], res

    # the single domain: the plain call and the collective one (local there)
    one = lfa.Sim(size, method=cfg["method"], blending=cfg["blending"])
    one.seed_block(lo, hi)
    for _ in range(steps):
        assert one.time_step(dt)[2] >= 0
    ok = True
    single = {}
    for n in counts:
        pts = np.random.default_rng(n).random((n, 3)) * np.array(size, dtype=np.float64)
        plain = []
        for _ in range(1 + reps):
            vel, _ = one.sample_velocity(pts)
            plain.append(one.sample_velocity_ms())
        dev, wall, empty, owned, res = measure([one], pts)
        ok = ok and bool(res[0][1].tobytes() == vel.tobytes() and owned[0] == n)
        single[n] = (vel, med(plain[1:]), [min(plain[1:]), max(plain[1:])], dev[0], wall[0])
    one.close()
    for n_ranks in slabs:
        bounds = [(r * layers) // n_ranks for r in range(n_ranks + 1)]
        hub = lfa.LocalHub(n_ranks)
        sims = [lfa.Sim(size, method=cfg["method"], blending=cfg["blending"]) for _ in range(n_ranks)]
        for r, sim in enumerate(sims):
            sim.init_local_slab(hub.h, r, bounds)
            sim.seed_block(lo, hi)

        def run(r, s):
            for _ in range(steps):
                assert s.time_step(dt)[2] >= 0
            s.hash()

        on_ranks(sims, run)
        for n in counts:
            pts = np.random.default_rng(n).random((n, 3)) * np.array(size, dtype=np.float64)
            dev, wall, empty, owned, res = measure(sims, pts)
            vel = np.full((n, 3), np.nan)
            for idx, v, _ in res:
                vel[idx] = v
            ref = single[n][0]
            diff = float(np.abs(vel - ref).max())
            scale = float(np.abs(ref).max())
            same = bool(sum(owned) == n and np.isfinite(vel).all() and diff <= 1e-2 * max(scale, 1.0))
            ok = ok and same
            print(json.dumps({
                "config": name, "grid": list(size), "what": "points, collective", "ranks": n_ranks, "bounds": bounds, "points": n,
                "steps": steps, "reps": reps, "rank_device_ms": dev, "rank_wall_ms": wall, "rank_refresh_only_wall_ms": empty,
                "rank_owned": owned, "single_domain_plain_device_ms": single[n][1], "single_domain_plain_device_ms_min_max": single[n][2],
                "single_domain_collective_device_ms": single[n][3], "single_domain_collective_wall_ms": single[n][4],
                "max_abs_difference_to_single_domain": diff, "max_abs_single_domain": scale, "partition_and_values_ok": same}), flush=True)
        for sim in sims:
            sim.close()
        hub.close()
    return 0 if ok else 1


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
    ap.add_argument("--slabs", default="", help="measure the collective call on these numbers of virtual slabs instead, e.g. 2,4,8")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child and args.slabs:
        return slab_child(args.child, args.steps, args.reps, [int(x) for x in args.points.split(",")], [int(x) for x in args.slabs.split(",")])
    if args.child:
        return child(args.child, args.steps, args.reps, [int(x) for x in args.points.split(",")])
    for name in args.configs.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name] * (2 if args.slabs else 1)), sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps),
               "--reps", str(args.reps), "--points", args.points] + (["--slabs", args.slabs] if args.slabs else [])
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
