"""Seeding a scene: lfa_seed_box on the device against the route it replaces - the host loop of fluid_amd::simulation::seed_box
and lfa_upload_particles of its 152-byte records (tools/seed_host_route.cpp). Not bench.py: a measurement of one call, on the
blocks of the C2 and C4 configurations (libfluid_amd/scenes.py) as seed_box(0, block size) at density 2, cell size 1.

  device  HIP events around the call on the handle's stream (the call reads one count back in the middle, so this is the time
          from its first kernel to its last, waits included), and the wall time of the call plus a synchronise. The first call on
          a handle also allocates the particle arrays; the repetitions after it (the handle emptied in between) do not.
  host    wall time of the loop, and of the upload up to a synchronise; one run (its upload allocates as well).
  slabs   --slabs 2,4,8: the same block seeded collectively (LFA_SEED_COLLECTIVE) on N virtual slabs of one GPU, the tile layers
          split evenly, one rank after the other (the call sends no message). Per rank: the event time of its call - a first call,
          which allocates the rank's share - and the particles resident afterwards. The route this replaces on a rank is the host
          route above, whole set and all (lfa_upload_particles hands every rank every particle): its time stands beside the ranks'.
Both routes must leave the same number of particles and the same generator state. Every configuration runs in a child process of
its own under a time limit; a failure ends the probe. One JSON line per configuration.

    python tools/seed_probe.py [--configs C2,C4] [--reps 5] [--slabs 2,4,8] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = {"C2": 240, "C4": 540}


class Events:
    """hipEvent timing on a given stream, through the HIP runtime libfluid_amd.so is linked to."""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            self.check(self.hip.hipEventCreate(C.byref(e)))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def start(self):
        self.check(self.hip.hipEventRecord(self.a, self.stream))

    def stop_ms(self):
        self.check(self.hip.hipEventRecord(self.b, self.stream))
        self.check(self.hip.hipEventSynchronize(self.b))
        ms = C.c_float(0.0)
        self.check(self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return float(ms.value)


def slab_runs(lfa, cfg, box, s0, counts, want_n, want_state):
    """[{ranks, bounds, rank_event_ms, rank_particles}] for every slab count."""
    size = cfg["size"]
    layers = (size[2] + 7) // 8
    out = []
    for n_ranks in counts:
        bounds = [(r * layers) // n_ranks for r in range(n_ranks + 1)]
        hub = lfa.LocalHub(n_ranks)
        sims = [lfa.Sim(size, method=cfg["method"], blending=cfg["blending"]) for _ in range(n_ranks)]
        for r, sim in enumerate(sims):
            sim.init_local_slab(hub.h, r, bounds)
        ms, kept = [], []
        for sim in sims:
            ev = Events(sim.stream)
            sim.synchronize()
            ev.start()
            n, state, _ = sim.seed_box((0.0, 0.0, 0.0), box, density=2, rng_state=s0, flags=lfa.SEED_COLLECTIVE)
            ms.append(ev.stop_ms())
            assert state == want_state and sim.seed_last()[1] == want_n and sim.num_particles == n
            kept.append(n)
        assert sum(kept) == want_n
        for sim in sims:
            sim.close()
        hub.close()
        out.append({"ranks": n_ranks, "bounds": bounds, "rank_event_ms": ms, "rank_particles": kept})
    return out


def child(name, reps, slabs=()):
    import numpy as np
    import libfluid_amd as lfa
    from libfluid_amd import scenes
    from tests import seed_model as sm
    cfg = scenes.CONFIGS[name]
    size, (lo, hi) = cfg["size"], cfg["block"]
    assert tuple(lo) == (0, 0, 0)
    box = [float(x) for x in hi]
    s0 = sm.initial_state()
    sim = lfa.Sim(size, method=cfg["method"], blending=cfg["blending"])
    ev = Events(sim.stream)
    event_ms, wall_ms = [], []
    for k in range(1 + reps):
        sim.upload_particles(np.zeros(0, dtype=lfa.PARTICLE_DTYPE))  # an empty handle (the arrays stay allocated)
        sim.synchronize()
        t0 = time.perf_counter()
        ev.start()
        n, state, _ = sim.seed_box((0.0, 0.0, 0.0), box, density=2, rng_state=s0)
        event_ms.append(ev.stop_ms())
        sim.synchronize()
        wall_ms.append(1e3 * (time.perf_counter() - t0))
    assert sim.num_particles == n
    sim.close()
    slab = slab_runs(lfa, cfg, box, s0, slabs, n, state)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "seed_host_route")
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-o", exe, os.path.join(ROOT, "tools", "seed_host_route.cpp"),
                        "-L" + os.path.dirname(lfa.LIB_PATH), "-l:libfluid_amd.so", "-Wl,-rpath," + os.path.dirname(lfa.LIB_PATH)], check=True)
        r = subprocess.run([exe, *map(str, size), *map(str, box), "2"], capture_output=True, text=True, check=True)
    hn, loop_ms, upload_ms, hstate = r.stdout.split()
    med = statistics.median
    out = {"config": name, "grid": list(size), "box": box, "density": 2, "particles": n, "reps": reps,
           "device_first_call_event_ms": event_ms[0], "device_first_call_wall_ms": wall_ms[0],
           "device_event_ms": med(event_ms[1:]), "device_event_ms_min_max": [min(event_ms[1:]), max(event_ms[1:])],
           "device_wall_ms": med(wall_ms[1:]),
           "host_loop_wall_ms": float(loop_ms), "host_upload_wall_ms": float(upload_ms),
           "host_route_wall_ms": float(loop_ms) + float(upload_ms),
           "host_route_over_device_first_call": (float(loop_ms) + float(upload_ms)) / wall_ms[0],
           "same_count_and_state": bool(int(hn) == n and int(hstate) == state)}
    if slab:
        out["slabs"] = slab
    print(json.dumps(out), flush=True)
    return 0 if out["same_count_and_state"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slabs", default="", help="also seed collectively on these numbers of virtual slabs, e.g. 2,4,8")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, [int(x) for x in args.slabs.split(",") if x])
    for name in args.configs.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps),
               "--slabs", args.slabs]
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
