"""Seeding an inflow from the simulation's pcg32: lfa_update_sources_rng on a single domain, and the collective call
(LFA_SEED_COLLECTIVE) on N virtual slabs of one GPU. Not bench.py: a measurement of one call. The scene is a 512 x 512-cell inflow
plane (y = the top cell layer, every x and z) of target_density_cubic_root 2 on the empty C4 grid (libfluid_amd/scenes.py):
262 144 entries, 2 097 152 particles, and the plane crosses every slab face.

  single  HIP events around the call on the handle's stream (the call reads a count back in the middle and ends with the
          re-binning, so this is the time from its first kernel to its last, waits included), and the wall time of the call plus a
          synchronise. The first call on a handle also allocates the particle arrays; the repetitions after it (the handle emptied
          and re-binned in between) do not.
  slabs   --slabs 1,2,4: the same scene on N ranks, the tile layers split evenly, one host thread per rank (the call exchanges one
          all-reduce and re-bins collectively). Per rank the event time and the particles kept; the ranks of a virtual
          decomposition share one GPU, so their times overlap and do not add up to a job's time. The collective's overhead -
          the all-reduce, the scan over the job-wide entry list and the count pass - is reported as the difference between the
          1-slab collective call and the single-domain call, which create and bin the same particles.
The counts and the generator state of every run must agree. Every run is a child process under a time limit; a failure ends the
probe. One JSON line.

    python tools/source_probe.py [--reps 5] [--slabs 1,2,4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMIT_S = 540
ROOT3 = 2


def scene(lfa, scenes):
    import numpy as np
    cfg = scenes.CONFIGS["C4"]
    nx, ny, nz = cfg["size"]
    x, z = np.meshgrid(np.arange(nx, dtype=np.int32), np.arange(nz, dtype=np.int32), indexing="xy")
    cells = np.stack([x.ravel(), np.full(nx * nz, ny - 1, dtype=np.int32), z.ravel()], axis=1)  # z outer, x fastest
    return cfg, cells, (0.0, -1.0, 0.0)


def empty_and_bin(lfa, sims):
    import numpy as np
    for s in sims:
        s.upload_particles(np.zeros(0, dtype=lfa.PARTICLE_DTYPE))  # an empty handle (the arrays stay allocated)
    on_threads(sims, lambda r, s: s.hash())


def on_threads(sims, fn):
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
        t.join(timeout=300)
    if errors or any(t.is_alive() for t in threads):
        raise RuntimeError(f"rank threads failed or hung: {errors}")
    return out


def timed_calls(lfa, sims, s0, flags, reps):
    """1 + reps calls on the handles (a single domain: one handle); per call [(event ms, wall ms, kept)] in rank order."""
    from seed_probe import Events
    evs = [Events(s.stream) for s in sims]
    runs, state = [], None

    def call(r, s):
        s.synchronize()
        t0 = time.perf_counter()
        evs[r].start()
        n, st, _ = s.update_sources_rng(s0, flags=flags)
        ms = evs[r].stop_ms()
        s.synchronize()
        return ms, 1e3 * (time.perf_counter() - t0), n, st, s.source_last()[0]

    for _ in range(1 + reps):
        empty_and_bin(lfa, sims)
        res = on_threads(sims, call)
        assert len({(st, total) for _, _, _, st, total in res}) == 1
        assert sum(n for _, _, n, _, _ in res) == res[0][4]
        state = (res[0][3], res[0][4])
        runs.append([(ms, wall, n) for ms, wall, n, _, _ in res])
    return runs, state


def child(reps, slabs):
    import libfluid_amd as lfa
    from libfluid_amd import scenes
    from tests import seed_model as sm
    cfg, cells, vel = scene(lfa, scenes)
    size, s0, med = cfg["size"], sm.initial_state(), statistics.median
    kw = dict(method=cfg["method"], blending=cfg["blending"])
    one = lfa.Sim(size, **kw)
    one.add_source(cells, vel, ROOT3, True, False)
    runs, want = timed_calls(lfa, [one], s0, 0, reps)
    one.close()
    ev, wall = [r[0][0] for r in runs], [r[0][1] for r in runs]
    out = {"config": "C4", "grid": list(size), "entries": int(len(cells)), "root": ROOT3, "particles": want[1], "reps": reps,
           "single_first_call_event_ms": ev[0], "single_event_ms": med(ev[1:]), "single_event_ms_min_max": [min(ev[1:]), max(ev[1:])],
           "single_wall_ms": med(wall[1:]), "slabs": []}
    assert want[1] == len(cells) * ROOT3 ** 3 and want[0] == sm.advance(s0, 6 * want[1])
    layers = (size[2] + 7) // 8
    for n_ranks in slabs:
        bounds = [(r * layers) // n_ranks for r in range(n_ranks + 1)]
        hub = lfa.LocalHub(n_ranks)
        sims = [lfa.Sim(size, **kw) for _ in range(n_ranks)]
        for r, s in enumerate(sims):
            s.init_local_slab(hub.h, r, bounds)
            s.add_source(cells, vel, ROOT3, True, False)
        runs, got = timed_calls(lfa, sims, s0, lfa.SEED_COLLECTIVE, reps)
        assert got == want, (got, want)
        for s in sims:
            s.close()
        hub.close()
        rank_ms = [med([run[r][0] for run in runs[1:]]) for r in range(n_ranks)]
        slowest = [max(ms for ms, _, _ in run) for run in runs[1:]]
        out["slabs"].append({"ranks": n_ranks, "bounds": bounds, "rank_event_ms": rank_ms, "rank_particles": [k for _, _, k in runs[-1]],
                             "slowest_rank_event_ms": med(slowest), "slowest_rank_event_ms_min_max": [min(slowest), max(slowest)],
                             "wall_ms": med([max(w for _, w, _ in run) for run in runs[1:]])})
    if out["slabs"] and out["slabs"][0]["ranks"] == 1:
        out["collective_overhead_ms_1_slab"] = out["slabs"][0]["slowest_rank_event_ms"] - out["single_event_ms"]
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slabs", default="1,2,4", help="numbers of virtual slabs for the collective call ('' for none)")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.reps, [int(x) for x in args.slabs.split(",") if x])
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--slabs", args.slabs]
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
