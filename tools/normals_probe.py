"""Vertex normals: the device pass (lfa_mesher_normals) against the serial host loop (fluid_amd::mesh::generate_normals) on the
same mesh. Not bench.py: a measurement of one call, on two meshes -

  dam100 : the 100^3 dam-break surface of tests/test_mesher.py::test_dam_break_surface_at_scale
  C5     : the surface `bench.py --config C5 --obstacle --mesh` meshes (1024 x 512 x 512 cells, 134 M particles, the voxelised
           sphere, bench.py's default 20 + 50 steps with dt = min(3 cfl, 0.033))

For each: medians over --reps repetitions after --warmup warm-ups of
  device  HIP-event time of lfa_mesher_normals alone on the mesher's stream (lfa_mesher_normals_time), and the wall time of
          compute + download of the normals; every repetition starts from a fresh extraction, so the face vectors are
          computed inside it;
  host    wall time of the loop on the downloaded mesh (tools/normals_host_loop.cpp, g++ -O2, one thread);
and the bytes the device pass must move at the least (24 nv written + 8 ni indices + 24 nv positions read once), hence its share
of the measured 5.8-6.2 TB/s copy ceiling. The two results are also compared (NaN beside NaN counts as equal).
Every mesh runs in a child process of its own under a time limit; a failure ends the probe. One JSON line per mesh.

--windows N[,N...]: the same surface cut into N equal z-windows on the one GPU (what the ranks of a slab run hold), normals by
lfa_mesher_window_normals_from from the top window down. Per window: the device time (lfa_mesher_normals_time; every repetition
starts from a fresh extraction, so the face vectors are computed inside it) and the bytes of the boundary it exports; the sum
over the windows stands beside the whole-grid device time and the host loop on the stitched mesh, which is what a slab run
has to use without it. The stitched normals are compared with the whole grid's. One more JSON line per N.

    python tools/normals_probe.py [--meshes dam100,C5] [--windows 2,8] [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = {"dam100": 240, "C5": 540}
COPY_CEILING_TBPS = (5.8, 6.2)


def build_host_loop(d):
    exe = os.path.join(d, "normals_host_loop")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tools", "normals_host_loop.cpp")],
                   check=True)
    return exe


def mesh_dam100(lfa, np):
    from libfluid_amd import scenes
    p = scenes.seed_block((1, 1, 1), (49, 49, 49))["pos"]
    p = p[np.random.default_rng(9).permutation(len(p))]
    m = lfa.Mesher(size=(100, 100, 100), grid_offset=(0.0, 0.0, 0.0), cell_size=0.5, particle_extent=1.0, cell_radius=3)
    m.sample(p, 0.5)
    return m, None


def mesh_c5(lfa, np):
    """bench.py's C5 run with --obstacle --mesh up to the mesher call (single GPU, default solver settings): a restatement of
    bench.py's build_sim (Sim arguments), add_obstacle (sphere radius, centre, icosphere level 5), its default 20 + 50 steps with
    one_step's dt rule, and the Mesher arguments of its --mesh leg. bench.py is the yardstick and is not to import from a tool,
    so the two are kept together by hand: C5_EXPECTED below is what that run meshes; a count further off means one of them moved."""
    from libfluid_amd import scenes
    cfg = scenes.CONFIGS["C5"]
    size, (blo, bhi) = list(cfg["size"]), [list(x) for x in cfg["block"]]
    sim = lfa.Sim(size, method=cfg["method"], blending=cfg["blending"])
    rad = 0.16 * min(bhi[0] - blo[0], bhi[1] - blo[1], bhi[2] - blo[2])
    ctr = [min(bhi[0] + 2.0 * rad, size[0] - 1.5 * rad), blo[1] + 1.2 * rad, 0.5 * (blo[2] + bhi[2])]
    mpos, midx = scenes.icosphere(ctr, rad, 5)
    vox = lfa.Voxels.from_mesh(mpos, midx, 1.0, (0.0, 0.0, 0.0))
    sim.set_solid_from_voxels(vox, True, True)
    vox.close()
    sim.seed_block(blo, bhi)
    for _ in range(70):
        sim.time_step(min(3.0 * sim.cfl(), 0.033))
    m = lfa.Mesher(size, (0.0, 0.0, 0.0), 1.0, 1.0, 2)
    m.sample_sim(sim, 0.5)
    return m, sim


# vertices, triangles of bench.py --config C5 --obstacle --mesh (profiles/normals_probe.jsonl). The simulation's fp32 atomic sums
# are not reproducible bit for bit, so after 70 steps two runs differ by a fraction of a per cent (545 054 / 547 320 vertices seen)
C5_EXPECTED, C5_SLACK = (547320, 1093364), 0.02


def window_lines(lfa, np, name, m, counts, reps, warmup, whole_ms, host_ms, whole_nrm):
    """One result per window count: the C5 / dam100 surface from the whole-grid handle's samples, cut into equal z-windows."""
    values = m.values()
    nz = m.size[2]
    out = []
    for n in counts:
        bounds = [(nz * k) // n for k in range(n + 1)]
        ws = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            w = lfa.Mesher(m.size, window=(lo, hi), **m.grid)
            w.set_window_values(values)
            ws.append(w)
        per = [[] for _ in ws]
        for k in range(warmup + reps):
            for w in ws:
                w.marching_cubes()  # (a fresh mesh: no cached face vectors)
            for i in reversed(range(n)):
                ws[i].compute_window_normals(ws[i + 1] if i + 1 < n else None)
                if k >= warmup:
                    per[i].append(ws[i].normals_ms())
        nrm = lfa.stitch_windows(ws, normals=True)[2]
        nxy = m.size[0] * m.size[1]
        blob = [0] + [nxy + 24 * len(w.boundary()[1]) for w in ws[1:]]
        med = statistics.median
        totals = [sum(per[i][k] for i in range(n)) for k in range(reps)]
        out.append({"mesh": name, "windows": n, "bounds": bounds, "reps": reps, "warmup": warmup,
                    "vertices_per_window": [w._counts[0] for w in ws],
                    "window_event_ms": [med(x) for x in per], "boundary_bytes_exported": blob,
                    "windows_total_event_ms": med(totals), "windows_total_event_ms_min_max": [min(totals), max(totals)],
                    "whole_grid_event_ms": whole_ms, "host_loop_wall_ms": host_ms,
                    "stitched_equals_whole_grid": bool(np.array_equal(nrm, whole_nrm, equal_nan=True))})
        for w in ws:
            w.close()
    return out


def child(name, reps, warmup, windows=()):
    import numpy as np
    import libfluid_amd as lfa
    m, sim = {"dam100": mesh_dam100, "C5": mesh_c5}[name](lfa, np)
    t0 = time.perf_counter()
    pos, idx = m.marching_cubes()
    mc_ms = 1e3 * (time.perf_counter() - t0)
    nv, ni = len(pos), len(idx)
    if name == "C5" and max(abs(nv / C5_EXPECTED[0] - 1.0), abs(ni / 3 / C5_EXPECTED[1] - 1.0)) > C5_SLACK:
        print(f"note: the C5 mesh has {nv} vertices / {ni // 3} triangles, expected {C5_EXPECTED}: mesh_c5 and bench.py differ",
              file=sys.stderr, flush=True)
    ev, compute, total = [], [], []
    for k in range(warmup + reps):
        m.marching_cubes()  # (a fresh mesh: no cached face vectors, every repetition holds both passes)
        t0 = time.perf_counter()
        m.compute_normals()  # (returns after the stream has drained)
        t1 = time.perf_counter()
        nrm = m.download_normals()
        t2 = time.perf_counter()
        if k >= warmup:
            ev.append(m.normals_ms())
            compute.append(1e3 * (t1 - t0))
            total.append(1e3 * (t2 - t0))
    if sim is not None:
        sim.close()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mesh.bin")
        with open(path, "wb") as f:
            np.array([nv, ni], dtype=np.uint64).tofile(f)
            pos.tofile(f)
            idx.tofile(f)
        r = subprocess.run([build_host_loop(d), path, str(warmup), str(reps), os.path.join(d, "n.bin")], capture_output=True,
                           text=True, check=True)
        host = [float(x) for x in r.stdout.split()]
        host_nrm = np.fromfile(os.path.join(d, "n.bin"), dtype=np.float64).reshape(-1, 3)
    med = statistics.median
    least = 24 * nv + 8 * ni + 24 * nv
    out = {"mesh": name, "vertices": nv, "triangles": ni // 3, "reps": reps, "warmup": warmup,
           "marching_cubes_ms_incl_download": mc_ms,
           "device_event_ms": med(ev), "device_event_ms_min_max": [min(ev), max(ev)],
           "device_compute_wall_ms": med(compute), "device_compute_plus_download_wall_ms": med(total),
           "device_compute_plus_download_wall_ms_min_max": [min(total), max(total)],
           "host_loop_wall_ms": med(host), "host_loop_wall_ms_min_max": [min(host), max(host)],
           "host_over_device_total": med(host) / med(total),
           "least_bytes": least,
           "fraction_of_copy_ceiling": [least / (med(ev) * 1e-3) / (c * 1e12) for c in COPY_CEILING_TBPS],
           "kernel_shape": "two passes: face vectors (thread per triangle, 24 B per triangle), ordered gather (thread per cell)",
           "device_equals_host_loop": bool(np.array_equal(nrm, host_nrm, equal_nan=True))}
    print(json.dumps(out), flush=True)
    ok = out["device_equals_host_loop"]
    for line in window_lines(lfa, np, name, m, windows, reps, warmup, med(ev), med(host), nrm) if ok else []:
        print(json.dumps(line), flush=True)
        ok = ok and line["stitched_equals_whole_grid"]
    m.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--meshes", default="dam100,C5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", default="", help="window counts, e.g. 2,8: also cut every mesh into that many equal z-windows")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < 3:
        raise SystemExit("at least 20 repetitions after 3 warm-ups")
    windows = [int(x) for x in args.windows.split(",") if x]
    if args.child:
        return child(args.child, args.reps, args.warmup, windows)
    for name in args.meshes.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name] + (120 if windows else 0)), sys.executable, os.path.abspath(__file__),
               "--child", name, "--reps", str(args.reps), "--warmup", str(args.warmup), "--windows", args.windows]
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
