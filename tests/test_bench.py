"""bench.py's own contract: a plain run times the steps and prints the headline line, nothing else measured; `--dump-outputs DIR`
writes what one timed step computes from the seeded input; `--full` adds the secondary figures. (The N > 1 paths: tests/test_gpu_slabs.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("ms_per_step_serial_stages", "hbm_ceiling_measured", "roofline", "kernels_isolated", "hot_path", "pcg_mic0", "cpu_baseline")


def bench(*args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def line_of(p):
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("args", [["--steps", "0"], ["--gpus", "2", "--dump-outputs", "out"], ["--force-slabs", "--dump-outputs", "out"]])
def test_bench_refuses_what_it_cannot_honour_before_touching_a_gpu(args, tmp_path):
    p = bench(*args, timeout=120)
    assert p.returncode != 0 and not p.stdout.strip(), p.stdout[-500:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_a_reproducible_step(tmp_path):
    out = line_of(bench("--config", "C2", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)))
    assert out["metric"] == "particle_steps_per_sec" and out["unit"] == "particle-steps/s" and out["higher_is_better"] is True
    assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["dtype"] == "f32"
    assert out["value"] == pytest.approx(out["config"]["particles_per_gpu"] * 1e3 / out["ms_per_step"], rel=1e-9)
    assert not [k for k in SECONDARY if k in out]
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == {"particle_index", "position", "velocity", "affine", "pressure_cell", "pressure", "step_dt_residual_iterations"}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20
    k = 1 << 18
    pi = got["particle_index"]
    assert pi.shape == (k,) and (np.diff(pi) > 0).all() and pi[0] >= 0 and pi[-1] < out["config"]["particles_per_gpu"]
    assert got["position"].shape == (k, 3) and got["velocity"].shape == (k, 3) and got["affine"].shape == (k, 3, 3)
    assert ((got["position"] >= 0) & (got["position"] <= 128)).all() and np.abs(got["velocity"]).max() > 0
    pc = got["pressure_cell"]  # C2's block is [0, 64)^3 of 128^3: fewer cells than the sample size, all of them
    assert pc.shape == got["pressure"].shape == (64 ** 3,) and (np.diff(pc) > 0).all() and pc[-1] < 128 ** 3
    assert (got["pressure"] != 0).mean() > 0.25
    dt, res, it = got["step_dt_residual_iterations"]
    assert 0 < dt <= 0.033 and res >= 0 and it >= 1
    # another run with other timed steps dumps the same arrays: the same step from the same seeded input, up to the order of the
    # position correction's sums
    line_of(bench("--config", "C2", "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / "b")))
    other = {f[:-4]: np.load(os.path.join(tmp_path / "b", f)) for f in os.listdir(tmp_path / "b")}
    assert {n: a.shape for n, a in other.items()} == {n: a.shape for n, a in got.items()}
    assert np.array_equal(other["particle_index"], pi) and np.array_equal(other["pressure_cell"], pc)
    assert np.abs(other["position"] - got["position"]).max() < 1e-4
    for n in ("velocity", "affine", "pressure"):
        assert np.abs(other[n] - got[n]).max() <= 1e-4 * np.abs(got[n]).max(), n
    assert other["step_dt_residual_iterations"][0] == dt and abs(other["step_dt_residual_iterations"][2] - it) <= 1


@pytest.mark.gpu
def test_full_run_adds_the_secondary_figures():
    out = line_of(bench("--config", "C2", "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline"))
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert all(k in out for k in SECONDARY if k != "cpu_baseline")
