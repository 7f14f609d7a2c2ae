"""bench.py's plain / --full result lines and --dump-outputs.

The library's reductions use no floating-point atomics, so two runs of the
same arguments on the same build must agree bit for bit; the time-based clock
ramp in front of the warm-up (a different number of iterations in every run)
must not leak into what the timed steps compute."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels_ms", "kernels_schedule", "cpu_baseline")
SMALL = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--T", "400")


def _bench(tmp_path, *args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FASST_BENCH_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".npy")}


def test_dump_outputs_files_and_sample(tmp_path):
    """Arrays within their share of the budget are written whole; a larger
    one as the same fixed sample of its elements in every call."""
    rng = np.random.RandomState(3)
    arrays = {"small": rng.rand(7, 5), "big": rng.rand(1000, 33)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=2 * 800 * 8)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["big", "small"]
    assert np.array_equal(a["small"], arrays["small"])
    assert a["big"].shape == (800,) and a["big"].dtype == np.float64
    assert np.array_equal(a["big"], b["big"])
    assert np.isin(a["big"], arrays["big"]).all()
    assert sum(v.nbytes for v in a.values()) <= 2 * 800 * 8


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.main(["--steps", "0", "--dry-run"])


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    line = _bench(d, *SMALL, "--warm-s", "0.2", "--dump-outputs", str(d / "out"))
    return line, _load(str(d / "out"))


@pytest.mark.gpu
def test_plain_line_and_dump(plain_run):
    line, out = plain_run
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 3 and line["unit"] == "EM it/s" and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(3 / (line["ms_per_step"] * 3e-3), rel=1e-3)
    F, T, J, K = bench.F_BINS, 400, bench.J_SRC, bench.K_NMF
    want = {"loglik": (3,)}
    for j in range(J):
        want.update({"spat%d_params" % j: (bench.RANK, 2, F, 2), "spec%d_FB" % j: (F, K),
                     "spec%d_FW" % j: (K, K), "spec%d_TW" % j: (K, T)})
    assert {k: v.shape for k, v in out.items()} == want
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in out.values())
    assert out["loglik"][-1] == line["clips"][0]["loglik"]


@pytest.mark.gpu
def test_dump_is_the_same_from_run_to_run(plain_run, tmp_path):
    """A second process with a longer clock ramp writes the same bits."""
    _, first = plain_run
    _bench(tmp_path, *SMALL, "--warm-s", "0.5", "--dump-outputs", str(tmp_path / "out"))
    second = _load(str(tmp_path / "out"))
    assert sorted(first) == sorted(second)
    for k in first:
        assert np.array_equal(first[k], second[k]), k


@pytest.mark.gpu
def test_full_line_carries_the_secondary_measurements(tmp_path):
    line = _bench(tmp_path, *SMALL, "--warm-s", "0", "--full", "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE)
    assert line["kernels_ms"]["k_estep"] > 0 and "cpu_baseline" not in line
    # (the roofline block is None where, as at this small T, the longest
    # kernel is not one of those with a work model)
    assert "roofline" in line and "in situ" in line["kernels_schedule"]
