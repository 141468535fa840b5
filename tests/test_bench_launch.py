"""bench.py launch contract: ``python bench.py --gpus N`` with no launcher
around it starts N ranks itself and reports n_gpus = N; a --gpus / WORLD_SIZE mismatch is fatal.
Runs the CPU mode (FDX_BENCH_DEVICE=cpu: same code path on CPU tensors over gloo)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    env["FDX_BENCH_DEVICE"] = "cpu"
    env.update(kw)
    return env


def _json_line(out: str) -> dict:
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out  # rank 0 prints exactly one JSON line
    return json.loads(lines[0])


def test_self_launch_two_ranks():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--rows-per-gpu", "20000"], cwd=ROOT, env=_env(), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["global_batch"] == 2 * 16000
    assert "self-launch" in r.stderr


def test_single_rank_default():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "1", "--warmup", "0", "--rows-per-gpu", "20000"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 1 and out["config"]["parallelism"] == "dp1"


def test_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed fit's result as float64 .npy files; the inputs are
    seeded, so a second run with the same arguments writes the same arrays.  --full is accepted."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--rows-per-gpu", "20000", "--dump-outputs", str(d)] + extra,
                           cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = _json_line(r.stdout)
        assert out["steps"] == 2 and out["ms_per_step"] > 0
        dumps.append({p.name: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == set(b) and {"weights.npy", "scaler_mean.npy", "scaler_scale.npy", "row_counts.npy"} <= set(a)
    for k in a:
        assert a[k].dtype == np.float64 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert a["weights.npy"].shape == (32,) and np.abs(a["weights.npy"]).max() > 0
    assert a["row_counts.npy"][0] == 16000


def test_extras_run_only_with_full():
    """The lean / full split: a plain command line selects no extra measurement, --full selects
    them, the deprecated --no-extras overrides --full, and the CPU contract mode never runs them."""
    import bench  # the repository root is on sys.path (tests/conftest.py)

    plain = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert plain.steps == 3 and plain.warmup == 1 and plain.dump_outputs is None
    assert not bench._wants_extras(plain, cpu_mode=False)
    assert bench._wants_extras(bench.parse(["--full"]), cpu_mode=False)
    assert not bench._wants_extras(bench.parse(["--full", "--no-extras"]), cpu_mode=False)
    assert not bench._wants_extras(bench.parse(["--no-extras"]), cpu_mode=False)
    assert not bench._wants_extras(bench.parse(["--full"]), cpu_mode=True)


@pytest.mark.gpu
def test_plain_run_reports_headline_only(tmp_path):
    """On the GPU a plain run's result line holds the headline fields and none of the extras
    (--full adds those: bench.py main)."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FDX_BENCH_DEVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--rows-per-gpu", "200000", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["unit"] == "rows/s"
    for k in ("auc", "sgd", "phase_ms", "linear_shap_values_per_sec", "sgd_bf16", "newton_bf16", "end_to_end",
              "cv_job", "gbdt", "predict_1M", "kernelshap_worker"):
        assert k not in out, k
    assert (tmp_path / "weights.npy").exists()


def test_world_size_mismatch_is_fatal():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "1", "--warmup", "0"],
                       cwd=ROOT, env=_env(WORLD_SIZE="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "FATAL" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
