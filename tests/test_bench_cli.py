"""bench.py command-line contract: a plain run times exactly --steps steps
and prints one result line, --dump-outputs writes the last timed step's
outputs reproducibly, and --full adds the measurements that take steps of
their own. Runs the CPU config with any GPU hidden from the child."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = "-1"
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--config", "cpu", "--steps", "3", "--warmup", "1", *extra],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    """A tensor over its share of the byte budget is stored as the same
    seeded, order-preserving sample of its elements on every call."""
    import importlib.util

    import torch
    spec = importlib.util.spec_from_file_location(
        "bench_under_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 100)  # 50 per tensor
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    small = torch.ones(5, 10, dtype=torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    got = np.load(tmp_path / "a" / "big.npy")
    assert got.dtype == np.float32 and got.shape == (50,)
    assert (np.diff(got) > 0).all() and got.max() < 1000
    assert np.array_equal(got, np.load(tmp_path / "b" / "big.npy"))
    assert np.load(tmp_path / "a" / "small.npy").shape == (5, 10)


def test_plain_run_dumps_reproducible_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    rec = _bench("--dump-outputs", str(a))
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and rec["unit"] == "seq/s"
    assert abs(rec["value"] - 8 * 1000.0 / rec["ms_per_step"]) < 1e-6 * rec["value"]
    assert "train_3class_acc" not in rec["config"]  # needs --full

    # --full leaves the timed path (and so its dumped outputs) unchanged
    rec_full = _bench("--full", "--dump-outputs", str(b))
    assert 0.0 <= rec_full["config"]["train_3class_acc"] <= 1.0
    assert rec_full["metric"] == rec["metric"]

    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"loss.npy", "logits.npy", "param.linear.weight.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n  # same seeds -> same CPU results
        total += os.path.getsize(a / n)
    assert np.load(a / "logits.npy").shape == (8, 4)
    assert total <= 64_000_000


def test_predict_config_honours_steps_warmup_and_dumps(tmp_path):
    """The streaming-inference config times exactly --steps ticks after
    exactly --warmup ones and dumps the last tick's probabilities."""
    rec = _bench("--config", "predict", "--steps", "4", "--warmup", "0",
                 "--dump-outputs", str(tmp_path / "p"))
    assert rec["steps"] == 4 and rec["warmup"] == 0
    assert rec["unit"] == "ms" and rec["higher_is_better"] is False
    assert rec["ms_per_step"] == rec["value"] > 0
    probs = np.load(tmp_path / "p" / "probabilities.npy")
    assert probs.dtype == np.float32 and probs.shape == (4,)
    assert ((probs >= 0) & (probs <= 1)).all()
    assert os.listdir(tmp_path / "p") == ["probabilities.npy"]
