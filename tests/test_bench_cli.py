"""bench.py's command line: a plain run prints the headline record alone, --full adds the roofline,
--dump-outputs writes the last timed step's results as float .npy files under 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dump_array_is_float_and_samples_reproducibly(tmp_path):
    """An array over its cap is stored as the same seeded element sample every time; integers become float64."""
    import bench
    a = np.arange(1000, dtype=np.float32).reshape(10, 100)
    bench._dump_array(str(tmp_path), "whole", a, 1000)
    bench._dump_array(str(tmp_path), "part", a, 100)
    bench._dump_array(str(tmp_path), "again", a + 0, 100)
    bench._dump_array(str(tmp_path), "ints", np.arange(5), 10)
    whole, part = np.load(tmp_path / "whole.npy"), np.load(tmp_path / "part.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, a)
    assert part.shape == (100,) and np.all(np.diff(part) > 0)          # distinct elements, in memory order
    assert np.array_equal(part, np.load(tmp_path / "again.npy"))
    assert np.load(tmp_path / "ints.npy").dtype == np.float64


def test_plain_and_full_are_separate_options():
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"]
        a = bench.parse()
        assert not a.full and a.dump_outputs is None and a.steps == 3 and a.warmup == 2
        sys.argv += ["--full", "--dump-outputs", "d"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "d"
    finally:
        sys.argv = argv


@pytest.mark.gpu
def test_plain_run_prints_headline_only_and_dumps_outputs(tmp_path):
    """--steps 2 at batch 64: the record holds the headline fields and no roofline / CPU baseline; the dump holds the
    last step's loss, prediction, parameters, buffers and gradients, finite, and the loss file equals the record's."""
    d = tmp_path / "out"
    rec = _bench("--steps", "2", "--warmup", "1", "--batch", "64", "--dump-outputs", str(d))
    for k in HEADLINE:
        assert k in rec, k
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(64 * 1e3 / rec["ms_per_step"], rel=1e-3)
    assert "roofline" not in rec and "cpu_baseline" not in rec
    files = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert set(files) == {"loss", "grad_norm", "output", "params", "buffers", "grads_sample"}
    assert sum(a.nbytes for a in files.values()) <= 64e6
    for name, a in files.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    assert files["output"].shape == (64, 1, 40, 40)
    assert files["params"].size == 7834588 and files["grads_sample"].size == 4000000
    assert float(files["loss"][0]) == pytest.approx(rec["config"]["final_loss"], abs=1e-6)
    assert np.abs(files["grads_sample"]).max() > 0
