"""GPU: a plain `bench.py` run prints the headline line only, and --dump-outputs writes what the last timed step handed its caller"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(dump, steps=3, warmup=1):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "f16" and line["finite_logits"] is True
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-6 * 1e3          # one stream: ms per step = 1000 / tokens per s
    for extra in ("roofline", "parity", "cpu_baseline", "gemv_layers", "beyond_the_metric", "mfma_roofline", "dequant_hqq"):
        assert extra not in line, extra
    logits, token = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "a" / "next_token.npy")
    assert logits.dtype == np.float32 and logits.shape == (32000,) and np.isfinite(logits).all()
    assert token.dtype == np.float64 and token.shape == (1,) and logits[int(token[0])] == logits.max()     # the greedy choice of those logits
    # the same arguments: the same seeded inputs, so the same outputs (up to the order of floating-point sums)
    _bench(tmp_path / "b")
    logits_b, token_b = np.load(tmp_path / "b" / "logits.npy"), np.load(tmp_path / "b" / "next_token.npy")
    assert np.array_equal(token, token_b)
    assert np.abs(logits - logits_b).max() <= 1e-3 * np.abs(logits).max()
