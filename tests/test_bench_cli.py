"""bench.py's command line: a plain run does only what its headline figure needs, --full adds the extra measurements, --steps sets the
timed steps, --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--layers", "2", "--pairs-per-gpu", "2", "--pairs-per-group", "2"]


def _bench(args, timeout=900):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "HALVA_DP_FORCE", "HALVA_SHARE_GPU", "HALVA_BENCH_SHARE_GPU"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_rejects_zero_steps():
    r = _bench(["--steps", "0"], timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(out)] + SMALL)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(2 / (rec["ms_per_step"] * 1e-3), rel=1e-2)      # 2 pairs per step
    assert rec["roofline"] is None and rec["cpu_baseline"] is None      # the extra measurements are --full's
    names = sorted(os.listdir(out))
    assert names == ["alignment.npy", "divergence.npy", "grad_sample.npy", "loss.npy", "master_sample.npy"]
    total = 0
    for n in names:
        a = np.load(out / n)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all()
        total += (out / n).stat().st_size
    assert total <= 64 * 2 ** 20
    loss = np.load(out / "loss.npy")
    assert loss.shape == (1,) and round(float(loss[0]), 5) == rec["loss"]
    assert float(loss[0]) == pytest.approx(float(np.load(out / "alignment.npy")[0]) + float(np.load(out / "divergence.npy")[0]) * 0.4, abs=1e-4)
    assert np.abs(np.load(out / "grad_sample.npy")).sum() > 0


@pytest.mark.gpu
def test_full_bench_adds_the_roofline():
    r = _bench(["--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline"] + SMALL)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    assert rec["steps"] == 1 and rec["cpu_baseline"] is None
    assert rec["roofline"]["achieved"] > 0 and rec["roofline"]["launches"] > 0 and "fwd_in_step" in rec["roofline"]
