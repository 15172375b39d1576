"""bench.py's plain single-GPU run at the headline size: exactly --steps timed iterations and nothing besides the headline, and
--dump-outputs gives the same arrays from run to run (the same arguments give the same inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_RECORDS = ("clock", "timed_regions", "ms_per_step_runs", "roofline_gae", "strict_f32", "with_stats_readback", "configs", "cpu_baseline", "suite")


def _plain_run(out_dir, steps=3, warmup=1):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(out_dir)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_times_the_commanded_steps_and_dumps_the_same_outputs_twice(tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(65536 * 128 / (d["ms_per_step"] * 1e-3), rel=1e-9)
        assert not [k for k in SIDE_RECORDS if k in d], "a plain run computes the headline only (side records belong to --full)"
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert {"params.npy", "adam_m.npy", "adam_v.npy", "action.npy", "advantage.npy", "return.npy", "episode_stats.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), n
        total += x.nbytes
        assert np.array_equal(x, y), f"{n}: the same arguments gave other outputs (max |diff| {np.max(np.abs(x.astype(np.float64) - y)):.3g})"
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "params.npy").size == np.load(tmp_path / "a" / "adam_m.npy").size
    assert np.load(tmp_path / "a" / "episode_stats.npy")[0] > 0, "episodes finished during warm-up + timed steps"
