"""bench.py's two modes: a plain run reports the timed steps alone; --full adds the measurements taken after the timed region
(the rollout / update split, the kernel rooflines; the CPU baseline is left out here with --no_cpu_baseline, it takes a minute)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("rollout_env_steps_per_s", "collection_s", "learn_s", "roofline", "policy_roofline")


def _bench_line(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--num_envs", "512"] + extra,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_reports_the_timed_steps_alone():
    d = _bench_line([])
    assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "env-steps/s"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["num_envs_per_gpu"] == 512
    assert not any(k in d for k in FULL_ONLY + ("cpu_baseline",))


@pytest.mark.gpu
def test_full_run_adds_the_phase_split_and_the_kernel_rooflines():
    d = _bench_line(["--full", "--no_cpu_baseline"])
    assert all(k in d for k in HEADLINE + FULL_ONLY) and "cpu_baseline" not in d
    assert d["collection_s"] > 0 and d["rollout_env_steps_per_s"] > 0
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["kernel_ms_back_to_back"] > 0 and d["policy_roofline"]["kernel_ms"] > 0
