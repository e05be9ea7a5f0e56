"""bench.py's plain run: set-up, warm-up, the timed steps, --dump-outputs and the line -- nothing that only --full measures.
(--full at N > 1: tests/test_distributed.py::test_bench_self_launches_its_ranks_from_a_bare_shell.)"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = {"sustained_200_steps", "variants", "in_loop_kernels", "scaling_model", "roofline", "roofline_normalised",
             "roofline_widening", "reasoning_learner", "cpu_baseline", "cpu_baseline_token_tier", "speedup_vs_cpu_baseline",
             "probe_errors"}


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only(tmp_path):
    dump = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(dump)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["metric"] == "env_steps_per_sec" and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["total_envs"] == 1024 and line["config"]["global_batch"] == 8192
    assert not FULL_ONLY & set(line), sorted(FULL_ONLY & set(line))
    for name in ("params", "exp_avg", "exp_avg_sq", "rollout.rewards"):
        a = np.load(dump / f"{name}.npy")
        assert a.size > 0 and np.isfinite(a).all(), name
