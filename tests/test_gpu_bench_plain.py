"""GPU: a plain `python bench.py` run (no --full) does only what its headline needs - set-up, warm-up, the timed steps, --dump-outputs and the line -
and its timed path computes exactly what a --full run's does: both dump the same proof from the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXTRAS = ("transcript_prefix_cached", "reference_order", "roofline_hbm", "sparse", "kernel_ms_per_step", "concurrent_proofs_extra", "verify_ms",
          "verify_accepts", "cpu_baseline", "prep_prove", "scaling_vs_1")


def _bench(flags, dump_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump_dir)] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def test_plain_run_is_the_headline_and_the_same_timed_path(tmp_path):
    plain, err = _bench([], tmp_path / "plain")
    assert plain["full"] is False and plain["n_gpus"] == 1 and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["unit"] == "constraints/s" and plain["higher_is_better"] is True and plain["dtype"].startswith("u256")
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["frac"] > 0  # the roofline kernel is timed inside the steps
    assert plain["sharded"] is None and "[bench] sharded." not in err
    assert not [k for k in EXTRAS if k in plain] and "other_kernels" not in plain["roofline"]

    full, _ = _bench(["--full", "--no-cpu-baseline", "--no-sharded", "--concurrent", "0"], tmp_path / "full")
    assert full["full"] is True and all(k in full for k in EXTRAS if k not in ("cpu_baseline", "scaling_vs_1")) and "other_kernels" in full["roofline"]

    for name in ("proof_words", "tape_blocks_used"):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.shape == b.shape and (a == b).all(), name
