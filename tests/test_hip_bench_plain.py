"""A plain bench.py run (no --full) does only what its headline needs: set-up, warm-up, the timed passes, --dump-outputs and
the one JSON line.  The roofline replays, the CPU baseline and the other configs' legs stay behind --full.  The run is a fresh
CHILD process started before this process touches the GPU for it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_writes_only_the_dump(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    side = os.path.join(ROOT, bench.LEGS_FILE)
    before = os.stat(side).st_mtime_ns if os.path.exists(side) else None
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["value"] > 0 and out["unit"] == "tokens/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 4 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["timed_passes"]["n"] == 3
    assert out["config"]["warmup_steps_executed"] >= 2
    for k in ("roofline", "cpu_baseline", "legs", "details"):
        assert k not in out, k
    for msg in ("instrumented replay", "cpu baseline", "parity on the cpu sample"):       # nothing beside the headline ran
        assert msg not in r.stderr, msg
    hyp = np.load(tmp_path / "hypotheses.npy")
    assert hyp.shape == (4 * out["config"]["batch_per_gpu"], out["config"]["decode_steps"])
    assert (os.stat(side).st_mtime_ns if os.path.exists(side) else None) == before          # no side file written
