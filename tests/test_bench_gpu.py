"""A plain bench.py run (no --full): one JSON line with the headline figure and the timed loop's own figures, none of the legs that
take runs of their own, and the --dump-outputs arrays of its timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

pytestmark = pytest.mark.gpu

# keys only the legs behind --full add to the line
FULL_ONLY = ("value_block_until_mapped", "value_pipelined", "value_pcie_inclusive", "roofline_throughput_mode", "extra_configs",
             "cpu_baseline_other", "speedup_vs_cpu_baseline")


def test_plain_run_times_the_headline_only(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "LSD_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["cpu_baseline"] is None
    assert not set(FULL_ONLY) & set(d), sorted(set(FULL_ONLY) & set(d))
    assert d["steps"] == 20 and d["warmup"] == 5 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 1.0) < 1e-6
    assert d["validation"]["ok"] is True and d["roofline"]["bound"] == "hbm"
    assert np.load(os.path.join(str(tmp_path), "poses.npy")).shape == (20, 7)
