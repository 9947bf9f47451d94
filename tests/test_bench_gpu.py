"""GPU: a plain `bench.py` run times its steps and prints the headline line only (the legs beside it run with --full), and
--dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0 and j["dtype"] == "bf16"
    for k in ("roofline", "top_kernels", "images_per_sec_all_rows_of_last_block", "warmup_phase_images_per_sec", "images_per_sec_fp32_mode",
              "cpu_baseline"):
        assert k not in j, k                   # --full only
    names = sorted(f[:-4] for f in os.listdir(out))
    for n in ("loss", "outputs_0", "gnorm", "cur", "s", "r", "g", "params"):
        assert n in names, (n, names)
    arrs = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["outputs_0"].shape == (32, 1000)
    assert abs(float(arrs["loss"].reshape(-1)[0]) - j["final_loss"]) <= 1e-4 and abs(float(arrs["cur"].reshape(-1)[0]) - j["cur_resource"]) <= 1e-4
