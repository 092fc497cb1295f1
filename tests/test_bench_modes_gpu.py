"""bench.py's plain run against `--full` at a small size: the plain line carries the headline's fields and none of what `--full`
measures after the timed steps, and both runs leave the same state after those steps (restart checksums and the dumped fields,
bit for bit) -- the plain run times the same work."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--ni", "360", "--nj", "272", "--steps", "4", "--warmup", "2"]
FULL_ONLY = {"thermo", "hbm_step", "ale_remap_leg", "diag_leg", "box_calibration", "cpu_baseline"}


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-pmc", "--cpu-steps", "4", "--no-cpu-full-size", "--dump-outputs", str(tmp_path / "full"))
    for out in (plain, full):
        assert out["metric"] == out["unit"] == "simulated-days/wall-sec" and out["higher_is_better"] is True and out["dtype"] == "f64"
        assert out["value"] > 0 and out["ms_per_step"] > 0 and (out["steps"], out["warmup"]) == (4, 2)
        assert out["config"]["thermo_steps_in_timed_region"] == 1
    assert not FULL_ONLY & set(plain) and "newton_evals_per_solve" not in plain["config"], sorted(plain)
    assert FULL_ONLY <= set(full) and "newton_evals_per_solve" in full["config"], sorted(full)
    assert plain["restart_checksums"] == full["restart_checksums"]
    shapes = plain["dumped_outputs"]["shapes"]
    assert shapes == full["dumped_outputs"]["shapes"] and {"u", "v", "h", "T", "S"} <= set(shapes)
    for name in shapes:
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert np.array_equal(a, b), name
