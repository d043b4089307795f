"""bench.py's plain run (no --full): the headline line alone, and --dump-outputs DIR with the final state of the last timed step.
Checked: the line's headline fields, none of the --full legs, the dumped arrays (float64, the shapes of lidar_imu_init_amd.State) and
that the dumped pose is the line's last_state_pose."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--workload", "vlp16",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1, p.stdout[-3000:]
    d = json.loads(rows[0])
    assert d["steps"] == 12 and d["value"] > 0 and d["unit"] == "scans/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    for leg in ("value_long", "roofline", "cpu_baseline", "parity", "calibration", "complete_pipeline"):
        assert leg not in d, leg
    shapes = {"rot_end": (3, 3), "pos_end": (3,), "offset_R_L_I": (3, 3), "offset_T_L_I": (3,), "vel_end": (3,), "bias_g": (3,),
              "bias_a": (3,), "gravity": (3,), "cov": (24, 24)}
    got = {}
    for name, shape in shapes.items():
        a = np.load(out_dir / (name + ".npy"))
        assert a.dtype == np.float64 and a.shape == shape, (name, a.dtype, a.shape)
        assert np.all(np.isfinite(a)), name
        got[name] = a
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in shapes)
    np.testing.assert_array_equal(np.r_[got["rot_end"].reshape(-1), got["pos_end"]], np.array(d["last_state_pose"]))
