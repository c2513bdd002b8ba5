"""bench.py's command line: a plain run (no --full) times exactly `--steps` steps and measures nothing else; --dump-outputs
writes what the last timed step computed, within 64 MB, the same from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["image", "radii", "depth_alpha", "means2D_grad", "means3D_grad", "shs_grad", "opacities_grad", "scales_grad",
         "rotations_grad"]
FULL_ONLY = ["dropin_views_per_s", "sustained", "rotating_cameras", "training_like", "trainer_step", "init_state",
             "forward_only", "roofline", "exchange", "rccl", "cpu_baseline", "max_grad_err_vs_oracle"]


def test_write_outputs_samples_within_the_budget(tmp_path):
    import bench
    big = np.arange(12_000_000, dtype=np.float32).reshape(4, 3, 1000, 1000)
    arrays = {"big": big, "wide": np.ones((5_000_000, 3), np.float64), "ints": np.arange(7, dtype=np.int32),
              "small": np.full((2, 5), 0.5, np.float32)}
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{n}.npy" for n in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert got["ints"].dtype == np.float32 and np.array_equal(got["ints"], np.arange(7))
    assert got["wide"].dtype == np.float64 and got["big"].dtype == np.float32
    assert np.array_equal(got["small"], arrays["small"])
    # the sample: distinct entries in index order (arange makes value = flat index), the same in every run
    s = got["big"]
    assert 0 < s.size < big.size and (np.diff(s) > 0).all()
    for n in arrays:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--gaussians",
           "20000", "--res", "256", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(built_lib, tmp_path):
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        line = _plain_run(d)
        assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert line["unit"] == "views/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
        # value = views per second of the same timed region: 4 views per step
        assert abs(line["value"] * line["ms_per_step"] / 4e3 - 1) < 1e-2, (line["value"], line["ms_per_step"])
        assert all(line[key] is None for key in FULL_ONLY), {key: line[key] for key in FULL_ONLY if line[key] is not None}
        files = sorted(os.listdir(d))
        assert files == sorted(f"{n}.npy" for n in NAMES)
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        runs.append({n: np.load(d / f"{n}.npy") for n in NAMES})
    a, b = runs
    assert a["image"].shape == (4, 3, 256, 256) and a["means2D_grad"].shape == (4, 20000, 3)
    assert a["shs_grad"].shape == (20000, 16, 3)
    for n in NAMES:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
    assert a["image"].std() > 0 and np.abs(a["means3D_grad"]).max() > 0
    assert np.array_equal(a["radii"], b["radii"])
    for n in NAMES:
        np.testing.assert_allclose(a[n], b[n], rtol=0, atol=1e-5 * max(1e-6, float(np.abs(a[n]).max())), err_msg=n)
