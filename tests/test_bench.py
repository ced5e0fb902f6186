"""bench.py's own contract: a plain run times --steps steps and reports them, and --dump-outputs writes what the last timed
step computed as <name>.npy (float32 / float64, fixed samples of large arrays, under 64 MB) so that two builds can be
compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_dump_outputs_format_and_fixed_samples(tmp_path):
    import bench
    big = torch.arange(3 * bench.DUMP_SAMPLE_DEFAULT, dtype=torch.float32).reshape(3, -1)
    arrays = {"loss": torch.tensor(2.5), "state.w": big, "state.n": torch.tensor([7], dtype=torch.int64),
              "state.small": torch.ones(4, 5, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert got["loss"].dtype == np.float32 and float(got["loss"]) == 2.5
    assert got["state.n"].dtype == np.float64 and got["state.n"].tolist() == [7.0]
    assert got["state.small"].dtype == np.float64 and got["state.small"].shape == (4, 5)
    w = got["state.w"]
    assert w.dtype == np.float32 and w.shape == (bench.DUMP_SAMPLE_DEFAULT,)
    assert np.all(np.diff(w) > 0) and np.array_equal(w, np.unique(w))       # distinct elements, in index order
    for n in arrays:                                                         # the same sample in every run
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy")), n


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--frames", "4", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "video-text pairs/s" and out["dtype"] == "f16" and out["metric"]
    for key in ("roofline", "roofline_hbm", "vit_forward", "comm", "ms_per_step_unfolded"):
        assert out[key] is None, key
    assert "cpu_baseline" not in out
    files = sorted(os.listdir(out_dir))
    assert "loss.npy" in files and "grad_norm.npy" in files and len(files) > 100
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 * 2 ** 20
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), f
    assert abs(float(np.load(out_dir / "loss.npy")) - out["final_loss"]) < 1e-3
