"""``python bench.py --gpus 1`` as a plain command: only the headline is measured, exactly ``--steps`` steps are timed, and
``--dump-outputs DIR`` writes the frames of the last timed step -- the same frames from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "frames.npy"))


def test_plain_bench_times_the_headline_only_and_dumps_its_frames(tmp_path):
    assert torch.cuda.is_available()
    line, frames = _plain_run(tmp_path / "a")
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 4 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert len(line["timed_blocks"]["ms_per_step"]) == 1 and line["ms_per_step"] == line["timed_blocks"]["ms_per_step"][0]
    assert line["value"] > 0 and abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) < 1e-2 * line["value"]
    for extra in ("roofline", "eager", "cpu_baseline", "bf16x3", "train_step", "single_frame"):
        assert extra not in line, extra
    assert frames.dtype == np.float32 and frames.shape == (8, 3, 256, 256)
    assert np.isfinite(frames).all() and frames.std() > 0
    _, again = _plain_run(tmp_path / "b")
    assert rel_l2(again, frames) < 1e-6
