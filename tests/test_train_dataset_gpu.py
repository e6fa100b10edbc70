"""GPU: train_bundle_nobm.py --data-dir as a user runs it -- a fresh child process reads TFRecord files and JPEG frames written here,
trains two steps (the second one also runs the ten held-out batches of test/) and prints a finite loss; with a frame file missing it
ends with a message that names the file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dataset_fixture import samples, write_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(data_dir, model_dir):
    cmd = [sys.executable, os.path.join(ROOT, "train_bundle_nobm.py"), "--data-dir", data_dir, "--no-imagenet-init", "--iters", "2",
           "--batch-size", "2", "--height", "64", "--width", "96", "--model-dir", model_dir]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_driver_trains_from_a_dataset_and_names_a_missing_frame(cuda, tmp_path):
    from stabnet_amd.dataset import write_dataset
    d = str(tmp_path / "data")
    write_frames(d)
    s = samples((64, 96), flow=False)
    write_dataset(d, "train", s[:8])
    write_dataset(d, "test", s[8:])
    r = _run(d, str(tmp_path / "models"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("final loss")]
    assert len(last) == 1 and np.isfinite(float(last[0].split()[-1])), r.stdout[-2000:]
    assert "Test Loss" in r.stdout and "train: 8 records" in r.stdout

    write_dataset(d, "train", [s[2]])                               # clip 0 at pos 36, whatever the shuffle draws
    missing = os.path.join(d, "unstable", "0", "36.jpg")
    os.remove(missing)
    r = _run(d, str(tmp_path / "models2"))
    assert r.returncode != 0
    assert missing in r.stderr and "Traceback" not in r.stderr, r.stderr[-3000:]
