"""GPU: deploy_bundle.py --decode device.  A short Motion-JPEG .avi (8 frames of 64x96, Pillow-encoded with restart intervals, written
with AviMjpegWriter) goes through the driver with its frames decoded on the GPU, serially and with --pipeline: every output file is
the --decode host run's, byte for byte (the .npz by its arrays).  A 4:2:2 clip, which the device decoder does not take, falls back to
Pillow with a note and gives the same files too."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 64, 96, 8


def _frames():
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H + 16, 0:W + 16].astype(np.float64)
    big = np.stack([128 + 100 * np.sin(x / 6.0 + y / 9.0), 128 + 90 * np.cos(x / 4.0 - y / 7.0), 30 + 2.0 * x + 1.5 * y], -1)
    big = np.clip(big + rng.normal(0, 6.0, big.shape), 0, 255).astype(np.uint8)
    shake = rng.integers(0, 16, (T, 2))
    return [np.ascontiguousarray(big[dy:dy + H, dx:dx + W]) for dy, dx in shake]


def _write_clip(path, **opts):
    from PIL import Image
    from stabnet_amd.avi import AviMjpegWriter
    with AviMjpegWriter(str(path), W, H, 25) as w:
        for f in _frames():
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, "JPEG", quality=85, **opts)
            w.write(buf.getvalue())


def _deploy(prefix, out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(H), "--width", str(W), "--output-dir", str(out_dir),
           "--test-list", str(prefix / "list"), "--prefix", str(prefix), "--ingest", "device", "--mjpg"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    """The clips and their --decode host outputs, made once: {kind: (prefix, output directory, stdout)}."""
    runs = {}
    for kind, opts in (("420", dict(subsampling="4:2:0", restart_marker_blocks=2)), ("422", dict(subsampling="4:2:2"))):
        prefix = tmp_path_factory.mktemp("data" + kind)
        os.makedirs(prefix / "unstable")
        _write_clip(prefix / "unstable" / "clip.avi", **opts)
        (prefix / "list").write_text("clip.avi\n")
        out = tmp_path_factory.mktemp("host" + kind)
        runs[kind] = (prefix, out, _deploy(prefix, out, "--decode", "host"))
    return runs


def _same_files(a, b):
    names = sorted(os.listdir(a / "output"))
    assert names == sorted(os.listdir(b / "output"))
    assert {"clip.avi", "clip_stable.npy", "clip_stable_bgr.npy", "clip_maps.npz"} <= set(names)
    for n in names:
        if n.endswith(".npz"):
            za, zb = np.load(a / "output" / n), np.load(b / "output" / n)
            assert za.files == zb.files and all(np.array_equal(za[k], zb[k]) for k in za.files), n
        else:
            assert open(a / "output" / n, "rb").read() == open(b / "output" / n, "rb").read(), n


@pytest.mark.parametrize("loop", ["serial", "pipeline"])
def test_device_decode_writes_the_host_decode_files(cuda, host_runs, tmp_path, loop):
    prefix, host_out, host_stdout = host_runs["420"]
    assert "decoded on the host with Pillow" in host_stdout
    stdout = _deploy(prefix, tmp_path, "--decode", "device", *(["--pipeline"] if loop == "pipeline" else []))
    assert "decoded on the GPU frame by frame (one lane per restart interval)" in stdout and "Pillow" not in stdout
    _same_files(host_out, tmp_path)
    assert np.load(tmp_path / "output" / "clip_stable_bgr.npy").shape == (T - 1, H, W, 3)


def test_unsupported_clip_falls_back_to_pillow(cuda, host_runs, tmp_path):
    prefix, host_out, _ = host_runs["422"]
    stdout = _deploy(prefix, tmp_path, "--decode", "device")
    assert "note: --decode device:" in stdout and "unsupported" in stdout and "decoded on the host with Pillow" in stdout
    _same_files(host_out, tmp_path)
