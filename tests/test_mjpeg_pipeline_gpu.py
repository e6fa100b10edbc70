"""GPU: the JPEG encoder through the drivers.  ClipPipeline(jpeg=...) hands out, per frame, exactly the bytes MjpegEncoder gives for
the frame the pipeline without `jpeg` returns, with and without the raw download; deploy_bundle.py --mjpg writes the two .avi files of
the reference's loop (first frame + every stabilised frame; the crop), identical between the serial and the --pipeline loop, without
changing the .npy outputs; and such an .avi can be read back as an input clip."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import riff_walk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clip(H, W, T):
    from stabnet_amd import synthetic
    grey = synthetic.make_clip(H, W, T, seed=11).astype(np.float32)
    g8 = ((grey + 0.5) * 255).clip(0, 255)
    bgr = np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)
    return grey, bgr


@pytest.mark.parametrize("colour", [True, False])
def test_pipeline_jpeg_equals_encoder_on_the_pipeline_frame(cuda, colour):
    import torch
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import ClipPipeline, StabNetStream
    from stabnet_amd.mjpeg import MjpegEncoder
    H, W, T = 144, 176, 13
    cfg = Config(height=H, width=W)
    params = synthetic.make_params(cfg, seed=3, theta_scale=0.2)
    grey, bgr = _clip(H, W, T)
    stream = lambda: StabNetStream(params, H, W, cfg, device=cuda, use_graph=True)
    opts = dict(quality=80, subsampling="420", restart_mcus=2)
    plain = ClipPipeline(stream(), colour=colour).run(grey, bgr if colour else None)
    assert len(plain) == T - 1 and all("jpeg" not in r for r in plain)
    enc = MjpegEncoder(H, W, 3 if colour else 1, device=cuda, **opts)
    key = "bgr" if colour else "output"
    want = [enc.encode_bytes(torch.from_numpy(r[key]).to(cuda))[0] for r in plain]
    assert len(set(want)) == T - 1
    pipe = ClipPipeline(stream(), colour=colour, jpeg=opts)
    both = pipe.run(grey, bgr if colour else None)
    assert [r["t"] for r in both] == list(range(1, T))
    for r, p, w in zip(both, plain, want):
        assert bytes(r["jpeg"]) == w, r["t"]
        assert np.array_equal(r["output"], p["output"]) and (not colour or np.array_equal(r["bgr"], p["bgr"]))
    seen = []
    pipe.run(grey, bgr if colour else None, raw=False, sink=lambda r: seen.append((sorted(r), bytes(r["jpeg"]))))
    assert [s[1] for s in seen] == want
    assert all(s[0] == ["jpeg", "t"] for s in seen)
    assert 0 < pipe.jpeg_bytes_down < (T - 1) * H * W * (3 if colour else 1)
    # a chunk smaller than the frames: the rest arrives by the second copy, same bytes
    pipe.jpeg_chunk = 256
    assert [bytes(r["jpeg"]) for r in pipe.run(grey, bgr if colour else None, raw=False)] == want
    from stabnet_amd import _lib
    with pytest.raises(_lib.StabnetError):
        ClipPipeline(stream(), colour=colour).run(grey, bgr if colour else None, raw=False)


def _deploy(out_dir, *extra, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", "144", "--width", "176", "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def test_deploy_bundle_writes_the_reference_videos(cuda, tmp_path):
    import torch
    from PIL import Image
    from stabnet_amd.avi import AviMjpegReader
    from stabnet_amd.mjpeg import MjpegEncoder
    H, W, T = 144, 176, 12
    base = ["--synthetic", str(T)]
    _deploy(tmp_path / "plain", *base)
    _deploy(tmp_path / "serial", *base, "--mjpg")
    _deploy(tmp_path / "pipe", *base, "--mjpg", "--pipeline")
    f = lambda d, n: str(tmp_path / d / "output" / n)
    # the .npy outputs do not change
    for n in ("synthetic_stable.npy", "synthetic_maps.npz", "synthetic_cut.npy"):
        ref = open(f("plain", n), "rb").read()
        assert open(f("serial", n), "rb").read() == ref, n
    assert not os.path.exists(f("plain", "synthetic.avi"))
    stable = np.load(f("serial", "synthetic_stable.npy"))
    cut = np.load(f("serial", "synthetic_cut.npy"))
    assert stable.shape == (T - 1, H, W) and stable.dtype == np.uint8
    assert np.array_equal(np.load(f("pipe", "synthetic_stable.npy")), stable)
    enc = MjpegEncoder(H, W, 1, device=cuda)                          # the driver's defaults: q75, 4:2:0 (ignored for grey)
    t = riff_walk.walk(f("serial", "synthetic.avi"))
    assert len(t["frames"]) == T and t["avih"][4] == T and (t["strf"]["width"], t["strf"]["height"]) == (W, H)
    assert t["strh"]["rate"] / t["strh"]["scale"] == 30.0
    for i in range(T):
        im = Image.open(io.BytesIO(riff_walk.jpeg_of(t, i)))
        im.load()
        assert im.size == (W, H) and im.mode == "L"
    for i in range(1, T):
        assert riff_walk.jpeg_of(t, i) == enc.encode_bytes(torch.from_numpy(stable[i - 1]).to(cuda))[0], i
    # frame 0 is the unprocessed first frame: close to the first stabilised frame's source, not equal to any stabilised frame
    assert riff_walk.jpeg_of(t, 0) not in [riff_walk.jpeg_of(t, i) for i in range(1, T)]
    c = riff_walk.walk(f("serial", "synthetic_cut.avi"))
    assert len(c["frames"]) == T - 1 and (c["strf"]["width"], c["strf"]["height"]) == (cut.shape[2], cut.shape[1])
    cenc = MjpegEncoder(cut.shape[1], cut.shape[2], 1, device=cuda)
    for i in range(T - 1):
        assert riff_walk.jpeg_of(c, i) == cenc.encode_bytes(torch.from_numpy(np.ascontiguousarray(cut[i])).to(cuda))[0]
        assert Image.open(io.BytesIO(riff_walk.jpeg_of(c, i))).size == (cut.shape[2], cut.shape[1])
    # the two loops write the same files
    for n in ("synthetic.avi", "synthetic_cut.avi"):
        assert open(f("pipe", n), "rb").read() == open(f("serial", n), "rb").read(), n
    # the project reads what it writes: the .avi as the input clip
    prefix = tmp_path / "data"
    os.makedirs(prefix / "unstable")
    os.replace(f("serial", "synthetic.avi"), str(prefix / "unstable" / "again.avi"))
    (tmp_path / "list").write_text("again.avi\n")
    out = _deploy(tmp_path / "again", "--test-list", str(tmp_path / "list"), "--prefix", str(prefix), "--mjpg", "--fps", "12")
    assert "decoded on the host with Pillow" in out
    r = AviMjpegReader(f("again", "again.avi"))
    assert len(r) == T and r.size == (W, H) and r.fps == 30.0          # the input's rate wins over --fps
    assert np.load(f("again", "again_stable.npy")).shape == (T - 1, H, W)
