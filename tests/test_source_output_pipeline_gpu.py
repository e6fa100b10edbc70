"""GPU: output at source resolution through the drivers (network 64x96, source 160x240 BGR, 5 frames).  ClipPipeline(output="source")
hands out the bytes of a serial loop of step_u8 + warp.warpRevBundle2_src + MjpegEncoder at the source's size, eagerly and from its
graphs; the default output is what it was; deploy_bundle.py --output-size source writes the clip, the colour frames and the crop at
the size of the frames it read, the same bytes with and without --pipeline."""
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_src_model as M
import riff_walk
from oracle import stabnet_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, SH, SW, T = 64, 96, 160, 240, 5


def _clip(sh, sw, n, seed=11):
    """uint8 BGR [n, sh, sw, 3]: the synthetic shaky clip, tinted."""
    from stabnet_amd import synthetic
    g8 = ((synthetic.make_clip(sh, sw, n, seed=seed).astype(np.float32) + 0.5) * 255).clip(0, 255)
    return np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)


def _setup(cuda, channels=3):
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    from stabnet_amd.ingest import FrameIngest
    cfg = Config(height=H, width=W)
    params = synthetic.make_params(cfg, seed=3, theta_scale=0.2)
    stream = lambda **kw: StabNetStream(params, H, W, cfg, device=cuda, **kw)
    return stream, FrameIngest(SH, SW, channels, H, W, device=cuda)


def test_pipeline_at_source_size_equals_the_serial_loop(cuda):
    import torch
    from stabnet_amd import _lib, warp
    from stabnet_amd.deploy import ClipPipeline
    from stabnet_amd.mjpeg import MjpegEncoder
    stream, ing = _setup(cuda)
    bgr = _clip(SH, SW, T)
    opts = dict(quality=80, subsampling="420", restart_mcus=2)
    enc = MjpegEncoder(SH, SW, 3, device=cuda, **opts)
    s = stream(use_graph=True)
    s.start_u8(torch.from_numpy(bgr[0:1]).to(cuda), ing)
    acc = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    serial = []
    for t in range(1, T):
        raw = torch.from_numpy(bgr[t:t + 1]).to(cuda)
        r = s.step_u8(raw, ing)
        out = ((r["output"][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8)
        warped = warp.warpRevBundle2_src(raw[0], r["x_map"], r["y_map"], black_count=acc)
        if t == 1:                                                         # the serial loop itself against the model, once
            want, _, _, blk = M.warp_src(bgr[t], r["x_map"][0, :, :, 0].cpu().numpy(), r["y_map"][0, :, :, 0].cpu().numpy())
            assert np.array_equal(warped.cpu().numpy(), want) and np.array_equal(acc.cpu().numpy(), blk.astype(np.int32))
        serial.append((out, warped.cpu().numpy(), enc.encode_bytes(warped)[0]))
    acc = acc.cpu().numpy()
    pipe = ClipPipeline(stream(use_graph=True), colour=True, jpeg=opts, ingest=ing, output="source")
    assert not hasattr(pipe, "d_bgr") and pipe.h_warp[0].shape == (SH, SW, 3) and (pipe.enc.H, pipe.enc.W) == (SH, SW)
    for rnd in range(2):                                                   # first use of every slot runs eagerly, then its graph replays
        got = pipe.run(bgr)
        assert [r["t"] for r in got] == list(range(1, T))
        for r, (out, col, jpg) in zip(got, serial):
            assert np.array_equal(r["output"], out), (rnd, r["t"])
            assert r["bgr"].shape == (SH, SW, 3) and np.array_equal(r["bgr"], col), (rnd, r["t"])
            assert bytes(r["jpeg"]) == jpg, (rnd, r["t"])
        assert np.array_equal(pipe.all_black_src.cpu().numpy(), acc), rnd   # zeroed by run, counted inside the graphs
    assert len(pipe._graphs) == pipe.slots and all(g is not None for g in pipe._graphs.values())
    assert len(set(j for _, _, j in serial)) == T - 1 and acc.max() >= 1
    with pytest.raises(_lib.StabnetError):
        ClipPipeline(stream(), colour=True, output="source")                 # no ingest: the raw frame is not on the device
    with pytest.raises(_lib.StabnetError):
        ClipPipeline(stream(), colour=False, ingest=ing, output="source")     # the grey frame of a BGR source does not exist at its size
    with pytest.raises(_lib.StabnetError):
        ClipPipeline(stream(), colour=True, ingest=ing, output="both")


def test_grey_source_at_source_size(cuda):
    import torch
    from stabnet_amd import warp
    from stabnet_amd.deploy import ClipPipeline
    stream, ing = _setup(cuda, channels=1)
    grey = np.ascontiguousarray(_clip(SH, SW, T)[..., 1])
    s = stream(use_graph=True)
    s.start_u8(torch.from_numpy(grey[0:1]).to(cuda), ing)
    serial = []
    for t in range(1, T):
        raw = torch.from_numpy(grey[t]).to(cuda)
        r = s.step_u8(raw, ing)
        serial.append(warp.warpRevBundle2_src(raw, r["x_map"], r["y_map"]).cpu().numpy())
    got = ClipPipeline(stream(use_graph=True), colour=False, ingest=ing, output="source").run(grey)
    for r, w in zip(got, serial):
        assert r["bgr"].shape == (SH, SW) and np.array_equal(r["bgr"], w), r["t"]


def test_default_output_is_what_it_was(cuda):
    """output="network" (the default): resize, then remap, at the network's size -- the serial loop's bytes, as before."""
    import torch
    from stabnet_amd import warp
    from stabnet_amd.deploy import ClipPipeline
    from stabnet_amd.mjpeg import MjpegEncoder
    stream, ing = _setup(cuda)
    bgr = _clip(SH, SW, T)
    opts = dict(quality=80, subsampling="420", restart_mcus=2)
    enc = MjpegEncoder(H, W, 3, device=cuda, **opts)
    s = stream(use_graph=True)
    s.start_u8(torch.from_numpy(bgr[0:1]).to(cuda), ing)
    serial = []
    for t in range(1, T):
        raw = torch.from_numpy(bgr[t:t + 1]).to(cuda)
        r = s.step_u8(raw, ing)
        warped = warp.warpRevBundle2(ing.colour(raw)[0], r["x_map"], r["y_map"])
        serial.append((warped.cpu().numpy(), enc.encode_bytes(warped)[0]))
    for kw in ({}, dict(output="network")):
        pipe = ClipPipeline(stream(use_graph=True), colour=True, jpeg=opts, ingest=ing, **kw)
        assert not pipe.src_out and not hasattr(pipe, "all_black_src") and pipe.h_warp[0].shape == (H, W, 3)
        for rnd in range(2):
            for r, (col, jpg) in zip(pipe.run(bgr), serial):
                assert np.array_equal(r["bgr"], col) and bytes(r["jpeg"]) == jpg, (kw, rnd, r["t"])


def _deploy(out_dir, *extra, timeout=300, ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(H), "--width", str(W), "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if not ok:
        return r
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def test_deploy_bundle_writes_at_source_size(cuda, tmp_path):
    import torch
    from stabnet_amd.mjpeg import MjpegEncoder
    n, sh, sw = 5, 90, 150
    clip = _clip(sh, sw, n, seed=4)
    prefix = tmp_path / "data"
    os.makedirs(prefix / "unstable")
    np.save(str(prefix / "unstable" / "shaky.npy"), clip)
    (tmp_path / "list").write_text("shaky.npy\n")
    base = ["--test-list", str(tmp_path / "list"), "--prefix", str(prefix), "--mjpg", "--ingest", "device"]
    f = lambda d, name: str(tmp_path / d / "output" / name)
    out = _deploy(tmp_path / "src", *base, "--output-size", "source")
    assert "--output-size source: frames are written at %dx%d" % (sw, sh) in out
    _deploy(tmp_path / "net", *base)
    # what stays at the network's size is what the default run writes
    for name in ("shaky_stable.npy", "shaky_maps.npz"):
        assert open(f("src", name), "rb").read() == open(f("net", name), "rb").read(), name
    assert np.load(f("net", "shaky_stable_bgr.npy")).shape == (n - 1, H, W, 3)
    colour = np.load(f("src", "shaky_stable_bgr.npy"))
    assert colour.shape == (n - 1, sh, sw, 3) and colour.dtype == np.uint8
    # every colour frame is the model's warp of the frame as read by the maps the run saved; the coverage accumulates beside
    maps = np.load(f("src", "shaky_maps.npz"))
    acc = np.zeros((sh, sw), np.int64)
    for i in range(n - 1):
        want, _, _, blk = M.warp_src(clip[i + 1], maps["x_map"][i], maps["y_map"][i])
        assert np.array_equal(colour[i], want), i
        acc += blk
    t = riff_walk.walk(f("src", "shaky.avi"))
    assert len(t["frames"]) == n and (t["strf"]["width"], t["strf"]["height"]) == (sw, sh)
    enc = MjpegEncoder(sh, sw, 3, device=cuda)                            # the driver's defaults: q75, 4:2:0
    assert riff_walk.jpeg_of(t, 0) == enc.encode_bytes(torch.from_numpy(clip[0]).to(cuda))[0]      # the first frame as read
    for i in range(1, n):
        assert riff_walk.jpeg_of(t, i) == enc.encode_bytes(torch.from_numpy(colour[i - 1]).to(cuda))[0], i
    # the crop: the rectangle the model's accumulated coverage gives, cut at source resolution
    ans, area = O.max_inscribed_rect(acc)
    names = ["shaky_stable.npy", "shaky_stable_bgr.npy", "shaky_maps.npz", "shaky.avi"]
    print("coverage: %d of %d pixels black in some frame; crop %s" % (int((acc > 0).sum()), acc.size, ans))
    if ans:
        ch, cw = ans[2] - ans[0] + 1, ans[3] - ans[1] + 1
        assert "crop %s area %d" % (ans, area) in out
        cut = np.load(f("src", "shaky_cut.npy"))
        assert cut.shape == (n - 1, ch, cw, 3) and np.array_equal(cut, colour[:, ans[0]:ans[2] + 1, ans[1]:ans[3] + 1])
        c = riff_walk.walk(f("src", "shaky_cut.avi"))
        assert len(c["frames"]) == n - 1 and (c["strf"]["width"], c["strf"]["height"]) == (cw, ch)
        names += ["shaky_cut.npy", "shaky_cut.avi"]
    else:                                                                 # no black-free start pixel: nothing is cut
        assert not os.path.exists(f("src", "shaky_cut.npy")) and not os.path.exists(f("src", "shaky_cut.avi"))
    # the pipelined loop writes the same files
    _deploy(tmp_path / "pipe", *base, "--output-size", "source", "--pipeline")
    for name in names:
        assert open(f("pipe", name), "rb").read() == open(f("src", name), "rb").read(), name


def test_source_size_needs_the_device_ingest(tmp_path):
    r = _deploy(tmp_path / "bad", "--synthetic", "3", "--output-size", "source", ok=False)
    assert r.returncode != 0 and "--ingest device" in r.stderr
    r = _deploy(tmp_path / "bad", "--synthetic", "3", "--ingest", "host", "--output-size", "source", ok=False)
    assert r.returncode != 0
