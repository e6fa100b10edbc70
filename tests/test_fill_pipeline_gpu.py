"""GPU: borderless output through the drivers (network 64x96, source 160x240 BGR, 5 frames).  ClipPipeline(window=...) hands out the
bytes of a serial loop of step_u8 + warp.warpRevBundle2_win + MjpegEncoder, at source size and at the network's size, eagerly and
from its graphs, with the coverage counted at the output pixels; without a window it gives what it gave; deploy_bundle.py --fill R
writes the same files with and without --pipeline, and --fill auto adds the second pass's files to an otherwise unchanged run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_win_model as WM
import riff_walk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, SH, SW, T = 64, 96, 160, 240, 5
OPTS = dict(quality=80, subsampling="420", restart_mcus=2)


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


def _serial(cuda, stream, ing, bgr, window, source):
    """The loop one frame at a time: [(network output, kept frame, its JPEG)], the coverage counts; frame 1 against the model."""
    import torch
    from stabnet_amd import warp
    from stabnet_amd.mjpeg import MjpegEncoder
    kh, kw = (SH, SW) if source else (H, W)
    enc = MjpegEncoder(kh, kw, 3, device=cuda, **OPTS)
    s = stream(use_graph=True)
    s.start_u8(torch.from_numpy(bgr[0:1]).to(cuda), ing)
    acc = torch.zeros((kh, kw), dtype=torch.int32, device=cuda)
    serial = []
    for t in range(1, T):
        raw = torch.from_numpy(bgr[t:t + 1]).to(cuda)
        r = s.step_u8(raw, ing)
        out = ((r["output"][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8)
        frame = raw[0] if source else ing.colour(raw)[0]
        warped = warp.warpRevBundle2_win(frame, r["x_map"], r["y_map"], window, black_count=acc)
        if t == 1:
            want, _, _, blk = WM.warp_win(frame.cpu().numpy(), r["x_map"][0, :, :, 0].cpu().numpy(), r["y_map"][0, :, :, 0].cpu().numpy(), window)
            assert np.array_equal(warped.cpu().numpy(), want) and np.array_equal(acc.cpu().numpy(), blk.astype(np.int32))
        serial.append((out, warped.cpu().numpy(), enc.encode_bytes(warped)[0]))
    return serial, acc.cpu().numpy()


@pytest.mark.parametrize("output", ["source", "network"])
def test_pipeline_with_a_window_equals_the_serial_loop(cuda, output):
    from stabnet_amd.deploy import ClipPipeline
    from stabnet_amd.warp import ratio_window
    stream, ing = _setup(cuda)
    bgr = _clip(SH, SW, T)
    source = output == "source"
    kh, kw = (SH, SW) if source else (H, W)
    window = ratio_window(kh, kw, 0.8)
    serial, acc = _serial(cuda, stream, ing, bgr, window, source)
    pipe = ClipPipeline(stream(use_graph=True), colour=True, jpeg=OPTS, ingest=ing, output=output, window=window)
    assert pipe.h_warp[0].shape == (kh, kw, 3) and (pipe.enc.H, pipe.enc.W) == (kh, kw) and pipe.all_black_win.shape == (kh, kw)
    for rnd in range(2):                                                   # first use of every slot runs eagerly, then its graph replays
        got = pipe.run(bgr)
        assert [r["t"] for r in got] == list(range(1, T))
        for r, (out, col, jpg) in zip(got, serial):
            assert np.array_equal(r["output"], out), (rnd, r["t"])
            assert r["bgr"].shape == (kh, kw, 3) and np.array_equal(r["bgr"], col), (rnd, r["t"])
            assert bytes(r["jpeg"]) == jpg, (rnd, r["t"])
        assert np.array_equal(pipe.all_black_win.cpu().numpy(), acc), rnd   # zeroed by run, counted inside the graphs
        if source:
            assert int(pipe.all_black_src.sum()) == 0                       # not updated with a window
    assert len(pipe._graphs) == pipe.slots and all(g is not None for g in pipe._graphs.values())
    assert len(set(j for _, _, j in serial)) == T - 1


def test_without_a_window_nothing_changes(cuda):
    import torch
    from stabnet_amd import warp
    from stabnet_amd.deploy import ClipPipeline
    from stabnet_amd.mjpeg import MjpegEncoder
    stream, ing = _setup(cuda)
    bgr = _clip(SH, SW, T)
    enc = MjpegEncoder(SH, SW, 3, device=cuda, **OPTS)
    s = stream(use_graph=True)
    s.start_u8(torch.from_numpy(bgr[0:1]).to(cuda), ing)
    acc = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    serial = []
    for t in range(1, T):
        raw = torch.from_numpy(bgr[t:t + 1]).to(cuda)
        r = s.step_u8(raw, ing)
        warped = warp.warpRevBundle2_src(raw[0], r["x_map"], r["y_map"], black_count=acc)
        serial.append((warped.cpu().numpy(), enc.encode_bytes(warped)[0]))
    for kw in ({}, dict(window=None)):
        pipe = ClipPipeline(stream(use_graph=True), colour=True, jpeg=OPTS, ingest=ing, output="source", **kw)
        assert pipe.window is None and not hasattr(pipe, "all_black_win")
        for rnd in range(2):
            for r, (col, jpg) in zip(pipe.run(bgr), serial):
                assert np.array_equal(r["bgr"], col) and bytes(r["jpeg"]) == jpg, (kw, rnd, r["t"])
            assert np.array_equal(pipe.all_black_src.cpu().numpy(), acc.cpu().numpy())


def test_refusals(cuda):
    from stabnet_amd import _lib
    from stabnet_amd.deploy import ClipPipeline
    stream, ing = _setup(cuda)
    _, grey = _setup(cuda, channels=1)
    st = stream()                                                              # a refused pipeline leaves the stream as it was
    with pytest.raises(_lib.StabnetError, match="window"):
        ClipPipeline(st, colour=False, window=(0, 0, H, W))                                    # keeps the network's grey output
    with pytest.raises(_lib.StabnetError, match="window"):
        ClipPipeline(st, colour=False, ingest=grey, window=(0, 0, H, W))
    for bad in ((0, 0, SH, SW + 1), (-1, 0, SH, SW), (0, 0, 0, SW), (0, 0, SH), (0, 0, float("nan"), SW), "auto"):
        with pytest.raises(_lib.StabnetError, match="window"):
            ClipPipeline(st, colour=True, ingest=ing, output="source", window=bad)
    with pytest.raises(_lib.StabnetError, match="window"):
        ClipPipeline(st, colour=True, ingest=ing, window=(0, 0, SH, SW))                        # the kept frame is HxW here
    # a grey source at its own size has a remapped frame to cut
    assert ClipPipeline(st, colour=False, ingest=grey, output="source", window=(0, 0, SH, SW)).all_black_win.shape == (SH, SW)


def _deploy(out_dir, *extra, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(H), "--width", str(W), "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def _data(tmp_path, n=5, sh=90, sw=150):
    clip = _clip(sh, sw, n, seed=4)
    prefix = tmp_path / "data"
    os.makedirs(prefix / "unstable")
    np.save(str(prefix / "unstable" / "shaky.npy"), clip)
    (tmp_path / "list").write_text("shaky.npy\n")
    return clip, ["--test-list", str(tmp_path / "list"), "--prefix", str(prefix), "--mjpg", "--ingest", "device", "--output-size", "source"]


def test_deploy_bundle_fill_ratio_serial_and_pipelined(cuda, tmp_path):
    import torch
    from stabnet_amd.mjpeg import MjpegEncoder
    from stabnet_amd.warp import ratio_window
    n, sh, sw = 5, 90, 150
    clip, base = _data(tmp_path, n, sh, sw)
    f = lambda d, name: str(tmp_path / d / "output" / name)
    out = _deploy(tmp_path / "ser", *base, "--fill", "0.8")
    assert "left some pixel uncovered" in out and "fps=" in out
    window = ratio_window(sh, sw, 0.8)
    info = json.load(open(f("ser", "shaky_fill_window.json")))
    assert tuple(info["window"]) == window and info["rect"] is None and info["output_size"] == [sh, sw]
    # every kept frame is the model's window of the frame as read by the maps the run saved
    colour, maps = np.load(f("ser", "shaky_stable_bgr.npy")), np.load(f("ser", "shaky_maps.npz"))
    assert colour.shape == (n - 1, sh, sw, 3)
    per = []
    for i in range(n - 1):
        want, _, _, blk = WM.warp_win(clip[i + 1], maps["x_map"][i], maps["y_map"][i], window)
        assert np.array_equal(colour[i], want), i
        per.append(int(blk.sum()))
    assert info["uncovered"]["per_frame"] == per and info["uncovered"]["frames_uncovered"] == sum(1 for c in per if c)
    t = riff_walk.walk(f("ser", "shaky.avi"))
    enc = MjpegEncoder(sh, sw, 3, device=cuda)
    assert len(t["frames"]) == n and riff_walk.jpeg_of(t, 0) == enc.encode_bytes(torch.from_numpy(clip[0]).to(cuda))[0]
    for i in range(1, n):
        assert riff_walk.jpeg_of(t, i) == enc.encode_bytes(torch.from_numpy(colour[i - 1]).to(cuda))[0], i
    names = ["shaky_stable.npy", "shaky_stable_bgr.npy", "shaky_maps.npz", "shaky.avi", "shaky_fill_window.json"]
    names += [x for x in ("shaky_cut.npy", "shaky_cut.avi") if os.path.exists(f("ser", x))]
    _deploy(tmp_path / "pipe", *base, "--fill", "0.8", "--pipeline")
    assert sorted(os.listdir(tmp_path / "pipe" / "output")) == sorted(os.listdir(tmp_path / "ser" / "output"))
    for name in names:
        assert open(f("pipe", name), "rb").read() == open(f("ser", name), "rb").read(), name


def test_deploy_bundle_fill_auto_adds_a_second_pass(cuda, tmp_path):
    import torch
    from stabnet_amd.mjpeg import MjpegEncoder
    from stabnet_amd.warp import fit_window
    n, sh, sw = 5, 90, 150
    clip, base = _data(tmp_path, n, sh, sw)
    f = lambda d, name: str(tmp_path / d / "output" / name)
    out = _deploy(tmp_path / "auto", *base, "--fill", "auto")
    _deploy(tmp_path / "plain", *base)
    # everything the run wrote before is written as without --fill
    plain = sorted(os.listdir(tmp_path / "plain" / "output"))
    assert {"shaky_stable.npy", "shaky_stable_bgr.npy", "shaky_maps.npz", "shaky.avi"} <= set(plain)
    for name in plain:
        assert open(f("auto", name), "rb").read() == open(f("plain", name), "rb").read(), name
    extra = sorted(set(os.listdir(tmp_path / "auto" / "output")) - set(plain))
    if "shaky_cut.npy" not in plain:                                      # no black-free rectangle: a note, no _fill files
        assert extra == [] and "no black-free rectangle" in out
        pytest.fail("the clip of this test has no black-free rectangle: the second pass was not exercised")
    assert extra == ["shaky_fill.avi", "shaky_fill.npy", "shaky_fill_window.json"]
    assert "fill pass: fps=" in out
    info = json.load(open(f("auto", "shaky_fill_window.json")))
    rect, window = info["rect"], tuple(info["window"])
    cut = np.load(f("auto", "shaky_cut.npy"))
    assert cut.shape[1:3] == (rect[2] - rect[0] + 1, rect[3] - rect[1] + 1)
    assert window == fit_window(rect, sh, sw) and info["output_size"] == [sh, sw] and info["mode"] == "auto"
    filled, maps = np.load(f("auto", "shaky_fill.npy")), np.load(f("auto", "shaky_maps.npz"))
    assert filled.shape == (n - 1, sh, sw, 3) and filled.dtype == np.uint8
    per = []
    for i in range(n - 1):
        want, _, _, blk = WM.warp_win(clip[i + 1], maps["x_map"][i], maps["y_map"][i], window)
        assert np.array_equal(filled[i], want), i
        per.append(int(blk.sum()))
    assert info["uncovered"]["per_frame"] == per
    t = riff_walk.walk(f("auto", "shaky_fill.avi"))
    assert len(t["frames"]) == n and (t["strf"]["width"], t["strf"]["height"]) == (sw, sh)
    enc = MjpegEncoder(sh, sw, 3, device=cuda)
    assert riff_walk.jpeg_of(t, 0) == enc.encode_bytes(torch.from_numpy(clip[0]).to(cuda))[0]
    for i in range(1, n):
        assert riff_walk.jpeg_of(t, i) == enc.encode_bytes(torch.from_numpy(filled[i - 1]).to(cuda))[0], i
