"""GPU: --interp cubic through the driver (network 64x96, source 90x150 BGR, 6 frames; seeded synthetic weights).  The serial loop's kept
frames are the model's (tests/remap_cubic_model.py) over the maps it saved, at source size and at the network's size; --pipeline writes
the serial loop's bytes; the Y4M loop writes the planar model's frames; --fill adaptive keeps the wider margin and no tap of its windows
leaves the frame; --interp linear writes what a run without the flag writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import remap_cubic_model as CM
import remap_src_model as M
import remap_win_model as WM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)
H, W, SH, SW, T = 64, 96, 90, 150, 6


def _clip(sh, sw, n, seed=11):
    """uint8 BGR [n, sh, sw, 3]: the synthetic shaky clip, tinted."""
    from stabnet_amd import synthetic
    g8 = ((synthetic.make_clip(sh, sw, n, seed=seed).astype(np.float32) + 0.5) * 255).clip(0, 255)
    return np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)


def _deploy(out_dir, *extra, **kw):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(H), "--width", str(W), "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=ENV, capture_output=True, timeout=300, **kw)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert b"Traceback" not in r.stderr, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("cubic")
    clip = _clip(SH, SW, T, seed=4)
    os.makedirs(d / "data" / "unstable")
    np.save(str(d / "data" / "unstable" / "shaky.npy"), clip)
    (d / "list").write_text("shaky.npy\n")
    return d, clip, ["--test-list", str(d / "list"), "--prefix", str(d / "data"), "--ingest", "device"]


@pytest.fixture(scope="module")
def serial_source(cuda, data):
    """--output-size source --mjpg --interp cubic in the serial loop, run once and shared."""
    d, clip, base = data
    _deploy(d / "ser", *base, "--output-size", "source", "--mjpg", "--interp", "cubic")
    return d / "ser" / "output"


def test_serial_source_size_equals_the_model(cuda, data, serial_source):
    d, clip, base = data
    colour, maps = np.load(str(serial_source / "shaky_stable_bgr.npy")), np.load(str(serial_source / "shaky_maps.npz"))
    assert colour.shape == (T - 1, SH, SW, 3)
    differs = 0
    for i in range(T - 1):
        want = CM.warp_src(clip[i + 1], maps["x_map"][i], maps["y_map"][i])[0]
        assert np.array_equal(colour[i], want), i
        differs += not np.array_equal(want, M.warp_src(clip[i + 1], maps["x_map"][i], maps["y_map"][i])[0])
    assert differs == T - 1                                  # and it is not the bilinear frame


def test_pipeline_writes_the_serial_bytes(cuda, data, serial_source):
    d, clip, base = data
    _deploy(d / "pipe", *base, "--output-size", "source", "--mjpg", "--interp", "cubic", "--pipeline")
    names = sorted(os.listdir(serial_source))
    assert sorted(os.listdir(d / "pipe" / "output")) == names and "shaky.avi" in names and "shaky_stable_bgr.npy" in names
    for name in names:
        assert open(d / "pipe" / "output" / name, "rb").read() == open(serial_source / name, "rb").read(), name


def test_serial_network_size_equals_the_model(cuda, data):
    import torch
    from stabnet_amd.ingest import FrameIngest
    d, clip, base = data
    _deploy(d / "net", *base, "--interp", "cubic")
    out = d / "net" / "output"
    colour, maps = np.load(str(out / "shaky_stable_bgr.npy")), np.load(str(out / "shaky_maps.npz"))
    assert colour.shape == (T - 1, H, W, 3)
    ing = FrameIngest(SH, SW, 3, H, W, device=cuda)
    for i in range(T - 1):
        small = ing.colour(torch.from_numpy(clip[i + 1:i + 2]).to(cuda))[0].cpu().numpy()        # cv2.resize of the frame as read
        assert np.array_equal(colour[i], CM.warp_src(small, maps["x_map"][i], maps["y_map"][i])[0]), i


def test_fill_adaptive_keeps_every_tap_inside(cuda, data):
    d, clip, base = data
    _deploy(d / "fill", *base, "--output-size", "source", "--interp", "cubic", "--fill", "adaptive", "--fill-min", "0.6", "--fill-up", "0.01", "--pipeline")
    out = d / "fill" / "output"
    info = json.load(open(out / "shaky_fill_window.json"))
    assert info["interp"] == "cubic" and info["params"] == dict(r_min=0.6, up=0.01, margin_q=40)
    colour, maps = np.load(str(out / "shaky_stable_bgr.npy")), np.load(str(out / "shaky_maps.npz"))
    free = 0
    for i in range(T - 1):
        xm, ym, window = maps["x_map"][i], maps["y_map"][i], tuple(info["windows"][i])
        want, px, py, blk = CM.warp_win(clip[i + 1], xm, ym, window)
        assert np.array_equal(colour[i], want), i
        if info["r_safe"][i] >= 0.6:                          # not held at r_min: the window is provably inside the shrunk frame
            assert CM.taps_inside(px, py, SH, SW).all() and not blk.any(), i
            free += 1
    assert free >= 1


def test_y4m_loop_equals_the_planar_model(cuda, data):
    import torch
    from stabnet_amd import synthetic, y4m
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    from stabnet_amd.ingest import FrameIngest, lut256_limited
    d, clip, base = data
    f, g = str(d / "in.y4m"), str(d / "out.y4m")
    rng = np.random.default_rng(2)
    frames = []
    for t in range(T):                                       # the clip's green channel as luma, chroma planes of their own
        y = clip[t][..., 1].astype(np.float64) * (219.0 / 255.0) + 16.0
        planes = [y, 128 + 0.4 * (y[::2, ::2] - 128) + rng.integers(-3, 4, (SH // 2, SW // 2)), 128 - 0.3 * (y[::2, ::2] - 128)]
        frames.append(np.concatenate([p.round().clip(0, 255).astype(np.uint8).reshape(-1) for p in planes]))
    with y4m.Y4mWriter(f, SW, SH, (30, 1), "420mpeg2", aspect=(1, 1)) as w:
        for fr in frames:
            w.write(fr)
    r = _deploy(d / "y4m", "--y4m-in", f, "--y4m-out", g, "--interp", "cubic")
    rd = y4m.Y4mReader(g)
    buf, got = bytearray(rd.frame_bytes), []
    while rd.read_into(buf):
        got.append(np.frombuffer(bytes(buf), np.uint8))
    rd.close()
    assert len(got) == T and np.array_equal(got[0], frames[0]) and rd.colour_range == "limited"
    assert json.load(open(g + ".json"))["interp"] == "cubic"
    # the maps of the same loop in this process, then the planar model frame by frame
    cfg = Config(height=H, width=W)
    s = StabNetStream(synthetic.make_params(cfg, seed=0, theta_scale=0.2), H, W, cfg, streams=1, device=cuda, refine=1, use_graph=True,
                      operand_mode=4)
    ing = FrameIngest(SH, SW, 1, H, W, device=cuda, lut=lut256_limited())
    dev = torch.empty(SH * SW * 3 // 2, dtype=torch.uint8, device=cuda)
    y_view = dev[:SH * SW].view(SH, SW)
    dev.copy_(torch.from_numpy(frames[0]))
    s.start_u8(y_view, ing)
    for t in range(1, T):
        dev.copy_(torch.from_numpy(frames[t]))
        m = s.step_u8(y_view, ing)
        xm, ym = m["x_map"][0, :, :, 0].cpu().numpy(), m["y_map"][0, :, :, 0].cpu().numpy()
        want = CM.warp_i420(frames[t], xm, ym, SH, SW, 3, None, None, 16)[0]
        assert np.array_equal(got[t], want), t


def test_interp_linear_writes_what_no_flag_writes(cuda, data):
    d, clip, base = data
    _deploy(d / "lin", *base, "--output-size", "source", "--mjpg", "--interp", "linear")
    _deploy(d / "none", *base, "--output-size", "source", "--mjpg")
    names = sorted(os.listdir(d / "none" / "output"))
    assert sorted(os.listdir(d / "lin" / "output")) == names and "shaky_stable_bgr.npy" in names
    for name in names:
        assert open(d / "lin" / "output" / name, "rb").read() == open(d / "none" / "output" / name, "rb").read(), name
