"""GPU: the Y4M loop of the driver (deploy_bundle.py --y4m-in / --y4m-out) end to end on a generated 7-frame 96x160 C420mpeg2 stream at
network size 64x96 with the seeded synthetic weights: file to file against a recomputation in this process, stdin to stdout byte for
byte the same, --fill, a mono stream, a refused stream, and the driver without the new flags against the loop it always ran."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "deploy_bundle.py")
ENV = dict(os.environ, PYTHONPATH=ROOT)
T, SH, SW, NH, NW = 7, 96, 160, 64, 96
NET = ["--height", str(NH), "--width", str(NW)]


def _clip(chroma, seed=3):
    """T frames: a smooth random picture in the limited range that drifts and shakes, chroma planes of its own."""
    rng = np.random.default_rng(seed)
    big = rng.integers(16, 236, (SH // 8 + 4, SW // 8 + 4)).astype(np.float64)
    big = np.kron(big, np.ones((8, 8)))
    frames = []
    for t in range(T):
        dy, dx = 12 + int(rng.integers(-6, 7)), 12 + int(rng.integers(-6, 7)) + t
        y = big[dy:dy + SH, dx:dx + SW]
        planes = [y]
        if chroma != "mono":
            planes += [128 + 0.4 * (y[::2, ::2] - 128), 128 - 0.3 * (y[::2, ::2] - 128)]
        frames.append(np.concatenate([p.round().astype(np.uint8).reshape(-1) for p in planes]))
    return frames


def _write(path, chroma, header_chroma=None):
    from stabnet_amd import y4m
    frames = _clip(chroma)
    with y4m.Y4mWriter(path, SW, SH, (30000, 1001), chroma, aspect=(1, 1)) as w:
        for f in frames:
            w.write(f)
    if header_chroma is not None:                                  # a tag the writer refuses, for the refusal test
        data = open(path, "rb").read().replace(b" C" + chroma.encode(), b" C" + header_chroma.encode(), 1)
        open(path, "wb").write(data)
    return frames


def _read(path_or_bytes):
    from stabnet_amd import y4m
    rd = y4m.Y4mReader(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else path_or_bytes)
    buf, frames = bytearray(rd.frame_bytes), []
    while rd.read_into(buf):
        frames.append(np.frombuffer(bytes(buf), np.uint8))
    rd.close()
    return rd, frames


def _drive(*args, **kw):
    return subprocess.run([sys.executable, DRIVER] + NET + list(args), env=ENV, capture_output=True, timeout=600, **kw)


@pytest.fixture(scope="module")
def file_run(cuda, tmp_path_factory):
    """--y4m-in f --y4m-out g, run once and shared: (f, g, the input's frames, the finished process)."""
    d = tmp_path_factory.mktemp("y4m")
    f, g = str(d / "in.y4m"), str(d / "out.y4m")
    frames = _write(f, "420mpeg2")
    r = _drive("--y4m-in", f, "--y4m-out", g)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return f, g, frames, r


def test_file_to_file_equals_a_recomputation(cuda, file_run):
    import torch
    from stabnet_amd import synthetic, warp
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    from stabnet_amd.ingest import FrameIngest, lut256_limited
    f, g, frames, r = file_run
    rd, got = _read(g)
    assert (rd.width, rd.height, rd.fps, rd.aspect, rd.chroma, rd.colour_range) == (SW, SH, (30000, 1001), (1, 1), "420mpeg2", "limited")
    assert len(got) == T and np.array_equal(got[0], frames[0])
    assert r.stdout == b"" and b"fps=" in r.stderr and b"total length=" in r.stderr
    # the recomputation: the stream, the ingest with the limited-range table on the Y plane's view, the planar warp
    cfg = Config(height=NH, width=NW)
    s = StabNetStream(synthetic.make_params(cfg, seed=0, theta_scale=0.2), NH, NW, cfg, streams=1, device=cuda, refine=1, use_graph=True,
                      operand_mode=4)
    black = torch.zeros((SH, SW), dtype=torch.int32, device=cuda)
    ing = FrameIngest(SH, SW, 1, NH, NW, device=cuda, lut=lut256_limited())
    dev = torch.empty(SH * SW * 3 // 2, dtype=torch.uint8, device=cuda)
    y_view = dev[:SH * SW].view(SH, SW)
    dev.copy_(torch.from_numpy(frames[0]))
    s.start_u8(y_view, ing)
    for t in range(1, T):
        dev.copy_(torch.from_numpy(frames[t]))
        m = s.step_u8(y_view, ing)
        want = warp.warpRevBundle2_i420(dev, m["x_map"], m["y_map"], (SH, SW), 3, border_y=16, black_count=black).cpu().numpy()
        assert np.array_equal(got[t], want), t
        assert not np.array_equal(got[t], frames[t])
    rep = json.load(open(g + ".json"))
    assert rep["input"] == {"width": SW, "height": SH, "fps": [30000, 1001], "aspect": [1, 1], "chroma": "420mpeg2", "colour_range": "limited",
                            "frame_bytes": SH * SW * 3 // 2}
    assert rep["network_size"] == [NH, NW] and rep["colour_range"] == "limited" and rep["border_y"] == 16 and rep["window"] is None
    assert rep["frames"] == T
    assert rep["pixels_ever_uncovered"] == int((black > 0).sum()) and rep["max_uncovered_count"] == int(black.max())


def test_stdin_to_stdout_gives_the_same_bytes(cuda, file_run):
    f, g, frames, _ = file_run
    with open(f, "rb") as fin:
        r = _drive("--y4m-in", "-", "--y4m-out", "-", stdin=fin)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == open(g, "rb").read()                       # the video and nothing else
    assert b"note: --y4m-in" in r.stderr and b"fps=" in r.stderr and b"inference with" in r.stderr
    assert not os.path.exists("-.json")


def test_fill_changes_the_frames_and_keeps_the_header(cuda, file_run, tmp_path):
    f, g, frames, _ = file_run
    h = str(tmp_path / "fill.y4m")
    r = _drive("--y4m-in", f, "--y4m-out", h, "--fill", "0.8")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    (rg, fg), (rh, fh) = _read(g), _read(h)
    assert rh.header_fields() == rg.header_fields() and len(fh) == T
    assert np.array_equal(fh[0], frames[0])
    assert all(not np.array_equal(a, b) for a, b in zip(fg[1:], fh[1:]))
    rep = json.load(open(h + ".json"))
    from stabnet_amd.warp import ratio_window
    assert rep["window"] == list(ratio_window(SH, SW, 0.8)) and rep["frames"] == T


def test_a_mono_stream_runs_and_writes_mono(cuda, tmp_path):
    f, g = str(tmp_path / "m.y4m"), str(tmp_path / "m_out.y4m")
    frames = _write(f, "mono")
    r = _drive("--y4m-in", f, "--y4m-out", g)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    rd, got = _read(g)
    assert rd.chroma == "mono" and rd.colour_range == "full" and rd.frame_bytes == SH * SW and len(got) == T
    assert np.array_equal(got[0], frames[0]) and not np.array_equal(got[1], frames[1])
    assert json.load(open(g + ".json"))["border_y"] == 0


def test_a_422_stream_is_refused_with_its_sentence(tmp_path):
    f = str(tmp_path / "c422.y4m")
    _write(f, "420mpeg2", header_chroma="422")
    r = _drive("--y4m-in", f, "--y4m-out", str(tmp_path / "o.y4m"))
    err = r.stderr.decode()
    assert r.returncode != 0 and "chroma 'C422' is not supported" in err and "Traceback" not in err
    assert r.stdout == b"" and not os.path.exists(tmp_path / "o.y4m")


def test_the_driver_without_the_new_flags_writes_what_its_loop_always_wrote(cuda, tmp_path):
    """deploy_bundle.py --synthetic 5 against the serial loop stated here as it stood before the Y4M mode: start(), step() per frame, the
    network's grey output on the 0..255 scale."""
    import torch
    import deploy_bundle
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    r = _drive("--synthetic", "5", "--output-dir", str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"fps=" not in r.stderr and b"total length=" in r.stdout                       # the messages stay on stdout
    got = np.load(tmp_path / "output" / "synthetic_stable.npy")
    cfg = Config(height=NH, width=NW)
    s = StabNetStream(synthetic.make_params(cfg, seed=0, theta_scale=0.2), NH, NW, cfg, streams=1, device=cuda, refine=1, use_graph=True,
                      operand_mode=4)
    s.track_black()
    clip = (synthetic.make_clip(NH, NW, 5, seed=1234) + 0.5) * 255.0
    s.start(torch.from_numpy(deploy_bundle.grey_train(clip[0], NH, NW)[None]).to(cuda))
    want = []
    for t in range(1, len(clip)):
        m = s.step(torch.from_numpy(deploy_bundle.grey_train(clip[t], NH, NW)[None]).to(cuda))
        want.append(((m["output"][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8))
    assert np.array_equal(got, np.stack(want))
