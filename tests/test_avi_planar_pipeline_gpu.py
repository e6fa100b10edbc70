"""GPU: the Motion-JPEG stream loop of the driver (deploy_bundle.py --avi-in / --avi-out / --y4m-out), YCbCr end to end.  Six frames of the
shaky picture of test_mjpeg_decode_pipeline_gpu._frames at that file's sizes, written 4:2:0 with restart markers; a twin without
restart markers; a grey one; one with a planted cut.
  planes   --avi-in A --y4m-out F writes, byte for byte, the file that --y4m-in G --y4m-out F' writes, G being the Y4M (C420jpeg
           XCOLORRANGE=FULL, the AVI's rate) of the model's decode_i420 of the same frames: the Y4M loop is held to its own models, so this
           pins decode + ingest + warp of the new loop; the same with --fill 0.8 --interp cubic, and with --scene-cut (equal scene lists)
  streams  --avi-out: AviMjpegReader reads it -- six frames of the input's size at the input's rate, every header the encoder's, frame
           t's coefficients transform_planes of frame t of the Y4M output by the tie rule, Pillow decodes every frame
  back end the clip without restart markers: --entropy parallel writes the bytes of --entropy auto; the report names the back end
  refusals a 4:2:2 clip; a clip whose third frame is truncated: one sentence, a non-zero exit, no traceback, valid outputs of two frames
"""
import io
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import jpeg_model as M
import jpeg_planar_model as P
from test_mjpeg_decode_pipeline_gpu import H, W, _frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "deploy_bundle.py")
ENV = dict(os.environ, PYTHONPATH=ROOT)
NET = ["--height", str(H), "--width", str(W)]
T = 6
QUALITY = 90


def _jpegs(kind):
    from PIL import Image
    frames = _frames()[:T]
    if kind == "cut":                                              # frames 3.. show another picture
        frames = frames[:3] + [np.ascontiguousarray(255 - f[::-1, ::-1, ::-1]) // 2 for f in frames[3:]]
    opts = {"dri": dict(subsampling="4:2:0", restart_marker_blocks=2), "nodri": dict(subsampling="4:2:0"), "cut": dict(subsampling="4:2:0", restart_marker_blocks=2),
            "grey": dict(restart_marker_blocks=3), "422": dict(subsampling="4:2:2")}[kind]
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f[..., 1].copy() if kind == "grey" else f).save(buf, "JPEG", quality=85, **opts)
        out.append(buf.getvalue())
    return out


def _write_avi(path, jpegs):
    from stabnet_amd.avi import AviMjpegWriter
    with AviMjpegWriter(str(path), W, H, 25) as w:
        for j in jpegs:
            w.write(j)
    return str(path)


def _write_y4m(path, jpegs, chroma="420jpeg"):
    """G: the model's planes of the same frames as a full-range Y4M at the AVI's rate."""
    from stabnet_amd import y4m
    with y4m.Y4mWriter(str(path), W, H, (25, 1), chroma, colour_range="full") as w:
        for j in jpegs:
            w.write(P.decode_i420(j))
    return str(path)


def _read_y4m(path):
    from stabnet_amd import y4m
    rd = y4m.Y4mReader(str(path))
    buf, frames = bytearray(rd.frame_bytes), []
    while rd.read_into(buf):
        frames.append(np.frombuffer(bytes(buf), np.uint8))
    rd.close()
    return rd, frames


def _drive(*args):
    r = subprocess.run([sys.executable, DRIVER] + NET + [str(a) for a in args], env=ENV, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "Traceback" not in r.stderr, r.stderr[-3000:]
    return r


def _ok(*args):
    r = _drive(*args)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == ""                                          # every message goes to stderr
    return r


@pytest.fixture(scope="module")
def clips(cuda, tmp_path_factory):
    d = tmp_path_factory.mktemp("avi_planar")
    out = {"dir": d}
    for kind in ("dri", "nodri", "cut", "grey"):
        j = _jpegs(kind)
        out[kind] = (_write_avi(d / (kind + ".avi"), j), _write_y4m(d / (kind + ".y4m"), j, "mono" if kind == "grey" else "420jpeg"), j)
    return out


@pytest.fixture(scope="module")
def main_run(clips):
    """--avi-in dri.avi --y4m-out F --avi-out A (both outputs at once), run once and shared."""
    d = clips["dir"]
    f, a = d / "main.y4m", d / "main.avi"
    r = _ok("--avi-in", clips["dri"][0], "--y4m-out", f, "--avi-out", a, "--jpeg-quality", QUALITY)
    return f, a, r


def test_planes_are_the_y4m_loops_of_the_models_planes(clips, main_run):
    f, a, r = main_run
    g = clips["dri"][1]
    f2 = clips["dir"] / "main_ref.y4m"
    _ok("--y4m-in", g, "--y4m-out", f2)
    got, ref = open(f, "rb").read(), open(f2, "rb").read()
    assert got.split(b"\n", 1)[0] == b"YUV4MPEG2 W%d H%d F25:1 Ip C420jpeg XCOLORRANGE=FULL" % (W, H)
    assert got == ref
    rd, frames = _read_y4m(f)
    assert len(frames) == T and np.array_equal(frames[0], P.decode_i420(clips["dri"][2][0]))          # frame 0 as decoded
    assert any(not np.array_equal(frames[t], P.decode_i420(clips["dri"][2][t])) for t in range(1, T))   # the others are warped
    assert "entropy decoding: restart lanes" in r.stderr


def test_fill_and_cubic_follow_the_y4m_loop(clips, main_run):
    d = clips["dir"]
    f, f2 = d / "fill.y4m", d / "fill_ref.y4m"
    _ok("--avi-in", clips["dri"][0], "--y4m-out", f, "--fill", "0.8", "--interp", "cubic")
    _ok("--y4m-in", clips["dri"][1], "--y4m-out", f2, "--fill", "0.8", "--interp", "cubic")
    assert open(f, "rb").read() == open(f2, "rb").read()
    assert open(f, "rb").read() != open(main_run[0], "rb").read()      # and the flags change the frames
    rep = json.load(open(str(f) + ".json"))
    assert rep["interp"] == "cubic" and rep["window"] is not None and rep["decode_backend"] == "restart lanes" and rep["jpeg"] is None


def test_scene_cut_follows_the_y4m_loop(clips):
    d = clips["dir"]
    f, f2 = d / "cut_out.y4m", d / "cut_ref.y4m"
    _ok("--avi-in", clips["cut"][0], "--y4m-out", f, "--scene-cut", "--scene-gap", "1")
    _ok("--y4m-in", clips["cut"][1], "--y4m-out", f2, "--scene-cut", "--scene-gap", "1")
    assert open(f, "rb").read() == open(f2, "rb").read()
    a, b = json.load(open(str(f) + ".json")), json.load(open(str(f2) + ".json"))
    assert a["scene_cuts"] == b["scene_cuts"] == [3] and a["scene_threshold"] == b["scene_threshold"]


def _pil(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return im


def _check_streams(avi_path, y4m_frames, C, quality):
    from stabnet_amd import mjpeg
    from stabnet_amd.avi import AviMjpegReader
    rd = AviMjpegReader(str(avi_path))
    assert len(rd) == len(y4m_frames) and rd.size == (W, H) and (rd.rate, rd.scale) == (25, 1)
    ql, qc = M.quant_tables(quality)
    header = M.header(H, W, C, "420", mjpeg.default_restart_mcus(C, 420), ql, qc)
    for t, frame in enumerate(y4m_frames):
        s = rd.jpeg(t)
        d = M.decode(s)
        assert s[:d["header_bytes"]] == header, t
        coef, ratio = P.transform_planes(*P.split(frame, H, W, C), ql, qc)
        diff = d["coef"] - coef
        assert not ((diff != 0) & ~(M.near_tie(ratio) & (np.abs(diff) <= 1))).any(), t
        assert (diff != 0).mean() <= 0.03
        im = _pil(s)
        assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")


def test_avi_out_holds_the_encoders_streams_of_the_y4m_frames(clips, main_run):
    f, a, r = main_run
    _, frames = _read_y4m(f)
    _check_streams(a, frames, 3, QUALITY)
    rep = json.load(open(str(a) + ".json"))
    assert rep["frames"] == T and rep["decode_backend"] == "restart lanes" and rep["jpeg"] == {"quality": QUALITY, "restart_mcus": 2}
    assert rep["network_size"] == [H, W] and rep["colour_range"] == "full" and rep["border_y"] == 0 and rep["interp"] == "linear"
    assert not os.path.exists(str(f) + ".json")                    # one report, beside the .avi


def test_a_clip_without_restart_markers_through_both_back_ends(clips):
    d = clips["dir"]
    a1, a2 = d / "auto.avi", d / "par.avi"
    r1 = _ok("--avi-in", clips["nodri"][0], "--avi-out", a1, "--fps", "30")
    r2 = _ok("--avi-in", clips["nodri"][0], "--avi-out", a2, "--fps", "30", "--entropy", "parallel")
    assert open(a1, "rb").read() == open(a2, "rb").read()
    assert json.load(open(str(a1) + ".json"))["decode_backend"] == "host coefficients"
    assert json.load(open(str(a2) + ".json"))["decode_backend"] == "parallel"
    assert "entropy decoding: host coefficients" in r1.stderr and "entropy decoding: parallel" in r2.stderr
    from stabnet_amd.avi import AviMjpegReader
    rd = AviMjpegReader(str(a1))
    assert len(rd) == T and (rd.rate, rd.scale) == (30, 1)         # --fps overrides the input's rate
    assert M.psnr(P.decode_i420(rd.jpeg(0)), P.decode_i420(clips["nodri"][2][0])) > 30.0            # frame 0: the input's, re-encoded at q75


def test_a_grey_clip_runs(clips):
    d = clips["dir"]
    f, a, f2 = d / "grey_out.y4m", d / "grey_out.avi", d / "grey_ref.y4m"
    _ok("--avi-in", clips["grey"][0], "--y4m-out", f, "--avi-out", a)
    _ok("--y4m-in", clips["grey"][1], "--y4m-out", f2)
    got = open(f, "rb").read()
    assert got.split(b"\n", 1)[0] == b"YUV4MPEG2 W%d H%d F25:1 Ip Cmono XCOLORRANGE=FULL" % (W, H)
    assert got == open(f2, "rb").read()
    rd, frames = _read_y4m(f)
    assert len(frames) == T and frames[0].size == H * W
    _check_streams(a, frames, 1, 75)
    assert json.load(open(str(a) + ".json"))["input"]["sampling"] == "grey"


def test_a_422_clip_is_refused_with_its_sentence(clips):
    d = clips["dir"]
    path = _write_avi(d / "s422.avi", _jpegs("422"))
    r = _drive("--avi-in", path, "--avi-out", d / "s422_out.avi")
    assert r.returncode != 0 and r.stdout == ""
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("deploy_bundle.py: --avi-in: ") and "sampling 21 11 11" in last and "test-list route" in last
    assert not (d / "s422_out.avi").exists()


def test_a_truncated_third_frame_ends_the_run_with_valid_outputs(clips, main_run):
    d = clips["dir"]
    jpegs = list(clips["dri"][2])
    jpegs[2] = jpegs[2][:len(jpegs[2]) // 2]
    path = _write_avi(d / "trunc.avi", jpegs)
    f, a = d / "trunc_out.y4m", d / "trunc_out.avi"
    r = _drive("--avi-in", path, "--y4m-out", f, "--avi-out", a)
    assert r.returncode != 0 and r.stdout == ""
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("deploy_bundle.py: --avi-in: ") and "frame 2" in last
    rd, frames = _read_y4m(f)
    assert len(frames) == 2
    _check_streams(a, frames, 3, 75)
    # and they are the frames of the whole clip's run
    _, whole = _read_y4m(main_run[0])
    assert np.array_equal(frames[0], whole[0]) and np.array_equal(frames[1], whole[1])
    rep = json.load(open(str(a) + ".json"))
    assert rep["frames"] == 2 and "frame 2" in rep["stopped"]
