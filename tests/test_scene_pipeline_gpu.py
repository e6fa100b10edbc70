"""GPU: deploy_bundle.py --scene-cut end to end on the uint8 clip A ++ B at 64 x 96 (tests/scene_model.py; the cut is frame 10): the
serial loop, --pipeline, the Y4M loop, --fill history and --score.  What the driver writes from the cut on equals, frame for frame,
what it writes for the clip [B0] ++ B -- the new scene with its first frame doubled."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "deploy_bundle.py")
ENV = dict(os.environ, PYTHONPATH=ROOT)
H, W, TA, TB = 64, 96, 10, 6
NET = ["--height", str(H), "--width", str(W)]


def _clips():
    A, B = M.cut_clip(H, W, TA, TB)
    return M.to_u8(np.concatenate([A, B])), M.to_u8(np.concatenate([B[0:1], B]))


def _drive(*args, **kw):
    r = subprocess.run([sys.executable, DRIVER] + NET + list(args), env=ENV, capture_output=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r


def _data_dir(d, clips):
    """<d>/unstable/<name>.npy and a test list naming them."""
    os.makedirs(d / "unstable")
    for name, c in clips.items():
        np.save(d / "unstable" / (name + ".npy"), c)
    (d / "list").write_text("".join(name + "\n" for name in clips))
    return ["--prefix", str(d), "--test-list", str(d / "list")]


@pytest.fixture(scope="module")
def grey_runs(cuda, tmp_path_factory):
    """One serial run over ab = A ++ B and bb = [B0] ++ B with --scene-cut --score, one --pipeline run and one run without the flag
    over ab.  -> the three output directories and the processes."""
    d = tmp_path_factory.mktemp("scene")
    ab, bb = _clips()
    src = _data_dir(d, {"ab": ab, "bb": bb})
    (d / "list_ab").write_text("ab\n")
    only_ab = src[:2] + ["--test-list", str(d / "list_ab")]
    serial = _drive(*src, "--scene-cut", "--scene-gap", "8", "--score", "--output-dir", str(d / "serial"))
    piped = _drive(*only_ab, "--scene-cut", "--pipeline", "--output-dir", str(d / "piped"))
    plain = _drive(*only_ab, "--output-dir", str(d / "plain"))
    return d, serial, piped, plain


def test_serial_run_after_the_cut_equals_the_run_over_the_new_scene(grey_runs):
    d, serial, _, _ = grey_runs
    out = d / "serial" / "output"
    sc = json.load(open(out / "ab_scenes.json"))
    assert sc["cuts"] == [TA] and sc["threshold"] == 0.35 and sc["gap"] == 8 and len(sc["d"]) == TA + TB and sc["d"][0] == 0.0
    assert sc["d"][TA] >= 0.6 and max(sc["d"][:TA] + sc["d"][TA + 1:]) <= 0.25
    _, _, d_model = M.run(np.stack([(f.astype(np.float32) * np.float32(1.0 / 255) - np.float32(0.5)) for f in _clips()[0]]), 0.35, 8)
    assert sc["d"] == [float(v) for v in d_model]
    assert json.load(open(out / "bb_scenes.json"))["cuts"] == []
    assert b"scene cut at frame %d (d = %.2f)" % (TA, sc["d"][TA]) in serial.stdout and serial.stdout.count(b"scene cut at frame") == 1
    sa, sb = np.load(out / "ab_stable.npy"), np.load(out / "bb_stable.npy")
    assert sa.shape == (TA + TB - 1, H, W) and sb.shape == (TB, H, W)
    assert np.array_equal(sa[TA - 1:], sb)                                          # kept frame k is the clip's frame k + 1
    ma, mb = np.load(out / "ab_maps.npz"), np.load(out / "bb_maps.npz")
    for k in ("x_map", "y_map", "black"):
        assert np.array_equal(ma[k][TA - 1:].view(np.uint8), mb[k].view(np.uint8)), k
    score = json.load(open(out / "ab_score.json"))
    assert score["scene_cuts"] == 1 and score["frames"] == TA + TB - 1
    assert not os.path.exists(out / "bb_score.json")                                # too short to score, as without the flag


def test_pipeline_gives_the_same_bytes_and_json(grey_runs):
    d, _, piped, _ = grey_runs
    a, b = d / "serial" / "output", d / "piped" / "output"
    assert np.array_equal(np.load(a / "ab_stable.npy"), np.load(b / "ab_stable.npy"))
    ma, mb = np.load(a / "ab_maps.npz"), np.load(b / "ab_maps.npz")
    for k in ("x_map", "y_map", "black"):
        assert np.array_equal(ma[k].view(np.uint8), mb[k].view(np.uint8)), k
    assert json.load(open(a / "ab_scenes.json")) == json.load(open(b / "ab_scenes.json"))
    assert piped.stdout.count(b"scene cut at frame %d " % TA) == 1


def test_without_the_flag_nothing_differs(grey_runs):
    d, serial, _, plain = grey_runs
    a, p = d / "serial" / "output", d / "plain" / "output"
    # (ab_cut.npy depends on the clip's black-free rectangle, which the two runs need not share)
    names = sorted(n for n in os.listdir(p) if n != "ab_cut.npy")
    assert names == ["ab_maps.npz", "ab_stable.npy"]
    assert names == sorted(n for n in os.listdir(a) if n.startswith("ab_") and n not in ("ab_scenes.json", "ab_score.json", "ab_cut.npy"))
    for text in (plain.stdout, plain.stderr):
        assert b"scene cut" not in text and b"scene-cut" not in text and b"_scenes.json" not in text
    sa, sp = np.load(a / "ab_stable.npy"), np.load(p / "ab_stable.npy")
    assert np.array_equal(sa[:TA - 1], sp[:TA - 1])                                 # up to the cut the two runs are the same run
    assert all(not np.array_equal(sa[k], sp[k]) for k in range(TA - 1, TA + TB - 1))


def _y4m(path, clip):
    from stabnet_amd import y4m
    chroma = np.full(H * W // 2, 128, np.uint8)
    with y4m.Y4mWriter(path, W, H, (30, 1), "420mpeg2", aspect=(1, 1), colour_range="full") as w:
        for f in clip:
            w.write(np.concatenate([f.reshape(-1), chroma]))


def _y4m_frames(path):
    from stabnet_amd import y4m
    rd = y4m.Y4mReader(path)
    buf, frames = bytearray(rd.frame_bytes), []
    while rd.read_into(buf):
        frames.append(bytes(buf))
    rd.close()
    return frames


def test_y4m_loop(cuda, tmp_path):
    ab, bb = _clips()
    _y4m(str(tmp_path / "ab.y4m"), ab); _y4m(str(tmp_path / "bb.y4m"), bb)
    ra = _drive("--y4m-in", str(tmp_path / "ab.y4m"), "--y4m-out", str(tmp_path / "ab_out.y4m"), "--scene-cut")
    _drive("--y4m-in", str(tmp_path / "bb.y4m"), "--y4m-out", str(tmp_path / "bb_out.y4m"))
    rep = json.load(open(tmp_path / "ab_out.y4m.json"))
    assert rep["scene_cuts"] == [TA] and rep["scene_threshold"] == 0.35 and rep["frames"] == TA + TB
    assert ra.stdout == b"" and ra.stderr.count(b"scene cut at frame %d " % TA) == 1
    rb = json.load(open(tmp_path / "bb_out.y4m.json"))
    assert "scene_cuts" not in rb and "scene_threshold" not in rb
    fa, fb = _y4m_frames(str(tmp_path / "ab_out.y4m")), _y4m_frames(str(tmp_path / "bb_out.y4m"))
    assert len(fa) == TA + TB and len(fb) == TB + 1
    for j in range(TB):
        assert fa[TA + j] == fb[1 + j], j


def test_fill_history_starts_over_at_the_cut(cuda, tmp_path):
    ab, bb = _clips()
    colour = lambda c: np.stack([c, c, c], axis=-1)                                 # grey of equal channels is the channel: the CPU margins hold
    src = _data_dir(tmp_path, {"abc": colour(ab), "bbc": colour(bb)})
    _drive(*src, "--scene-cut", "--ingest", "device", "--fill", "history", "--output-dir", str(tmp_path / "o"))
    out = tmp_path / "o" / "output"
    sc = json.load(open(out / "abc_scenes.json"))
    assert sc["cuts"] == [TA] and sc["d"][TA] >= 0.6 and max(sc["d"][:TA] + sc["d"][TA + 1:]) <= 0.25
    assert json.load(open(out / "bbc_scenes.json"))["cuts"] == []
    fa, fb = np.load(out / "abc_fill.npy"), np.load(out / "bbc_fill.npy")
    assert fa.shape == (TA + TB - 1, H, W, 3) and fb.shape == (TB, H, W, 3)
    assert np.array_equal(fa[TA - 1:], fb)
    assert np.array_equal(np.load(out / "abc_stable_bgr.npy")[TA - 1:], np.load(out / "bbc_stable_bgr.npy"))
    hist = json.load(open(out / "abc_fill_history.json"))
    assert hist["frames"] == TA + TB - 1 and len(hist["per_frame"]["status"]) == TA + TB - 1       # the log goes on across the cut
    assert hist["per_frame"]["status"][TA - 1] == 0                                                 # no model across the cut
