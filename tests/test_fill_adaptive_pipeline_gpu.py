"""GPU: adaptive borderless output through the drivers (network 32x64, source 90x150 BGR, 6 frames).  ClipPipeline(window='adaptive')
hands out the bytes of a serial loop of step_u8 + AdaptiveFill.update + warp.warpRevBundle2_win + MjpegEncoder -- frames, JPEGs, the
per-frame windows and stats, the coverage counts -- at source size and at the network's size, eagerly and from its graphs;
deploy_bundle.py --fill adaptive writes the same files with and without --pipeline, and the windows in its JSON are the model's
(tests/fill_adaptive_model.py) run over the maps it saved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fill_adaptive_model as FM
import remap_win_model as WM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, SH, SW, T = 32, 64, 90, 150, 6
OPTS = dict(quality=80, subsampling="420", restart_mcus=2)
FILL = dict(r_min=0.6, up=0.01, margin_q=8)


def _clip(sh, sw, n, seed=11):
    """uint8 BGR [n, sh, sw, 3]: the synthetic shaky clip, tinted."""
    from stabnet_amd import synthetic
    g8 = ((synthetic.make_clip(sh, sw, n, seed=seed).astype(np.float32) + 0.5) * 255).clip(0, 255)
    return np.stack([g8 * 0.8 + 20, g8, g8 * 0.65 + 60], -1).clip(0, 255).astype(np.uint8)


def _setup(cuda):
    from stabnet_amd import synthetic
    from stabnet_amd.config import Config
    from stabnet_amd.deploy import StabNetStream
    from stabnet_amd.ingest import FrameIngest
    cfg = Config(height=H, width=W)
    params = synthetic.make_params(cfg, seed=3, theta_scale=0.2)
    stream = lambda **kw: StabNetStream(params, H, W, cfg, device=cuda, **kw)
    return stream, FrameIngest(SH, SW, 3, H, W, device=cuda)


def _serial(cuda, stream, ing, bgr, source):
    """The loop one frame at a time: [(network output, kept frame, its JPEG, window, stats)], the coverage counts.  Every window is the
    model's for the frame's maps and the previous ratio; every kept frame the model's through that window."""
    import torch
    from stabnet_amd import warp
    from stabnet_amd.mjpeg import MjpegEncoder
    kh, kw = (SH, SW) if source else (H, W)
    enc = MjpegEncoder(kh, kw, 3, device=cuda, **OPTS)
    af = warp.AdaptiveFill(1, kh, kw, device=cuda, **FILL)
    s = stream(use_graph=True)
    s.start_u8(torch.from_numpy(bgr[0:1]).to(cuda), ing)
    acc = torch.zeros((kh, kw), dtype=torch.int32, device=cuda)
    serial, state = [], 1.0
    for t in range(1, T):
        raw = torch.from_numpy(bgr[t:t + 1]).to(cuda)
        r = s.step_u8(raw, ing)
        out = ((r["output"][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8)
        frame = raw[0] if source else ing.colour(raw)[0]
        warped = warp.warpRevBundle2_win(frame, r["x_map"], r["y_map"], af.update(r["x_map"], r["y_map"]), black_count=acc)
        window, stats = af.window[0].cpu().numpy(), af.stats[0].cpu().numpy()
        xm, ym = r["x_map"][0, :, :, 0].cpu().numpy(), r["y_map"][0, :, :, 0].cpu().numpy()
        state, mwin, key, cnt = FM.frame(xm, ym, kh, kw, state, **FILL)
        assert tuple(window) == mwin and tuple(stats) == (key, cnt) and float(af.state[0]) == state, t
        assert np.array_equal(warped.cpu().numpy(), WM.warp_win(frame.cpu().numpy(), xm, ym, mwin)[0]), t
        serial.append((out, warped.cpu().numpy(), enc.encode_bytes(warped)[0], window, stats))
    return serial, acc.cpu().numpy()


@pytest.mark.parametrize("output", ["source", "network"])
def test_adaptive_pipeline_equals_the_serial_loop(cuda, output):
    from stabnet_amd.deploy import ClipPipeline
    stream, ing = _setup(cuda)
    bgr = _clip(SH, SW, T)
    source = output == "source"
    kh, kw = (SH, SW) if source else (H, W)
    serial, acc = _serial(cuda, stream, ing, bgr, source)
    pipe = ClipPipeline(stream(use_graph=True), colour=True, jpeg=OPTS, ingest=ing, output=output, window="adaptive", fill=FILL)
    assert pipe.adaptive and pipe.window is None and pipe.all_black_win.shape == (kh, kw) and pipe.fill == (0.6, 0.01, 8)
    for rnd in range(2):                                                   # first use of every slot runs eagerly, then its graph replays
        got = pipe.run(bgr)
        assert [r["t"] for r in got] == list(range(1, T))
        for r, (out, col, jpg, window, stats) in zip(got, serial):
            assert np.array_equal(r["output"], out), (rnd, r["t"])
            assert r["bgr"].shape == (kh, kw, 3) and np.array_equal(r["bgr"], col), (rnd, r["t"])
            assert bytes(r["jpeg"]) == jpg, (rnd, r["t"])
            assert r["window"].dtype == np.float64 and np.array_equal(r["window"], window), (rnd, r["t"], r["window"], window)
            assert r["fill_stats"].dtype == np.int32 and np.array_equal(r["fill_stats"], stats), (rnd, r["t"])
        assert np.array_equal(pipe.all_black_win.cpu().numpy(), acc), rnd   # zeroed by run, counted inside the graphs
    assert len(pipe._graphs) == pipe.slots and all(g is not None for g in pipe._graphs.values())
    pipe.use_graph, pipe._graphs = False, {}                               # and every frame eagerly
    for r, (out, col, jpg, window, stats) in zip(pipe.run(bgr), serial):
        assert np.array_equal(r["bgr"], col) and bytes(r["jpeg"]) == jpg and np.array_equal(r["window"], window), r["t"]
    print("ratios:", [float(w[3]) / kw for _, _, _, w, _ in serial], "stats:", [tuple(int(v) for v in st) for _, _, _, _, st in serial])


def test_refusals(cuda):
    from stabnet_amd import _lib
    from stabnet_amd.deploy import ClipPipeline
    stream, ing = _setup(cuda)
    st = stream()
    with pytest.raises(_lib.StabnetError, match="window"):
        ClipPipeline(st, colour=False, window="adaptive")                                       # keeps the network's grey output
    for bad in (dict(r_min=0), dict(r_min=1.5), dict(up=-1), dict(up=float("nan")), dict(margin_q=-1), dict(margin_q=16 * SH + 1),
                dict(ratio=0.5)):
        with pytest.raises(_lib.StabnetError):
            ClipPipeline(st, colour=True, ingest=ing, output="source", window="adaptive", fill=bad)
    with pytest.raises(_lib.StabnetError, match="fill"):
        ClipPipeline(st, colour=True, ingest=ing, output="source", window=(0, 0, SH, SW), fill=FILL)
    with pytest.raises(_lib.StabnetError, match="fill"):
        ClipPipeline(st, colour=True, ingest=ing, output="source", fill=FILL)
    assert ClipPipeline(st, colour=True, ingest=ing, output="source", window="adaptive").fill == (0.5, 0.002, 8)


def _deploy(out_dir, *extra, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(H), "--width", str(W), "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def test_deploy_bundle_fill_adaptive_serial_and_pipelined(cuda, tmp_path):
    n = 6
    clip = _clip(SH, SW, n, seed=4)
    prefix = tmp_path / "data"
    os.makedirs(prefix / "unstable")
    np.save(str(prefix / "unstable" / "shaky.npy"), clip)
    (tmp_path / "list").write_text("shaky.npy\n")
    base = ["--test-list", str(tmp_path / "list"), "--prefix", str(prefix), "--mjpg", "--ingest", "device", "--output-size", "source",
            "--fill", "adaptive", "--fill-min", "0.6", "--fill-up", "0.01"]
    f = lambda d, name: str(tmp_path / d / "output" / name)
    out = _deploy(tmp_path / "ser", *base)
    assert "--fill adaptive" in out and "left some pixel uncovered" in out and "WARNING" not in out
    info = json.load(open(f("ser", "shaky_fill_window.json")))
    assert info["mode"] == "adaptive" and info["params"] == dict(r_min=0.6, up=0.01, margin_q=8) and info["output_size"] == [SH, SW]
    colour, maps = np.load(f("ser", "shaky_stable_bgr.npy")), np.load(f("ser", "shaky_maps.npz"))
    assert colour.shape == (n - 1, SH, SW, 3) and len(info["windows"]) == n - 1
    # the JSON's windows are the model's over the saved maps; every kept frame is the model's through its window
    state, per, held = 1.0, [], 0
    for i in range(n - 1):
        xm, ym = maps["x_map"][i], maps["y_map"][i]
        state, window, key, cnt = FM.frame(xm, ym, SH, SW, state, r_min=0.6, up=0.01, margin_q=8)
        r_safe = FM.r_safe_of(key, H // 4, W // 4)
        assert tuple(info["windows"][i]) == window and info["r_safe"][i] == r_safe and info["bad_nodes"][i] == cnt, i
        want, _, _, blk = WM.warp_win(clip[i + 1], xm, ym, window)
        assert np.array_equal(colour[i], want), i
        per.append(int(blk.sum()))
        held += r_safe < 0.6
        assert r_safe < 0.6 or per[-1] == 0, i                               # the promise: no uncovered pixel unless held at r_min
    assert info["uncovered"]["per_frame"] == per and info["held_at_min"] == held
    names = ["shaky_stable.npy", "shaky_stable_bgr.npy", "shaky_maps.npz", "shaky.avi", "shaky_fill_window.json"]
    names += [x for x in ("shaky_cut.npy", "shaky_cut.avi") if os.path.exists(f("ser", x))]
    _deploy(tmp_path / "pipe", *base, "--pipeline")
    assert sorted(os.listdir(tmp_path / "pipe" / "output")) == sorted(os.listdir(tmp_path / "ser" / "output"))
    for name in names:
        assert open(f("pipe", name), "rb").read() == open(f("ser", name), "rb").read(), name
