"""GPU: the frame ingest through the drivers (network 64x96, source 160x240 BGR, 5 frames).  StabNetStream.start_u8 / step_u8 give
the bits of start / step fed with the Pillow-chain float frames, with and without a frame graph; ClipPipeline(ingest=...) hands
out the bytes of the serial loop, the JPEG included; deploy_bundle.py --ingest device keeps the colour outputs of a clip that is
not at the network's size and writes the cv2-resized first frame to the .avi."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import ingest_model as M
import riff_walk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, SH, SW, T = 64, 96, 160, 240, 5


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


KEYS = ("output", "black_pix", "Hs", "x_map", "y_map", "theta", "frame")


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_u8_equals_step_on_the_pillow_chain(cuda, use_graph):
    import torch
    stream, ing = _setup(cuda)
    bgr = _clip(SH, SW, T)
    floats = [M.train_from_u8(M.real_pil_resize(M.grey_u8(f), H, W)) for f in bgr]
    a, b = stream(use_graph=use_graph), stream(use_graph=use_graph)
    a.start(torch.from_numpy(floats[0][None]).to(cuda))
    b.start_u8(torch.from_numpy(bgr[0:1]).to(cuda), ing)
    assert torch.equal(a.frames_ring, b.frames_ring)
    for t in range(1, T):
        ra = {k: v.clone() for k, v in a.step(torch.from_numpy(floats[t][None]).to(cuda)).items()}
        rb = b.step_u8(torch.from_numpy(bgr[t:t + 1]).to(cuda), ing)
        torch.cuda.synchronize()
        assert np.array_equal(b.cur.cpu().numpy()[0].view(np.int32), floats[t].view(np.int32)), t
        for k in KEYS:
            assert torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32)), (t, k)
    assert (b._graph_u8 is not None) == (use_graph and b.use_graph)
    from stabnet_amd import _lib
    with pytest.raises(_lib.StabnetError):
        b.step_u8(torch.from_numpy(bgr[1:2]), ing)                       # a CPU tensor
    with pytest.raises(_lib.StabnetError):
        b.step_u8(torch.from_numpy(bgr[1:2, :-1]).to(cuda), ing)          # not the ingest's source size
    with pytest.raises(_lib.StabnetError):
        stream().step_u8(torch.from_numpy(bgr[1:2]).to(cuda), ing)        # before start_u8


def test_pipeline_with_ingest_equals_the_serial_loop(cuda):
    import torch
    from stabnet_amd import _lib, warp
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
        col = ing.colour(raw)
        assert np.array_equal(col.cpu().numpy()[0], M.cv_resize(bgr[t], H, W))
        out = ((r["output"][0, :, :, 0].cpu().numpy() + 0.5) * 255).clip(0, 255).astype(np.uint8)
        warped = warp.warpRevBundle2(col[0], r["x_map"], r["y_map"])
        serial.append((out, warped.cpu().numpy(), enc.encode_bytes(warped)[0]))
    pipe = ClipPipeline(stream(use_graph=True), colour=True, jpeg=opts, ingest=ing)
    assert not hasattr(pipe, "h_grey") and not hasattr(pipe, "h_bgr")      # ONE upload per frame: the raw uint8 frame
    assert pipe.h_u8[0].shape == (SH, SW, 3)
    for rnd in range(2):                                                   # first use of every slot runs eagerly, then its graph replays
        got = pipe.run(bgr)
        assert [r["t"] for r in got] == list(range(1, T))
        for r, (out, col, jpg) in zip(got, serial):
            assert np.array_equal(r["output"], out), (rnd, r["t"])
            assert np.array_equal(r["bgr"], col), (rnd, r["t"])
            assert bytes(r["jpeg"]) == jpg, (rnd, r["t"])
    assert len(set(j for _, _, j in serial)) == T - 1
    # grey-only pipeline of the same clip: no colour frame is made or asked for
    grey = ClipPipeline(stream(use_graph=True), colour=False, ingest=ing).run(bgr)
    assert all(np.array_equal(r["output"], o) and "bgr" not in r for r, (o, _, _) in zip(grey, serial))
    from stabnet_amd.ingest import FrameIngest
    with pytest.raises(_lib.StabnetError):
        ClipPipeline(stream(), colour=True, ingest=FrameIngest(SH, SW, 1, H, W, device=cuda))
    with pytest.raises(_lib.StabnetError):
        ClipPipeline(stream(), colour=False, ingest=FrameIngest(SH, SW, 3, H + 8, W, device=cuda))


def _deploy(out_dir, *extra, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--height", str(H), "--width", str(W), "--output-dir", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def test_deploy_bundle_ingest_device_keeps_colour_and_writes_the_resized_first_frame(cuda, tmp_path):
    import torch
    from PIL import Image
    from stabnet_amd.mjpeg import MjpegEncoder
    n = 5
    clip = _clip(90, 150, n, seed=4)
    prefix = tmp_path / "data"
    os.makedirs(prefix / "unstable")
    np.save(str(prefix / "unstable" / "shaky.npy"), clip)
    (tmp_path / "list").write_text("shaky.npy\n")
    base = ["--test-list", str(tmp_path / "list"), "--prefix", str(prefix), "--mjpg"]
    f = lambda d, name: str(tmp_path / d / "output" / name)
    host = _deploy(tmp_path / "host", *base)
    assert "--ingest device" not in host
    assert os.path.exists(f("host", "shaky_stable.npy")) and not os.path.exists(f("host", "shaky_stable_bgr.npy"))
    out = _deploy(tmp_path / "dev", *base, "--ingest", "device")
    assert "on the GPU as the reference's cv2/PIL chain" in out
    stable = np.load(f("dev", "shaky_stable.npy"))
    colour = np.load(f("dev", "shaky_stable_bgr.npy"))
    assert stable.shape == (n - 1, H, W) and colour.shape == (n - 1, H, W, 3) and colour.dtype == np.uint8
    assert np.load(f("host", "shaky_stable.npy")).shape == stable.shape
    t = riff_walk.walk(f("dev", "shaky.avi"))
    assert len(t["frames"]) == n and (t["strf"]["width"], t["strf"]["height"]) == (W, H)
    want = M.cv_resize(clip[0], H, W)
    dec = lambda data: np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1].astype(np.int32)
    enc = MjpegEncoder(H, W, 3, device=cuda)                              # the driver's defaults: q75, 4:2:0
    own = np.abs(dec(enc.encode_bytes(torch.from_numpy(want).to(cuda))[0]) - want).max()
    got = np.abs(dec(riff_walk.jpeg_of(t, 0)) - want).max()
    print("first frame of the .avi: %d grey levels from the cv-resized frame; the encoder's own error on that frame %d" % (got, own))
    assert got <= own
    # frames 1.. are the stabilised colour frames
    for i in range(1, n):
        assert riff_walk.jpeg_of(t, i) == enc.encode_bytes(torch.from_numpy(colour[i - 1]).to(cuda))[0], i
    # the pipelined loop writes the same files
    _deploy(tmp_path / "pipe", *base, "--ingest", "device", "--pipeline")
    for name in ("shaky_stable.npy", "shaky_stable_bgr.npy", "shaky.avi"):
        assert open(f("pipe", name), "rb").read() == open(f("dev", name), "rb").read(), name
