"""GPU: the decoder's planes as they are (stabnet_mjpeg_decode_i420 / _sync_i420, mjpegd_planes_kernel of csrc/mjpeg_decode.hip)
against the NumPy model of tests/jpeg_planar_model.py, whose planes are Pillow's (tests/test_mjpeg_planar_cpu.py) -- bit for bit.
  streams   every fixture of tests/golden/mjpeg_planar_streams.npz through every back end that takes it: restart lanes for the streams
            with DRI; uploaded host coefficients, one lane, and the parallel back end for the others
  memory    a batch of three frames of different lengths, frames further apart than their size, the output at a base offset of 0, 3 and
            5 bytes (dword and byte stores), every buffer between canary bands, the bytes between the frames untouched
  graph     two replays of one hipGraph on changed input
  refusals  with device pointers: nothing is launched, the output stays as it was
Only valid streams go to the GPU."""
import io

import numpy as np
import pytest
import torch

import jpeg_decode_model as D
import jpeg_planar_model as P
from _guarded import Guarded

pytestmark = pytest.mark.gpu

GOLD = P.load_golden()


def _backends(jpeg):
    from stabnet_amd import mjpeg
    if mjpeg.parse(jpeg)["restart"]:
        return [dict()]                                                  # one lane per restart interval
    return [dict(), dict(host_entropy=False), dict(parallel=True), dict(parallel=True, chunk_bytes=8, sync_rounds=0)]


@pytest.mark.parametrize("name", list(GOLD))
def test_planes_equal_the_model_through_every_back_end(cuda, name):
    from stabnet_amd import mjpeg
    jpeg, _ = GOLD[name]
    ref = P.decode_i420(jpeg)
    info = mjpeg.parse(jpeg)
    for kw in _backends(jpeg):
        dec = mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda, planar=True, **kw)
        assert dec.planar and dec.frame_bytes == ref.size
        if not info["restart"]:
            assert (dec.host_entropy, dec.parallel) == (not kw, bool(kw.get("parallel")))
        dec.out.fill_(0xEE)
        got = dec.decode([jpeg])
        assert got.shape == (1, ref.size) and got.dtype == torch.uint8
        assert int(dec.status[0]) == 0
        assert np.array_equal(got[0].cpu().numpy(), ref), (name, kw)


def _picture(H, W, seed, noise=12.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 6.0 + y / 9.0), 128 + 90 * np.cos(x / 4.0 - y / 7.0), 30 + 3.0 * x + 2.0 * y], -1)
    return np.clip(np.rint(base + rng.normal(0.0, noise, base.shape)), 0, 255).astype(np.uint8)


def _pillow(img, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **opts)
    return buf.getvalue()


@pytest.mark.parametrize("offset", [0, 3, 5])
@pytest.mark.parametrize("mode", ["420", "grey"])
def test_batch_of_three_between_guards(cuda, mode, offset):
    """46x78: the Y rows (78 bytes) and the chroma rows (39 bytes) start at every alignment, so each store path runs in one call; the
    grey frame is 45x77.  Frames are 37 bytes further apart than their size."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.mjpeg import MjpegDecoder
    H, W, C = (46, 78, 3) if mode == "420" else (45, 77, 1)
    pics = [_picture(H, W, 10 + k, noise=4.0 + 20.0 * k) for k in range(3)]
    opts = dict(subsampling="4:2:0") if C == 3 else {}
    jpegs = [_pillow(p if C == 3 else p[..., 0].copy(), quality=60 + 15 * k, restart_marker_blocks=2 + k, **opts) for k, p in enumerate(pics)]
    assert len(set(len(j) for j in jpegs)) == 3
    dec = MjpegDecoder.for_stream(jpegs[0], device=cuda, batch=3, planar=True)
    for k, j in enumerate(jpegs):
        dec.stage(j, dec.h_in[k])
    fb, stride = dec.frame_bytes, dec.frame_bytes + 37
    g_in = Guarded(cuda, 3 * dec.in_stride, init=dec.h_in.numpy().reshape(-1), dtype=torch.uint8)
    g_out = Guarded(cuda, offset + 2 * stride + fb, dtype=torch.uint8)
    g_ws = Guarded(cuda, 3 * dec.layout["frame"], dtype=torch.uint8)
    g_st = Guarded(cuda, 3 * 4, dtype=torch.uint8)
    before = g_in.np()
    out = g_out.t[offset:]
    assert out.data_ptr() % 4 == offset % 4
    _lib.call("stabnet_mjpeg_decode_i420", ptr(g_in.t), dec.in_stride, 3, H, W, C, 420 if C == 3 else 0, 0, ptr(out), stride, ptr(g_st.t),
              ptr(g_ws.t), g_ws.n, stream_ptr(cuda), None, device=cuda)
    torch.cuda.synchronize()
    for what, g in (("in", g_in), ("out", g_out), ("workspace", g_ws), ("status", g_st)):
        g.check(what)
    assert np.array_equal(g_in.np(), before) and not g_st.np().any()
    got = g_out.np()
    assert (got[:offset] == 0xEE).all()
    for k, j in enumerate(jpegs):
        at = offset + k * stride
        assert np.array_equal(got[at:at + fb], P.decode_i420(j)), k
        if k < 2:
            assert (got[at + fb:at + stride] == 0xEE).all()            # the bytes between the frames are the caller's
    # a frame alone gives what it gave in the batch
    single = MjpegDecoder.for_stream(jpegs[1], device=cuda, planar=True)
    assert np.array_equal(single.decode([jpegs[1]])[0].cpu().numpy(), got[offset + stride:offset + stride + fb])


@pytest.mark.parametrize("parallel", [False, True])
def test_hipgraph_two_replays(cuda, parallel):
    from stabnet_amd.mjpeg import MjpegDecoder
    extra = {} if parallel else dict(restart_marker_blocks=3)
    jpegs = [_pillow(_picture(34, 50, 20 + k), quality=80, subsampling="4:2:0", **extra) for k in range(3)]
    dec = MjpegDecoder.for_stream(jpegs[0], device=cuda, planar=True, parallel=parallel)
    assert dec.parallel == parallel and not dec.host_entropy
    out = torch.zeros((1, dec.frame_bytes), dtype=torch.uint8, device=cuda)

    def upload(j):
        used = dec.stage(j, dec.h_in[0])
        dec.d_in[0, :used].copy_(dec.h_in[0, :used])
        torch.cuda.synchronize()

    upload(jpegs[0])
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        dec.enqueue(dec.d_in, 1, out, dec.status[:1])                   # warm-up outside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dec.enqueue(dec.d_in, 1, out, dec.status[:1])
    for j in jpegs[1:]:
        upload(j)
        out.zero_()
        dec.status.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        assert int(dec.status[0]) == 0
        assert np.array_equal(out[0].cpu().numpy(), P.decode_i420(j))


def test_refusals_with_device_pointers_launch_nothing(cuda):
    from stabnet_amd import _lib, mjpeg
    from stabnet_amd._tensor import ptr, stream_ptr
    jpeg, _ = GOLD["420_18x34_q75_r3"]
    dec = mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda, planar=True)
    used = dec.stage(jpeg, dec.h_in[0])
    dec.d_in[0, :used].copy_(dec.h_in[0, :used])
    out = torch.full((1, dec.frame_bytes), 0xEE, dtype=torch.uint8, device=cuda)
    L = _lib.lib()

    def call(H=18, W=34, C=3, sub=420, fs=dec.frame_bytes, o=out):
        with torch.cuda.device(cuda):
            return L.stabnet_mjpeg_decode_i420(ptr(dec.d_in), dec.in_stride, 1, H, W, C, sub, 0, ptr(o), fs, ptr(dec.status), ptr(dec.workspace),
                                               dec.workspace.numel(), stream_ptr(cuda), None)

    for kw, word in ((dict(H=17), b"odd side"), (dict(W=33), b"odd side"), (dict(sub=444), b"4:4:4"), (dict(fs=dec.frame_bytes - 1), b"frame_stride_bytes"),
                     (dict(o=None), b"null"), (dict(o=torch.zeros(dec.frame_bytes, dtype=torch.uint8)), b"not device memory")):
        assert call(**kw) == -1 and word in L.stabnet_last_error(), (kw, L.stabnet_last_error())
    torch.cuda.synchronize()
    assert bool((out == 0xEE).all())
    assert call() == 0                                                    # and the same call with nothing wrong decodes
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), P.decode_i420(jpeg))
    # the wrapper: a BGR-only stream is Unsupported before a decoder exists; stages belong to the BGR decoder
    with pytest.raises(mjpeg.Unsupported, match="odd"):
        mjpeg.MjpegDecoder.for_stream(D.load_golden()["420_45x77_q75_r3"][0], device=cuda, planar=True)
    with pytest.raises(mjpeg.Unsupported, match="4:4:4"):
        mjpeg.MjpegDecoder.for_stream(D.load_golden()["444_33x50_q75_r2"][0], device=cuda, planar=True)
    with pytest.raises(_lib.StabnetError, match="stages"):
        dec.enqueue(dec.d_in, 1, out, dec.status[:1], stages=2)
    # the BGR decoder of the same stream is untouched by all this
    assert np.array_equal(mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda).decode([jpeg])[0].cpu().numpy(), D.decode(jpeg))


@pytest.mark.parametrize("parallel", [False, True])
def test_profiler_kind_of_the_planes_launch(cuda, parallel):
    from stabnet_amd.deploy import Profiler
    from stabnet_amd.mjpeg import MjpegDecoder
    jpeg, _ = GOLD["420_46x78_q30_noisy"]
    dec = MjpegDecoder.for_stream(jpeg, device=cuda, planar=True, parallel=parallel)
    used = dec.stage(jpeg, dec.h_in[0])
    dec.d_in[0, :used].copy_(dec.h_in[0, :used])
    prof = Profiler(16)
    dec.enqueue(dec.d_in, 1, dec.out[:1], dec.status[:1], prof=prof)
    recs = prof.records()
    assert [r[0] for r in recs] == ["mjpegd_planes_kernel"]
    assert recs[0][3] == 2.0 * dec.frame_bytes
    assert np.array_equal(dec.out[0].cpu().numpy(), P.decode_i420(jpeg))
