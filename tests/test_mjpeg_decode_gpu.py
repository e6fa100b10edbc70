"""GPU: the JPEG decoder of csrc/mjpeg_decode.hip, stage by stage and whole, against the host back end, the NumPy model of
tests/jpeg_decode_model.py and the golden pixels (Pillow on libjpeg-turbo) of tests/golden/mjpeg_decode_streams.npz -- bit for bit.
  entropy   the kernel's coefficients equal stabnet_mjpeg_entropy_host's for restart intervals of 1 MCU, one MCU row, a value that
            does not divide the MCU count and one above it; 11-bit DC / 10-bit AC categories with ZRL runs; custom Huffman tables
  idct      the planes equal the model's
  frames    every fixture equals its golden pixels (4:2:0, 4:4:4, grey; odd sizes; below one MCU); streams without DRI through the
            host-entropy upload path; a batch of three frames of different lengths between canary bands, at an aligned and an
            unaligned row stride; two replays of one hipGraph; the project's own encoder round trip; status 0 everywhere
Only valid streams go to the GPU (corrupt ones: tests/test_mjpeg_decode_cpu.py, the same bounded routine)."""
import io

import numpy as np
import pytest
import torch

import jpeg_decode_model as D
from _guarded import Guarded

pytestmark = pytest.mark.gpu

GOLD = D.load_golden()
NAMES = list(GOLD)


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


def _extreme():
    """q100 (every quantiser 1) on hard edges and noise: DC differences of category 11, AC values of category 10, ZRL runs."""
    rng = np.random.default_rng(7)
    img = np.zeros((32, 48), np.uint8)
    img[:, 8:16] = 255                                  # black block next to a white one: DC -1024 -> +1016
    img[8:16, 24:28] = 255                              # half a block white: a first-row AC value near 900
    img[16:24, 32:48] = rng.integers(0, 256, (8, 16))   # noise
    yy, xx = np.mgrid[0:8, 0:8]
    img[24:32, 0:8] = 100 + (-1) ** (xx + yy)            # a +-1 checkerboard: only the highest frequencies survive, long zero runs
    return _pillow(img, quality=100, restart_marker_blocks=5)


def _coef_device(cuda, jpeg):
    from stabnet_amd.mjpeg import MjpegDecoder
    dec = MjpegDecoder.for_stream(jpeg, device=cuda, host_entropy=False)
    used = dec.stage(jpeg, dec.h_in[0])
    dec.d_in[0, :used].copy_(dec.h_in[0, :used])
    dec.workspace.fill_(0x5A)
    dec.enqueue(dec.d_in, 1, None, dec.status[:1], stages=1)
    torch.cuda.synchronize()
    assert int(dec.status[0]) == 0
    lay = dec.layout
    return dec.workspace[lay["coef"]:lay["coef"] + 2 * dec.coef_count].cpu().numpy().view(np.int16)


def _coef_host(jpeg):
    import ctypes
    from stabnet_amd import _lib, mjpeg
    i = mjpeg.parse(jpeg)
    blob = np.zeros(i["blob_bytes"], np.uint8)
    mjpeg.parse(jpeg, blob.ctypes.data, blob.size)
    coef = np.zeros(i["blocks"] * 64, np.int16)
    assert _lib.lib().stabnet_mjpeg_entropy_host(jpeg, len(jpeg), blob.ctypes.data, blob.size, coef.ctypes.data, coef.size) == 0
    return coef


ENTROPY_CASES = {
    # 40x56 4:2:0: 3 x 4 = 12 MCUs
    "r1": lambda: _pillow(_picture(40, 56, 1), quality=85, subsampling="4:2:0", restart_marker_blocks=1),
    "r_row": lambda: _pillow(_picture(40, 56, 2), quality=85, subsampling="4:2:0", restart_marker_blocks=4),
    "r_nodiv": lambda: _pillow(_picture(40, 56, 3), quality=85, subsampling="4:2:0", restart_marker_blocks=5),
    "r_above": lambda: _pillow(_picture(40, 56, 4), quality=85, subsampling="4:2:0", restart_marker_blocks=20),
    "444_r3": lambda: _pillow(_picture(33, 50, 5), quality=90, subsampling="4:4:4", restart_marker_blocks=3),
    "extreme": _extreme,
    "custom_tables": lambda: _pillow(_picture(40, 56, 6, noise=30.0), quality=92, subsampling="4:2:0", optimize=True, restart_marker_blocks=2),
}


@pytest.mark.parametrize("case", list(ENTROPY_CASES))
def test_entropy_kernel_equals_host(cuda, case):
    jpeg = ENTROPY_CASES[case]()
    host = _coef_host(jpeg)
    ref = D.coefficients(jpeg)
    assert np.array_equal(host.astype(np.int32), ref["coef"].reshape(-1))
    if case == "extreme":
        zz = np.zeros_like(ref["coef"])
        zz[...] = ref["coef"][..., D.NAT_OF_ZZ]                       # back to scan order
        blocks = zz.reshape(-1, 64)
        assert np.abs(np.diff(blocks[:, 0])).max() >= 1024             # category 11
        assert np.abs(blocks[:, 1:]).max() >= 512                      # category 10
        runs = [np.diff(np.flatnonzero(np.r_[1, b[1:]])).max(initial=0) for b in blocks]
        assert max(runs) > 16                                          # a ZRL in front of a coefficient
    if case == "custom_tables":
        assert D.annexk_dht()[4:33] not in jpeg
    if case == "r_above":
        from stabnet_amd import mjpeg
        assert mjpeg.parse(jpeg)["intervals"] == 1 and mjpeg.parse(jpeg)["restart"] == 20
    got = _coef_device(cuda, jpeg)
    assert np.array_equal(got, host)


@pytest.mark.parametrize("name", ["420_45x77_q75_r3", "444_33x50_q75_r2", "grey_45x77_q75_r4", "420_17x31_q100_verynoisy"])
def test_idct_planes_equal_model(cuda, name):
    from stabnet_amd.mjpeg import MjpegDecoder
    jpeg, _ = GOLD[name]
    dec = MjpegDecoder.for_stream(jpeg, device=cuda)
    used = dec.stage(jpeg, dec.h_in[0])
    dec.d_in[0, :used].copy_(dec.h_in[0, :used])
    dec.enqueue(dec.d_in, 1, None, dec.status[:1], stages=2)
    torch.cuda.synchronize()
    assert int(dec.status[0]) == 0
    lay, ws = dec.layout, dec.workspace.cpu().numpy()
    ref = D.planes(D.coefficients(jpeg))
    y = ws[lay["y"]:lay["y"] + lay["yh"] * lay["yw"]].reshape(lay["yh"], lay["yw"])
    assert np.array_equal(y, ref[0])
    if len(ref) == 3:
        for off, r in ((lay["cb"], ref[1]), (lay["cr"], ref[2])):
            assert np.array_equal(ws[off:off + lay["ch"] * lay["cw"]].reshape(lay["ch"], lay["cw"]), r)


@pytest.mark.parametrize("name", NAMES)
def test_full_decode_equals_golden(cuda, name):
    from stabnet_amd import mjpeg
    jpeg, px = GOLD[name]
    dec = mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda)
    assert dec.host_entropy == (mjpeg.parse(jpeg)["restart"] == 0)       # streams without DRI: coefficients from the host
    got = dec.decode([jpeg])
    assert int(dec.status[0]) == 0
    assert np.array_equal(got[0].cpu().numpy(), px)
    if dec.host_entropy:                                                 # and the same pixels with the one interval decoded by one lane
        dev = mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda, host_entropy=False)
        assert np.array_equal(dev.decode([jpeg])[0].cpu().numpy(), px) and int(dev.status[0]) == 0


@pytest.mark.parametrize("pad", [0, 3, 5])
def test_batch_of_three_between_guards(cuda, pad):
    """Three frames of one geometry and different byte lengths in one call; every buffer between canary bands; rows `pad` bytes apart
    from the natural stride (77 x 3 = 231 bytes: pad 0 and 3 leave rows unaligned, pad 5 gives 236: the dword stores)."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.mjpeg import MjpegDecoder
    H, W = 45, 77
    jpegs = [_pillow(_picture(H, W, 10 + k, noise=4.0 + 20.0 * k), quality=60 + 15 * k, subsampling="4:2:0", restart_marker_blocks=2 + k)
             for k in range(3)]
    assert len(set(len(j) for j in jpegs)) == 3
    dec = MjpegDecoder.for_stream(jpegs[0], device=cuda, batch=3)
    used = [dec.stage(j, dec.h_in[k]) for k, j in enumerate(jpegs)]
    stride = dec.in_stride
    g_in = Guarded(cuda, 3 * stride, init=dec.h_in.numpy().reshape(-1), dtype=torch.uint8)
    row = W * 3 + pad
    g_out = Guarded(cuda, 3 * H * row, dtype=torch.uint8)
    g_ws = Guarded(cuda, 3 * dec.layout["frame"], dtype=torch.uint8)
    g_st = Guarded(cuda, 3 * 4, dtype=torch.uint8)
    before = g_in.np()
    _lib.call("stabnet_mjpeg_decode", ptr(g_in.t), stride, 3, H, W, 3, 420, 0, ptr(g_out.t), row, H * row, ptr(g_st.t), ptr(g_ws.t),
              g_ws.n, 3, stream_ptr(cuda), device=cuda)
    torch.cuda.synchronize()
    for what, g in (("in", g_in), ("out", g_out), ("workspace", g_ws), ("status", g_st)):
        g.check(what)
    assert np.array_equal(g_in.np(), before) and not g_st.np().any()
    out = g_out.np().reshape(3, H, row)
    assert (out[:, :, W * 3:] == 0xEE).all()                            # the bytes between the rows are the caller's
    for k, j in enumerate(jpegs):
        assert np.array_equal(out[k, :, :W * 3].reshape(H, W, 3), D.decode(j))
    assert used == [dec.slot_bytes(len(j)) for j in jpegs]


def test_hipgraph_two_replays(cuda):
    from stabnet_amd.mjpeg import MjpegDecoder
    jpegs = [_pillow(_picture(33, 50, 20 + k), quality=80, subsampling="4:2:0", restart_marker_blocks=3) for k in range(3)]
    dec = MjpegDecoder.for_stream(jpegs[0], device=cuda)
    out = torch.zeros((1, 33, 50, 3), dtype=torch.uint8, device=cuda)

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
        assert np.array_equal(out[0].cpu().numpy(), D.decode(j))


@pytest.mark.parametrize("C,sub", [(3, "420"), (3, "444"), (1, "420")])
def test_encoder_round_trip(cuda, C, sub):
    """The project's own encoder (csrc/mjpeg.hip) -> the decoder: the model's pixels, and Pillow's where it is libjpeg-turbo."""
    from stabnet_amd.mjpeg import MjpegDecoder, MjpegEncoder
    H, W = 45, 77
    img = _picture(H, W, 30)
    img = img if C == 3 else np.ascontiguousarray(img[..., 0])
    enc = MjpegEncoder(H, W, C, quality=80, subsampling=sub, device=cuda)
    jpeg = enc.encode_bytes(torch.from_numpy(img).to(cuda))[0]
    dec = MjpegDecoder.for_stream(jpeg, device=cuda)
    assert not dec.host_entropy                                          # the encoder writes restart intervals
    got = dec.decode([jpeg])[0].cpu().numpy()
    assert int(dec.status[0]) == 0
    assert np.array_equal(got, D.decode(jpeg))
    if D.have_turbo():
        assert np.array_equal(got, D.pillow_bgr(jpeg))
