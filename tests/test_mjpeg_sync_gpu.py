"""GPU: the parallel entropy back end of csrc/mjpeg_decode_sync.hip (self-synchronising Huffman decoding of streams without restart
markers) against the sequential host routine, stabnet_mjpeg_entropy_host, the host_entropy=True decoder and the golden pixels -- bit
for bit.
  coefficients   stages = 1: the fixture's streams without restart markers, Pillow streams (grey, 4:4:4, 4:2:0; 33x50, 40x56; optimised
                 tables; q100 noise) and a 96x128 noisy q95 4:2:0 stream of more than 2 x 256 x 16 bytes: three or more workgroups at
                 chunk_bytes 16, also at 32 and 128 (and the other streams at 8 and 4096: a symbol that skips a chunk, one chunk per
                 stream); rounds 0 (everything left to the repair), 1 and the default
  pixels         equal to the host_entropy=True decoder's and to the golden pixels
  batch          three streams of different lengths between guard bytes, aligned and unaligned output row strides
  graph          one captured hipGraph replayed twice with other streams in the slots
  selection      for_stream(parallel=True) on a DRI stream keeps the lane back end; for_stream(jpeg) stays as it was
Only valid streams go to the GPU (corrupt ones: tests/test_mjpeg_sync_cpu.py, the same bounded walk)."""
import numpy as np
import pytest
import torch

import jpeg_decode_model as D
from _guarded import Guarded
from test_mjpeg_sync_cpu import STREAMS, _noise, _parse, _picture, _pillow, _host

pytestmark = pytest.mark.gpu

GOLD = D.load_golden()
_REF = {}


def _big():
    """96x128 noisy q95 4:2:0: long enough for three workgroups of 256 chunks at chunk_bytes 16."""
    img = np.clip(_picture(96, 128, 40, noise=0.0).astype(np.int32) + (_noise(96, 128, 41).astype(np.int32) - 128) // 2, 0, 255).astype(np.uint8)
    return _pillow(img, quality=95, subsampling="4:2:0")


def _stream(name):
    return _big() if name == "420_96x128_q95_noisy" else STREAMS[name]


def _ref(name):
    """The sequential routine's coefficients, computed once per stream and shared."""
    if name not in _REF:
        jpeg = _stream(name)
        rc, info, blob = _parse(jpeg)
        rc, coef = _host(jpeg, info, blob)
        assert rc == 0
        coef.setflags(write=False)
        _REF[name] = coef
    return _REF[name]


def _parallel_decoder(cuda, jpeg, **kw):
    """for_stream(parallel=True) -- or, for the fixture's one-MCU stream that carries a DRI (and so keeps the lane back end there), the
    parallel decoder made by hand: it is a single interval all the same."""
    from stabnet_amd import mjpeg
    i = mjpeg.parse(jpeg)
    assert i["intervals"] == 1
    if i["restart"]:
        dec = mjpeg.MjpegDecoder(i["H"], i["W"], i["C"], i["subsampling"] or 420, device=cuda, parallel=True, **kw)
    else:
        dec = mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda, parallel=True, **kw)
    assert dec.parallel and not dec.host_entropy
    return dec


def _coef_sync(cuda, jpeg, chunk, rounds):
    dec = _parallel_decoder(cuda, jpeg, chunk_bytes=chunk, sync_rounds=rounds)
    used = dec.stage(jpeg, dec.h_in[0])
    dec.d_in[0, :used].copy_(dec.h_in[0, :used])
    dec.workspace.fill_(0x5A)
    dec.enqueue(dec.d_in, 1, None, dec.status[:1], stages=1)
    torch.cuda.synchronize()
    assert int(dec.status[0]) == 0
    lay = dec.layout
    return dec.workspace[lay["coef"]:lay["coef"] + 2 * dec.coef_count].cpu().numpy().view(np.int16), dec.sync_stats[0].cpu().tolist()


def test_the_big_stream_spans_three_workgroups():
    jpeg = _big()
    rc, info, _ = _parse(jpeg)
    assert rc == 0 and info[4:6] == [0, 1] and info[8] - info[7] > 2 * 256 * 16


@pytest.mark.parametrize("rounds", [0, 1, None])
@pytest.mark.parametrize("chunk", [16, 32, 128])
def test_coefficients_big_stream(cuda, chunk, rounds):
    jpeg = _big()
    got, stats = _coef_sync(cuda, jpeg, chunk, rounds)
    assert np.array_equal(got, _ref("420_96x128_q95_noisy"))
    rc, info, _ = _parse(jpeg)
    nc = -(-(info[8] - info[7]) // chunk)
    assert stats[0] == nc and 1 <= stats[1] <= nc
    if rounds == 0:
        assert stats[1] == 1
    print("chunk %d rounds %s: %d chunks, %d left to the repair" % (chunk, rounds, stats[0], stats[0] - stats[1]))


@pytest.mark.parametrize("name", list(STREAMS))
def test_coefficients_equal_host_routine(cuda, name):
    jpeg = STREAMS[name]
    for chunk, rounds in ((None, None), (8, 1), (16, 0), (4096, None)):
        got, stats = _coef_sync(cuda, jpeg, chunk, rounds)
        assert np.array_equal(got, _ref(name)), (chunk, rounds)


@pytest.mark.parametrize("name", [n for n in STREAMS if n in GOLD])
def test_pixels_equal_host_entropy_decoder_and_golden(cuda, name):
    from stabnet_amd import mjpeg
    jpeg, px = GOLD[name]
    par = _parallel_decoder(cuda, jpeg)
    got = par.decode([jpeg])[0].cpu().numpy()
    assert int(par.status[0]) == 0
    host = mjpeg.MjpegDecoder.for_stream(jpeg, device=cuda, host_entropy=True)
    assert np.array_equal(got, host.decode([jpeg])[0].cpu().numpy())
    assert np.array_equal(got, px)


@pytest.mark.parametrize("pad", [0, 3, 5])
def test_batch_of_three_between_guards(cuda, pad):
    """Three frames of one geometry and different byte lengths in one call; every buffer between canary bands; rows `pad` bytes apart
    from the natural stride (77 x 3 = 231 bytes: pad 0 and 3 leave rows unaligned, pad 5 gives 236: the dword stores)."""
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    from stabnet_amd.mjpeg import MjpegDecoder
    H, W = 45, 77
    jpegs = [_pillow(_picture(H, W, 10 + k, noise=4.0 + 20.0 * k), quality=60 + 15 * k, subsampling="4:2:0") for k in range(3)]
    assert len(set(len(j) for j in jpegs)) == 3
    dec = MjpegDecoder.for_stream(jpegs[0], device=cuda, batch=3, parallel=True, chunk_bytes=16)
    used = [dec.stage(j, dec.h_in[k]) for k, j in enumerate(jpegs)]
    stride = dec.in_stride
    g_in = Guarded(cuda, 3 * stride, init=dec.h_in.numpy().reshape(-1), dtype=torch.uint8)
    row = W * 3 + pad
    g_out = Guarded(cuda, 3 * H * row, dtype=torch.uint8)
    g_ws = Guarded(cuda, dec.workspace.numel(), dtype=torch.uint8)
    g_st = Guarded(cuda, 3 * 4, dtype=torch.uint8)
    g_stats = Guarded(cuda, 3 * 2 * 4, dtype=torch.uint8)
    before = g_in.np()
    _lib.call("stabnet_mjpeg_decode_sync", ptr(g_in.t), stride, 3, H, W, 3, 420, ptr(g_out.t), row, H * row, ptr(g_st.t), ptr(g_ws.t),
              g_ws.n, 3, 16, -1, ptr(g_stats.t), stream_ptr(cuda), device=cuda)
    torch.cuda.synchronize()
    for what, g in (("in", g_in), ("out", g_out), ("workspace", g_ws), ("status", g_st), ("stats", g_stats)):
        g.check(what)
    assert np.array_equal(g_in.np(), before) and not g_st.np().any()
    out = g_out.np().reshape(3, H, row)
    assert (out[:, :, W * 3:] == 0xEE).all()                            # the bytes between the rows are the caller's
    for k, j in enumerate(jpegs):
        assert np.array_equal(out[k, :, :W * 3].reshape(H, W, 3), D.decode(j))
    stats = g_stats.np().view(np.int32).reshape(3, 2)
    for k, j in enumerate(jpegs):
        rc, info, _ = _parse(j)
        assert stats[k, 0] == -(-(info[8] - info[7]) // 16) and 1 <= stats[k, 1] <= stats[k, 0]
    assert used == [dec.slot_bytes(len(j)) for j in jpegs]


def test_hipgraph_two_replays(cuda):
    from stabnet_amd.mjpeg import MjpegDecoder
    jpegs = [_pillow(_picture(33, 50, 20 + k, noise=6.0 + 10.0 * k), quality=80 + 5 * k, subsampling="4:2:0") for k in range(3)]
    dec = MjpegDecoder.for_stream(jpegs[0], device=cuda, parallel=True)
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


def test_back_end_selection(cuda):
    from stabnet_amd import _lib, mjpeg
    dri, px = GOLD["420_45x77_q75_r3"]
    dec = mjpeg.MjpegDecoder.for_stream(dri, device=cuda, parallel=True)
    assert not dec.parallel and not dec.host_entropy                     # a DRI stream keeps one lane per interval
    assert np.array_equal(dec.decode([dri])[0].cpu().numpy(), px)
    plain = GOLD["420_45x77_q75"][0]
    assert mjpeg.parse(plain)["restart"] == 0
    d0 = mjpeg.MjpegDecoder.for_stream(plain, device=cuda)
    assert d0.host_entropy and not d0.parallel                           # the default stays what test_mjpeg_decode_gpu.py pins
    d1 = mjpeg.MjpegDecoder.for_stream(plain, device=cuda, parallel=True)
    assert d1.parallel and not d1.host_entropy
    with pytest.raises(_lib.StabnetError, match="excludes host_entropy"):
        mjpeg.MjpegDecoder(45, 77, 3, 420, device=cuda, parallel=True, host_entropy=True)
    with pytest.raises(_lib.StabnetError, match="restart intervals"):     # stage() names a frame of the other kind
        d1.stage(dri, d1.h_in[0], frame=3)
