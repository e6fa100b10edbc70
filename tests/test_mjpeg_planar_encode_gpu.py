"""GPU: the planar encoder (stabnet_mjpeg_encode_i420, mjpeg_transform_planar_kernel of csrc/mjpeg.hip) against the float64 model of
tests/jpeg_planar_model.py, the plain-Python entropy coder / decoder of tests/jpeg_model.py and Pillow as an independent decoder.
  coefficients  the stream, decoded by the model's decoder, gives transform_planes' coefficients by the rule of test_mjpeg_gpu.py: a
                coefficient may differ by +-1 only where the unrounded coef / Q lies within 0.01 of a half-integer, and at most 3 % differ
  bytes         header + the model's entropy coder over the stream's own coefficients gives the stream exactly
  decoder       Pillow opens every stream without warnings, at the right size, mode and tables
  memory        guard bands, frames further apart than their size at an unaligned base, max_bytes, batch independence, repeatability;
                a captured graph replayed on changing input gives the eager bytes
"""
import functools
import io
import warnings

import numpy as np
import pytest

import jpeg_model as M
import jpeg_planar_model as P

pytestmark = pytest.mark.gpu


def _pil(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return im


def _encoder(H, W, C, quality, R, batch=1, **kw):
    from stabnet_amd.mjpeg import MjpegEncoder
    return MjpegEncoder(H, W, C, quality=quality, restart_mcus=M.restart_of(R, H, W, C, "420"), device="cuda:0", batch=batch, planar=True, **kw)


@functools.lru_cache(maxsize=None)
def _run(case):
    import torch
    kind, H, W, C, quality, R, batch = case
    frames = P.make_planes(kind, H, W, C, batch)
    enc = _encoder(H, W, C, quality, R, batch)
    streams = enc.encode_bytes(torch.from_numpy(frames).cuda())
    return frames, enc, streams


def _check_coefficients(stream, frame, H, W, C, ql, qc):
    d = M.decode(stream)
    coef, ratio = P.transform_planes(*P.split(frame, H, W, C), ql, qc)
    assert d["coef"].shape == coef.shape
    diff = d["coef"] - coef
    tie = M.near_tie(ratio)
    wrong = (diff != 0) & ~(tie & (np.abs(diff) <= 1))
    share = (diff != 0).mean()
    print("coefficients %d, differing at a tie %d (%.4f %%), near a tie %.3f %%, wrong %d" % (diff.size, (diff != 0).sum(), 100 * share,
                                                                                           100 * tie.mean(), wrong.sum()))
    assert wrong.sum() == 0, "first wrong coefficients (mcu, block, k): %s" % np.argwhere(wrong)[:5].tolist()
    assert share <= 0.03
    return d


@pytest.mark.parametrize("case", P.ENCODE_CASES, ids=P.case_id)
def test_coefficients_equal_the_model(cuda, case):
    kind, H, W, C, quality, R, batch = case
    frames, enc, streams = _run(case)
    assert len(streams) == batch
    for frame, s in zip(frames, streams):
        d = _check_coefficients(s, frame, H, W, C, enc.q_luma, enc.q_chroma)
        assert (d["H"], d["W"], d["C"]) == (H, W, C) and d["restart"] == enc.restart_mcus
        assert d["sampling"] == ([(2, 2), (1, 1), (1, 1)] if C == 3 else [(1, 1)])
        assert np.array_equal(d["qtables"][0], enc.q_luma) and (C == 1 or np.array_equal(d["qtables"][1], enc.q_chroma))


@pytest.mark.parametrize("case", P.ENCODE_CASES, ids=P.case_id)
def test_bytes_equal_header_and_the_model_entropy_coder(cuda, case):
    from stabnet_amd.mjpeg import MjpegEncoder
    kind, H, W, C, quality, R, batch = case
    frames, enc, streams = _run(case)
    # the header, the size bound and the workspace are the BGR encoder's of C = planes, 4:2:0
    bgr = MjpegEncoder(H, W, C, quality=quality, subsampling="420", restart_mcus=enc.restart_mcus, device="cuda:0", batch=batch)
    assert enc.header == bgr.header == M.header(H, W, C, "420", enc.restart_mcus, enc.q_luma, enc.q_chroma)
    assert enc.max_bytes == bgr.max_bytes and enc.workspace.numel() == bgr.workspace.numel()
    for s in streams:
        d = M.decode(s)
        assert s[:d["header_bytes"]] == enc.header
        assert enc.header + M.entropy_encode(d["coef"], C, "420", enc.restart_mcus) + b"\xff\xd9" == s
        nint = -(-d["coef"].shape[0] // enc.restart_mcus)
        assert d["n_rst"] == nint - 1
        if R == "all":
            assert d["n_rst"] == 0
        assert len(s) <= enc.max_bytes


@pytest.mark.parametrize("case", P.ENCODE_CASES, ids=P.case_id)
def test_pillow_decodes_every_stream(cuda, case):
    kind, H, W, C, quality, R, batch = case
    frames, enc, streams = _run(case)
    for frame, s in zip(frames, streams):
        im = _pil(s)
        assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")
        q = {k: np.asarray(v) for k, v in im.quantization.items()}
        assert np.array_equal(q[0], enc.q_luma) and (C == 1 or np.array_equal(q[1], enc.q_chroma))
        # Pillow's Y of the stream is the model decoder's Y of it, and stays near the source's Y: within the quantiser's reach
        back = P.decode_i420(s)
        ycc = P.pillow_draft_planes(s)
        assert np.array_equal(ycc[..., 0] if C == 3 else ycc, P.split(back, H, W, C)[0])
        model = P.encode_i420(frame, H, W, C, restart_mcus=enc.restart_mcus, q_luma=enc.q_luma, q_chroma=enc.q_chroma)
        p_gpu, p_model = (M.psnr(P.decode_i420(x), frame) for x in (s, model))
        print("QUALITY %s: psnr gpu %.3f model %.3f dB; bytes gpu %d model %d%s" % (P.case_id(case), p_gpu, p_model, len(s), len(model),
                                                                                " identical to the model" if s == model else ""))
        assert abs(p_gpu - p_model) <= 0.05 if np.isfinite(p_model) else np.isinf(p_gpu)


@pytest.mark.parametrize("kind", ["checker1", "checker8"])
@pytest.mark.parametrize("C", [3, 1])
def test_checkerboards_at_quality_100_reach_the_clamps(cuda, kind, C):
    import torch
    H, W = 40, 56
    frame = P.make_planes(kind, H, W, C)
    enc = _encoder(H, W, C, 100, 3)
    (s,) = enc.encode_bytes(torch.from_numpy(frame).cuda())
    d = _check_coefficients(s, frame[0], H, W, C, enc.q_luma, enc.q_chroma)
    assert np.abs(d["coef"][..., 1:]).max() <= 1023 and np.abs(d["coef"][..., 0]).max() <= 1024
    assert np.abs(d["coef"]).max() >= 512                       # the largest AC category (10) or an 11-bit DC difference occurs
    assert enc.header + M.entropy_encode(d["coef"], C, "420", enc.restart_mcus) + b"\xff\xd9" == s
    assert _pil(s).size == (W, H)


@pytest.mark.parametrize("C,R,offset", [(3, 1, 0), (3, "row", 3), (1, 2, 5)])
def test_guard_bands_strides_batch_independence_and_repeatability(cuda, C, R, offset):
    """46x78 (grey: 45x77): partial MCUs on both sides; the source at a base offset of 0, 3, 5 bytes with frames 37 bytes further apart
    than their size, so the dword and the byte loads both run; the source is not written."""
    import torch
    from stabnet_amd import _lib
    from _guarded import Guarded
    H, W = (46, 78) if C == 3 else (45, 77)
    N, G = 3, 4096
    frames = P.make_planes("texture", H, W, C, N, seed=9)
    enc = _encoder(H, W, C, 75, R, batch=N)
    dev = torch.device("cuda:0")
    fb, stride = enc.frame_bytes, enc.frame_bytes + 37
    ws_bytes = _lib.lib().stabnet_mjpeg_workspace_bytes(N, H, W, C, 420, enc.restart_mcus)
    assert ws_bytes == enc.workspace.numel()
    g_src = Guarded(dev, offset + 2 * stride + fb, dtype=torch.uint8)
    src = g_src.t[offset:].as_strided((N, fb), (stride, 1))
    src.copy_(torch.from_numpy(frames))
    src_before = g_src.np()
    raw_out = torch.full((G + N * enc.max_bytes + G,), 0xA5, dtype=torch.uint8, device=dev)
    raw_ws = torch.full((G + ws_bytes + G,), 0xA5, dtype=torch.uint8, device=dev)
    raw_nb = torch.full((16 + N + 16,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    out = raw_out[G:G + N * enc.max_bytes].view(N, enc.max_bytes)
    nb = raw_nb[16:16 + N]
    enc.workspace = raw_ws[G:G + ws_bytes]
    enc.encode(src, out=out, nbytes=nb)
    torch.cuda.synchronize()
    for raw in (raw_out, raw_ws):
        assert bool((raw[:G] == 0xA5).all()) and bool((raw[-G:] == 0xA5).all())
    assert bool((raw_nb[:16] == -0x5A5A5A5B).all()) and bool((raw_nb[-16:] == -0x5A5A5A5B).all())
    g_src.check("src")
    assert np.array_equal(g_src.np(), src_before)
    lens = nb.cpu().tolist()
    assert all(0 < n <= enc.max_bytes for n in lens)
    first = [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lens)]
    for i, n in enumerate(lens):
        assert bool((out[i, n:] == 0xA5).all())                 # nothing was written past the stream
    # a second run gives the same bytes; a dense, aligned copy gives the same bytes; a frame alone gives what it gave in the batch
    enc.encode(src, out=out, nbytes=nb)
    torch.cuda.synchronize()
    assert [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(nb.cpu().tolist())] == first
    single = _encoder(H, W, C, 75, R)
    dense = torch.from_numpy(frames).cuda()
    for i in range(N):
        assert single.encode_bytes(dense[i:i + 1]) == [first[i]]
    for f, s in zip(frames, first):
        _check_coefficients(s, f, H, W, C, enc.q_luma, enc.q_chroma)
        assert _pil(s).size == (W, H)


def test_capture_in_a_graph_and_replay_on_changing_input(cuda):
    import torch
    H, W, C = 46, 78, 3
    frames = P.make_planes("texture", H, W, C, 3, seed=4)
    enc = _encoder(H, W, C, 75, 1)
    eager = [enc.encode_bytes(torch.from_numpy(frames[i:i + 1]).cuda())[0] for i in range(3)]
    assert len(set(eager)) == 3
    buf = torch.from_numpy(frames[0:1]).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            enc.encode(buf)
    for i in (1, 2, 0):
        buf.copy_(torch.from_numpy(frames[i:i + 1]))
        g.replay()
        torch.cuda.synchronize()
        n = int(enc.nbytes[0].item())
        assert enc.out[0, :n].cpu().numpy().tobytes() == eager[i]


def test_decoder_planes_into_the_encoder(cuda):
    """The two ends together, with nothing in between: the planar decoder's buffer is the planar encoder's input."""
    import torch
    from stabnet_amd.mjpeg import MjpegDecoder
    jpeg, _ = P.load_golden()["420_46x78_q30_noisy"]
    dec = MjpegDecoder.for_stream(jpeg, device="cuda:0", planar=True)
    planes = dec.decode([jpeg])
    enc = _encoder(46, 78, 3, 90, 2)
    (s,) = enc.encode_bytes(planes)
    _check_coefficients(s, P.decode_i420(jpeg), 46, 78, 3, enc.q_luma, enc.q_chroma)


def test_profiler_kinds_of_the_four_launches(cuda):
    import torch
    from stabnet_amd.deploy import Profiler
    enc = _encoder(46, 78, 3, 75, 1)
    prof = Profiler(64)
    enc.encode(torch.from_numpy(P.make_planes("texture", 46, 78, 3)).cuda(), prof=prof)
    names = [r[0] for r in prof.records()]
    assert names == ["mjpeg_transform_planar_kernel", "mjpeg_entropy_kernel", "mjpeg_layout_kernel", "mjpeg_gather_kernel"]
    assert all(r[3] > 0 for r in prof.records())
    nblk = 3 * 5 * 6
    assert prof.records()[0][3] == 46 * 78 * 3 // 2 + nblk * 128


def test_refusals(cuda):
    import torch
    from stabnet_amd import _lib
    from stabnet_amd._tensor import ptr, stream_ptr
    enc = _encoder(16, 16, 3, 75, 1)
    fb = enc.frame_bytes
    with pytest.raises(_lib.StabnetError):
        enc.encode(torch.zeros((1, fb), dtype=torch.uint8))                                     # host tensor: no CPU fallback
    with pytest.raises(_lib.StabnetError, match="planar frames"):
        enc.encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda:0"))              # a BGR frame is not a planar one
    with pytest.raises(_lib.StabnetError, match="planar frames"):
        enc.encode(torch.zeros((1, fb - 1), dtype=torch.uint8, device="cuda:0"))
    good = torch.zeros((1, fb), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_lib.StabnetError, match="out_stride"):
        enc.encode(good, out=torch.zeros((1, 64), dtype=torch.uint8, device="cuda:0"), nbytes=enc.nbytes)
    L = _lib.lib()
    enc.out.fill_(0xA5)

    def call(H=16, W=16, planes=3, fs=fb, R=1):
        with torch.cuda.device(enc.device):
            return L.stabnet_mjpeg_encode_i420(ptr(good), 1, H, W, planes, fs, R, ptr(enc._tables), enc._tables.data_ptr() + 128, ptr(enc._header),
                                               len(enc.header), ptr(enc.out), enc.out.stride(0), ptr(enc.nbytes), ptr(enc.workspace),
                                               enc.workspace.numel(), stream_ptr(enc.device), None)

    for kw, word in ((dict(planes=2), b"planes must be 1"), (dict(H=15), b"odd side"), (dict(W=15), b"odd side"), (dict(fs=fb - 1), b"frame_stride_bytes"),
                     (dict(R=0), b"restart interval")):
        assert call(**kw) == -1 and word in L.stabnet_last_error(), (kw, L.stabnet_last_error())
    torch.cuda.synchronize()
    assert bool((enc.out == 0xA5).all())                                                         # nothing was launched
    assert call() == 0
