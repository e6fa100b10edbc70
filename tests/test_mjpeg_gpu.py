"""GPU: the baseline JPEG encoder of csrc/mjpeg.hip against the float64 model, the plain-Python entropy coder / decoder of
tests/jpeg_model.py and Pillow (libjpeg-turbo) as an independent decoder.

  coefficients  the stream, decoded by the model's decoder, gives the model's quantised coefficients; a coefficient may differ by +-1
                only where the model's unrounded coef / Q lies within 0.01 of a half-integer (a margin over float32 rounding: the
                float32 and float64 runs of the model differ by < 1e-4 there), and such exemptions are at most 3 % of all
  bytes         re-encoding the stream's own coefficients with the model's entropy coder behind stabnet_mjpeg_header's bytes gives the
                stream exactly: Huffman codes, DC prediction per interval, 1-bit padding, stuffing, RSTm numbering, EOI, length
  decoder       Pillow opens every stream without warnings; its PSNR against the source is within 0.05 dB of the model stream's (they
                differ only by exempt ties); Pillow's own encoder with the same tables is printed beside it, not barred
  memory        guard bands around output, workspace and lengths stay intact; batch entries are independent; runs repeat; a captured
                graph replayed on changing input gives the eager bytes
"""
import functools
import io
import warnings

import numpy as np
import pytest

import jpeg_model as M

pytestmark = pytest.mark.gpu


def _pil(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return im


def _pil_pixels(im, C):
    return np.asarray(im.convert("RGB"))[..., ::-1] if C == 3 else np.asarray(im)[..., None]


def _encoder(H, W, C, sub, quality, R, batch=1, **kw):
    from stabnet_amd.mjpeg import MjpegEncoder
    return MjpegEncoder(H, W, C, quality=quality, subsampling=sub, restart_mcus=M.restart_of(R, H, W, C, sub), device="cuda:0", batch=batch, **kw)


@functools.lru_cache(maxsize=None)
def _run(case):
    import torch
    kind, H, W, C, sub, quality, R, batch = case
    imgs = M.make_input(kind, H, W, C, batch)
    enc = _encoder(H, W, C, sub, quality, R, batch)
    streams = enc.encode_bytes(torch.from_numpy(imgs).cuda())
    return imgs, enc, streams


def _check_coefficients(stream, img, sub, ql, qc):
    d = M.decode(stream)
    coef, ratio = M.transform(img, sub, ql, qc)
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


@pytest.mark.parametrize("case", M.GPU_CASES, ids=M.case_id)
def test_coefficients_equal_the_model(cuda, case):
    kind, H, W, C, sub, quality, R, batch = case
    imgs, enc, streams = _run(case)
    assert len(streams) == batch
    for img, s in zip(imgs, streams):
        d = _check_coefficients(s, img, sub, enc.q_luma, enc.q_chroma)
        assert (d["H"], d["W"], d["C"]) == (H, W, C) and d["restart"] == enc.restart_mcus
        assert np.array_equal(d["qtables"][0], enc.q_luma) and (C == 1 or np.array_equal(d["qtables"][1], enc.q_chroma))


@pytest.mark.parametrize("case", M.GPU_CASES, ids=M.case_id)
def test_bytes_equal_the_model_entropy_coder(cuda, case):
    kind, H, W, C, sub, quality, R, batch = case
    imgs, enc, streams = _run(case)
    for s in streams:
        d = M.decode(s)
        assert s[:d["header_bytes"]] == enc.header
        again = enc.header + M.entropy_encode(d["coef"], C, sub, enc.restart_mcus) + b"\xff\xd9"
        assert len(again) == len(s)
        assert again == s
        nint = -(-d["coef"].shape[0] // enc.restart_mcus)
        assert d["n_rst"] == nint - 1
        if R == "all":
            assert d["n_rst"] == 0
        assert len(s) <= enc.max_bytes


@pytest.mark.parametrize("case", M.GPU_CASES, ids=M.case_id)
def test_pillow_decodes_and_psnr_follows_the_model(cuda, case):
    from PIL import Image
    kind, H, W, C, sub, quality, R, batch = case
    imgs, enc, streams = _run(case)
    for img, s in zip(imgs, streams):
        im = _pil(s)
        assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")
        q = {k: np.asarray(v) for k, v in im.quantization.items()}
        assert np.array_equal(q[0], enc.q_luma) and (C == 1 or np.array_equal(q[1], enc.q_chroma))
        coef, _ = M.transform(img, sub, enc.q_luma, enc.q_chroma)
        model = enc.header + M.entropy_encode(coef, C, sub, enc.restart_mcus) + b"\xff\xd9"
        buf = io.BytesIO()
        src = Image.fromarray(img[..., ::-1].copy()) if C == 3 else Image.fromarray(img[..., 0])
        tabs = [[int(v) for v in enc.q_luma], [int(v) for v in enc.q_chroma]][:2 if C == 3 else 1]
        src.save(buf, "JPEG", qtables=tabs, subsampling={"420": 2, "444": 0}[sub])
        own = Image.open(io.BytesIO(buf.getvalue()))
        assert np.array_equal(np.asarray(own.quantization[0]), enc.q_luma)
        p_gpu, p_model, p_pil = (M.psnr(_pil_pixels(x, C), img) for x in (im, _pil(model), own))
        print("QUALITY %s: psnr gpu %.3f model %.3f pillow %.3f dB; bytes gpu %d model %d pillow %d (%+.1f %%)%s"
              % (M.case_id(case), p_gpu, p_model, p_pil, len(s), len(model), len(buf.getvalue()),
                 100.0 * (len(s) / len(buf.getvalue()) - 1), " identical to the model" if s == model else ""))
        if np.isinf(p_model):
            assert np.isinf(p_gpu)
        else:
            assert abs(p_gpu - p_model) <= 0.05


def test_stuffing_and_size_bound_on_noise_at_quality_100(cuda):
    import torch
    H, W = 48, 64
    img = M.make_input("noise", H, W, 3, seed=5)
    for sub, R in (("420", 2), ("444", 1)):
        enc = _encoder(H, W, 3, sub, 100, R)
        (s,) = enc.encode_bytes(torch.from_numpy(img).cuda())
        scan = s[len(enc.header):-2]
        assert b"\xff\x00" in scan
        assert len(s) <= enc.max_bytes
        d = _check_coefficients(s, img[0], sub, enc.q_luma, enc.q_chroma)
        assert enc.header + M.entropy_encode(d["coef"], 3, sub, enc.restart_mcus) + b"\xff\xd9" == s
        assert _pil(s).size == (W, H)


@pytest.mark.parametrize("kind", ["checker1", "checker8"])
@pytest.mark.parametrize("C,sub", [(3, "420"), (3, "444"), (1, "420")])
def test_checkerboards_at_quality_100_reach_the_clamps(cuda, kind, C, sub):
    import torch
    H, W = 40, 56
    img = M.make_input(kind, H, W, C)
    enc = _encoder(H, W, C, sub, 100, 3)
    (s,) = enc.encode_bytes(torch.from_numpy(img).cuda())
    d = _check_coefficients(s, img[0], sub, enc.q_luma, enc.q_chroma)
    assert np.abs(d["coef"][..., 1:]).max() <= 1023 and np.abs(d["coef"][..., 0]).max() <= 1024
    assert np.abs(d["coef"]).max() >= 512                       # the largest AC category (10) or an 11-bit DC difference occurs
    assert enc.header + M.entropy_encode(d["coef"], C, sub, enc.restart_mcus) + b"\xff\xd9" == s
    assert _pil(s).size == (W, H)


def test_custom_quant_tables_of_ones(cuda):
    import torch
    H, W = 24, 40
    img = M.make_input("checker1", H, W, 3)
    ones = np.ones(64, np.uint16)
    enc = _encoder(H, W, 3, "444", 75, 1, q_luma=ones, q_chroma=ones)
    (s,) = enc.encode_bytes(torch.from_numpy(img).cuda())
    d = _check_coefficients(s, img[0], "444", ones, ones)
    assert np.array_equal(d["qtables"][0], ones)
    assert _pil(s).size == (W, H)


@pytest.mark.parametrize("C,sub,R", [(3, "420", 1), (3, "444", 7), (1, "420", "row")])
def test_guard_bands_batch_independence_and_repeatability(cuda, C, sub, R):
    import torch
    from stabnet_amd import _lib
    H, W, N, G = 45, 77, 3, 4096
    imgs = M.make_input("texture", H, W, C, N, seed=9)
    enc = _encoder(H, W, C, sub, 75, R, batch=N)
    dev = torch.device("cuda:0")
    ws_bytes = _lib.lib().stabnet_mjpeg_workspace_bytes(N, H, W, C, int(sub), enc.restart_mcus)
    assert ws_bytes == enc.workspace.numel()
    raw_out = torch.full((G + N * enc.max_bytes + G,), 0xA5, dtype=torch.uint8, device=dev)
    raw_ws = torch.full((G + ws_bytes + G,), 0xA5, dtype=torch.uint8, device=dev)
    raw_nb = torch.full((16 + N + 16,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    out = raw_out[G:G + N * enc.max_bytes].view(N, enc.max_bytes)
    nb = raw_nb[16:16 + N]
    enc.workspace = raw_ws[G:G + ws_bytes]
    d_img = torch.from_numpy(imgs).cuda()
    enc.encode(d_img, out=out, nbytes=nb)
    torch.cuda.synchronize()
    for raw in (raw_out, raw_ws):
        assert bool((raw[:G] == 0xA5).all()) and bool((raw[-G:] == 0xA5).all())
    assert bool((raw_nb[:16] == -0x5A5A5A5B).all()) and bool((raw_nb[-16:] == -0x5A5A5A5B).all())
    lens = nb.cpu().tolist()
    assert all(0 < n <= enc.max_bytes for n in lens)
    first = [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lens)]
    # the untouched part of every frame's stride is still the fill: nothing was written past the stream
    for i, n in enumerate(lens):
        assert bool((out[i, n:] == 0xA5).all())
    # a second run gives the same bytes; a frame alone gives what it gave in the batch
    enc.encode(d_img, out=out, nbytes=nb)
    torch.cuda.synchronize()
    assert [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(nb.cpu().tolist())] == first
    single = _encoder(H, W, C, sub, 75, R)
    for i in range(N):
        assert single.encode_bytes(d_img[i:i + 1]) == [first[i]]
    for s in first:
        assert _pil(s).size == (W, H)


def test_capture_in_a_graph_and_replay_on_changing_input(cuda):
    import torch
    H, W, C = 144, 176, 3
    imgs = M.make_input("clip", H, W, C, 3, seed=4)
    enc = _encoder(H, W, C, "420", 75, 1)
    eager = [enc.encode_bytes(torch.from_numpy(imgs[i:i + 1]).cuda())[0] for i in range(3)]
    assert len(set(eager)) == 3
    buf = torch.from_numpy(imgs[0:1]).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            enc.encode(buf)
    for i in (1, 2, 0):
        buf.copy_(torch.from_numpy(imgs[i:i + 1]))
        g.replay()
        torch.cuda.synchronize()
        n = int(enc.nbytes[0].item())
        assert enc.out[0, :n].cpu().numpy().tobytes() == eager[i]


def test_profiler_kinds_of_the_four_launches(cuda):
    import torch
    from stabnet_amd.deploy import Profiler
    enc = _encoder(45, 77, 3, "420", 75, 1)
    prof = Profiler(64)
    enc.encode(torch.from_numpy(M.make_input("texture", 45, 77, 3)).cuda(), prof=prof)
    names = [r[0] for r in prof.records()]
    assert names == ["mjpeg_transform_kernel", "mjpeg_entropy_kernel", "mjpeg_layout_kernel", "mjpeg_gather_kernel"]
    assert all(r[3] > 0 for r in prof.records())


def test_wrong_device_arguments_raise(cuda):
    import torch
    from stabnet_amd import _lib
    enc = _encoder(16, 16, 3, "420", 75, 1)
    with pytest.raises(_lib.StabnetError):
        enc.encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8))           # host tensor: no CPU fallback
    with pytest.raises(_lib.StabnetError):
        enc.encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda:0"),
                   out=torch.zeros((1, 64), dtype=torch.uint8, device="cuda:0"), nbytes=enc.nbytes)        # stride below max_bytes
