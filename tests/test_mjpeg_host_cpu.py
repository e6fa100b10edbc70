"""CPU: the host half of the MJPEG encoder (tables, header, argument checks) against the model of tests/jpeg_model.py and against
Pillow (libjpeg-turbo) as an independent decoder; and the model on its own: its decoder inverts its encoder, Pillow decodes its streams,
and the share of coefficients near a rounding tie stays under 2.5 % on every input the GPU tests use."""
import ctypes
import io
import warnings

import numpy as np
import pytest

import jpeg_model as M


def _pil_open(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return im


def _pil_tables(im):
    """Image.quantization in natural order whatever this Pillow returns: compared through a stream whose tables are known."""
    return {k: np.asarray(v, np.int64) for k, v in im.quantization.items()}


def _c_tables(quality):
    from stabnet_amd import mjpeg
    return mjpeg.quant_tables(quality)


@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
def test_quant_tables_equal_the_model(quality):
    ql, qc = _c_tables(quality)
    ml, mc = M.quant_tables(quality)
    assert np.array_equal(ql, ml) and np.array_equal(qc, mc)
    assert ql.min() >= 1 and ql.max() <= 255


@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
@pytest.mark.parametrize("C,sub,mode", [(3, "420", "RGB"), (3, "444", "RGB"), (1, "420", "L")])
def test_header_plus_model_scan_opens_in_pillow(quality, C, sub, mode):
    from stabnet_amd import mjpeg
    H, W, R = 45, 77, 4
    img = M.make_input("texture", H, W, C)[0]
    ql, qc = _c_tables(quality)
    head = mjpeg.header_bytes(H, W, C, sub, R, ql, qc)
    assert head == M.header(H, W, C, sub, R, ql, qc)                  # two independent writers of the same layout
    coef, _ = M.transform(img, sub, ql, qc)
    data = head + M.entropy_encode(coef, C, sub, R) + b"\xff\xd9"
    im = _pil_open(data)
    assert im.size == (W, H) and im.mode == mode
    q = _pil_tables(im)
    zz_or_nat = lambda t: np.array_equal(q_, t) or np.array_equal(q_[M.ZIGZAG], t) or np.array_equal(q_, t[M.ZIGZAG])
    q_ = q[0]
    assert zz_or_nat(ql.astype(np.int64))
    if C == 3:
        q_ = q[1]
        assert zz_or_nat(qc.astype(np.int64))
    # what Pillow decodes is the picture, as well as Pillow's own encoder (same tables, same subsampling) keeps it: the two differ
    # only in integer against float arithmetic before the quantiser, measured at -0.05 .. +0.02 dB; 0.3 dB would be a wrong table
    from PIL import Image
    dec = np.asarray(im.convert("RGB"))[..., ::-1] if C == 3 else np.asarray(im)[..., None]
    buf = io.BytesIO()
    src = Image.fromarray(img[..., ::-1].copy()) if C == 3 else Image.fromarray(img[..., 0])
    src.save(buf, "JPEG", qtables=[[int(v) for v in ql], [int(v) for v in qc]][:2 if C == 3 else 1], subsampling={"420": 2, "444": 0}[sub])
    ref = Image.open(io.BytesIO(buf.getvalue()))
    assert np.array_equal(_pil_tables(ref)[0], ql)
    refdec = np.asarray(ref.convert("RGB"))[..., ::-1] if C == 3 else np.asarray(ref)[..., None]
    assert M.psnr(dec, img) > M.psnr(refdec, img) - 0.3, (M.psnr(dec, img), M.psnr(refdec, img))


def test_pillow_returns_tables_in_natural_order():
    """The comparison above accepts either order; this pins which one this Pillow uses, as the GPU tests rely on it."""
    from stabnet_amd import mjpeg
    ql, qc = _c_tables(75)
    head = mjpeg.header_bytes(16, 16, 3, "420", 1, ql, qc)
    coef, _ = M.transform(M.make_input("texture", 16, 16, 3)[0], "420", ql, qc)
    im = _pil_open(head + M.entropy_encode(coef, 3, "420", 1) + b"\xff\xd9")
    q = _pil_tables(im)
    assert np.array_equal(q[0], ql) and np.array_equal(q[1], qc)


def test_huffman_tables_are_the_ones_libjpeg_writes():
    """Annex K typed twice (here and in the HIP source) is checked against a third copy: the DHT segments of a non-optimised Pillow file."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(M.make_input("texture", 32, 32, 3)[0][..., ::-1].copy()).save(buf, "JPEG", quality=75, optimize=False)
    data = buf.getvalue()
    segs, p = {}, 2
    while data[p + 1] != 0xDA:
        ln = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xC4:
            s = data[p + 4:p + 2 + ln]
            while s:
                n = sum(s[1:17])
                segs[s[0]] = (list(s[1:17]), list(s[17:17 + n]))
                s = s[17 + n:]
        p += 2 + ln
    assert segs[0x00] == (M.DC_LUMA[0], M.DC_LUMA[1]) and segs[0x01] == (M.DC_CHROMA[0], M.DC_CHROMA[1])
    assert segs[0x10] == (M.AC_LUMA[0], M.AC_LUMA[1]) and segs[0x11] == (M.AC_CHROMA[0], M.AC_CHROMA[1])
    from stabnet_amd import mjpeg
    ql, qc = _c_tables(75)
    mine = M.decode(mjpeg.header_bytes(8, 8, 3, "444", 1, ql, qc) + M.entropy_encode(np.zeros((1, 3, 64), int), 3, "444", 1) + b"\xff\xd9")
    assert mine["coef"].shape == (1, 3, 64) and not mine["coef"].any()


@pytest.mark.parametrize("C,sub", [(3, "420"), (3, "444"), (1, "420")])
@pytest.mark.parametrize("R", [1, 4, "row", "all"])
def test_model_decoder_inverts_model_encoder_and_pillow_decodes(C, sub, R):
    H, W = 45, 77
    img = M.make_input("texture", H, W, C, seed=3)[0]
    r = M.restart_of(R, H, W, C, sub)
    data = M.encode(img, 75, sub, r)
    ql, qc = M.quant_tables(75)
    coef, _ = M.transform(img, sub, ql, qc)
    d = M.decode(data)
    assert (d["H"], d["W"], d["C"], d["restart"]) == (H, W, C, r)
    assert np.array_equal(d["coef"], coef)
    assert d["n_rst"] == -(-coef.shape[0] // r) - 1
    assert data[:d["header_bytes"]] + M.entropy_encode(d["coef"], C, sub, r) + b"\xff\xd9" == data
    im = _pil_open(data)
    assert im.size == (W, H)


def test_model_stuffing_and_extremes():
    ql = qc = np.ones(64, np.int64)
    img = M.make_input("noise", 48, 64, 3, seed=5)[0]
    coef, _ = M.transform(img, "420", ql, qc)
    scan = M.entropy_encode(coef, 3, "420", 2)
    assert b"\xff\x00" in scan
    data = M.header(48, 64, 3, "420", 2, ql, qc) + scan + b"\xff\xd9"
    assert np.array_equal(M.decode(data)["coef"], coef)
    _pil_open(data)
    for kind in ("checker1", "checker8"):
        img = M.make_input(kind, 32, 48, 3)[0]
        coef, _ = M.transform(img, "444", ql, qc)
        assert np.abs(coef[..., 1:]).max() <= 1023 and np.abs(coef[..., 0]).max() <= 1024
        data = M.header(32, 48, 3, "444", 1, ql, qc) + M.entropy_encode(coef, 3, "444", 1) + b"\xff\xd9"
        assert np.array_equal(M.decode(data)["coef"], coef)
        _pil_open(data)


@pytest.mark.parametrize("case", M.GPU_CASES, ids=M.case_id)
def test_share_of_near_ties_on_the_gpu_inputs(case):
    """The GPU test exempts coefficients within 0.01 of a rounding tie, at most 3 % of all: the inputs themselves stay under 2.5 %."""
    kind, H, W, C, sub, quality, R, batch = case
    ql, qc = M.quant_tables(quality)
    for img in M.make_input(kind, H, W, C, batch):
        _, ratio = M.transform(img, sub, ql, qc)
        share = M.near_tie(ratio).mean()
        print("near-tie share %.3f %%" % (100 * share))
        assert share <= 0.025, share


def test_float32_model_rounds_like_float64():
    ql, qc = M.quant_tables(95)
    img = M.make_input("texture", 144, 176, 3)[0]
    c64, r64 = M.transform(img, "420", ql, qc)
    c32, r32 = M.transform(img, "420", ql, qc, dtype=np.float32)
    assert np.abs(r64 - r32).max() < 1e-3
    assert ((c64 != c32) & ~M.near_tie(r64)).sum() == 0


def test_bad_arguments_return_minus_one():
    from stabnet_amd import _lib
    L = _lib.lib()
    ql, qc = (ctypes.c_ushort * 64)(), (ctypes.c_ushort * 64)()
    assert L.stabnet_jpeg_quant_tables(0, ql, qc) == -1 and L.stabnet_jpeg_quant_tables(101, ql, qc) == -1
    assert L.stabnet_jpeg_quant_tables(75, None, qc) == -1 and b"null" in L.stabnet_last_error()
    assert L.stabnet_jpeg_quant_tables(75, ql, qc) == 0
    buf = (ctypes.c_ubyte * 1024)()
    hb = L.stabnet_mjpeg_header(16, 16, 3, 420, 1, ql, qc, buf, 1024)
    assert hb > 600
    assert L.stabnet_mjpeg_header(16, 16, 3, 420, 1, ql, qc, None, 0) == L.stabnet_mjpeg_header(16, 16, 3, 420, 1, ql, qc, buf, 1024)
    assert L.stabnet_mjpeg_header(16, 16, 2, 420, 1, ql, qc, buf, 1024) == -1          # channels
    assert L.stabnet_mjpeg_header(16, 16, 3, 422, 1, ql, qc, buf, 1024) == -1          # subsampling
    assert L.stabnet_mjpeg_header(16, 16, 3, 420, 0, ql, qc, buf, 1024) == -1          # restart interval
    assert L.stabnet_mjpeg_header(16, 16, 3, 420, 65536, ql, qc, buf, 1024) == -1
    assert L.stabnet_mjpeg_header(0, 16, 3, 420, 1, ql, qc, buf, 1024) == -1           # size
    assert L.stabnet_mjpeg_header(16, 16, 3, 420, 1, None, qc, buf, 1024) == -1
    assert L.stabnet_mjpeg_header(16, 16, 3, 420, 1, ql, qc, buf, 100) == -1           # cap
    assert L.stabnet_mjpeg_max_bytes(16, 16, 2, 420, 1) == 0 and L.stabnet_mjpeg_workspace_bytes(0, 16, 16, 3, 420, 1) == 0
    mb = L.stabnet_mjpeg_max_bytes(16, 16, 3, 420, 1)
    assert mb >= 6 * 416 + 600
    ws = L.stabnet_mjpeg_workspace_bytes(2, 16, 16, 3, 420, 1)
    assert ws >= 2 * (6 * 128 + 6 * 416)
    # encode: every check comes before any launch, so it is testable without a GPU (non-null dummies are never dereferenced)
    one = ctypes.c_void_p(16)
    enc = lambda **k: L.stabnet_mjpeg_encode(*[k.get(n, d) for n, d in (
        ("img", one), ("N", 1), ("H", 16), ("W", 16), ("C", 3), ("sub", 420), ("R", 1), ("ql", one), ("qc", one), ("hd", one), ("hb", hb),
        ("out", one), ("stride", mb), ("nb", one), ("ws", one), ("wsb", ws), ("st", None), ("prof", None))])
    for bad in (dict(img=None), dict(out=None), dict(nb=None), dict(ws=None), dict(ql=None), dict(qc=None), dict(hd=None)):
        assert enc(**bad) == -1 and b"null" in L.stabnet_last_error(), bad
    for bad in (dict(C=2), dict(sub=411), dict(R=0), dict(R=70000), dict(N=0), dict(H=0), dict(W=-3), dict(stride=mb - 1), dict(hb=0)):
        assert enc(**bad) == -1, bad
    assert enc(stride=mb - 1) == -1 and b"out_stride" in L.stabnet_last_error()
    assert enc(hb=hb + 1) == -1 and b"header_bytes" in L.stabnet_last_error()
    assert enc(wsb=ws // 2 - 1) == -3 and b"workspace" in L.stabnet_last_error()
