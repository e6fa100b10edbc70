"""CPU: the planar (YCbCr) Motion-JPEG route without a GPU -- its NumPy model (tests/jpeg_planar_model.py) against Pillow's own planes,
the model's float32 run against its float64 run, and every refusal that precedes the device: of the three C entries
(stabnet_mjpeg_decode_i420, stabnet_mjpeg_decode_sync_i420, stabnet_mjpeg_encode_i420) and of deploy_bundle.py --avi-in."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_decode_model as D
import jpeg_model as M
import jpeg_planar_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = P.load_golden()


# ---- the model against Pillow ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GOLDEN))
def test_model_planes_are_pillows(name):
    """Y equals libjpeg-turbo's Y; the h2v2 fancy upsampling of the model's Cb / Cr equals libjpeg-turbo's upsampled Cb / Cr."""
    jpeg, ycc = GOLDEN[name]
    info, y, cb, cr = P.decode_planes(jpeg)
    H, W = info["H"], info["W"]
    if info["C"] == 1:
        assert ycc.shape == (H, W) and np.array_equal(y, ycc)
        assert np.array_equal(P.decode_i420(jpeg), ycc.reshape(-1))
        return
    assert ycc.shape == (H, W, 3)
    assert np.array_equal(y, ycc[..., 0])
    assert np.array_equal(D.upsample_h2v2(cb, H, W), ycc[..., 1])
    assert np.array_equal(D.upsample_h2v2(cr, H, W), ycc[..., 2])
    frame = P.decode_i420(jpeg)
    assert frame.dtype == np.uint8 and frame.shape == (H * W * 3 // 2,)
    fy, fcb, fcr = P.split(frame, H, W, 3)
    assert np.array_equal(fy, y) and np.array_equal(fcb, cb) and np.array_equal(fcr, cr)


def test_golden_file_is_what_the_tool_writes_when_pillow_is_turbo():
    if not D.have_turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    for name, (jpeg, ycc) in GOLDEN.items():
        assert np.array_equal(P.pillow_draft_planes(D.with_dht(jpeg)), ycc), name


def test_model_refuses_what_has_no_dense_frame():
    odd = D.load_golden()["420_45x77_q75"][0]
    with pytest.raises(AssertionError):
        P.decode_i420(odd)
    with pytest.raises(AssertionError):
        P.decode_i420(D.load_golden()["444_33x50_q75_r2"][0])


# ---- the encoder's model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.ENCODE_CASES, ids=P.case_id)
def test_float32_differs_from_float64_only_at_ties(case):
    kind, H, W, C, quality, R, batch = case
    ql, qc = M.quant_tables(quality)
    differing = total = 0
    for frame in P.make_planes(kind, H, W, C, batch):
        y, cb, cr = P.split(frame, H, W, C)
        c64, ratio = P.transform_planes(y, cb, cr, ql, qc, np.float64)
        c32, _ = P.transform_planes(y, cb, cr, ql, qc, np.float32)
        diff = c32 - c64
        assert not ((diff != 0) & ~(M.near_tie(ratio) & (np.abs(diff) <= 1))).any()
        differing += int((diff != 0).sum())
        total += diff.size
    print("%s: float32 differs in %d of %d coefficients (%.4f %%)" % (P.case_id(case), differing, total, 100.0 * differing / total))
    assert differing / total <= 0.03


def test_transform_planes_is_the_bgr_models_dct_of_the_same_planes():
    """On a grey picture the planar model and jpeg_model.transform are the same arithmetic: the same coefficients."""
    H, W = 45, 77
    img = M.make_input("texture", H, W, 1)[0]
    ql, qc = M.quant_tables(75)
    a, ra = M.transform(img, "420", ql, qc)
    b, rb = P.transform_planes(img[..., 0], None, None, ql, qc)
    assert np.array_equal(a, b) and np.array_equal(ra, rb)


@pytest.mark.parametrize("case", [c for c in P.ENCODE_CASES if c[1] * c[2] >= 256], ids=P.case_id)
def test_quality_100_round_trip_keeps_the_psnr_the_model_predicts(case):
    """decode_i420(encode_i420(x)) at quality 100 (every Q = 1).  The quantiser rounds every coefficient of an orthonormal transform:
    error uniform in [-0.5, 0.5], variance 1/12 per sample; the integer IDCT rounds every sample once more: at most another 1/12 -- the
    clamp to [0, 255] only moves a sample towards its source.  MSE <= 1/6 in expectation, PSNR >= 10 log10(255^2 * 6) = 55.91 dB; 0.5 dB
    are left for jidctint's 13-bit constants and for the sample of a few thousand values.  Pillow reads the same stream: the same Y."""
    kind, H, W, C, _, R, batch = case
    R = M.restart_of(R, H, W, C, "420")
    floor = 10 * np.log10(255.0 ** 2 * 6) - 0.5
    for frame in P.make_planes(kind, H, W, C, batch):
        stream = P.encode_i420(frame, H, W, C, quality=100, restart_mcus=R)
        back = P.decode_i420(stream)
        for a, b, what in zip(P.split(back, H, W, C), P.split(frame, H, W, C), "Y Cb Cr".split()):
            if a is not None:
                p = M.psnr(a, b)
                print("%s %s: %.2f dB (floor %.2f)" % (P.case_id(case), what, p, floor))
                assert p >= floor
        ycc = P.pillow_draft_planes(stream)
        assert np.array_equal(ycc[..., 0] if C == 3 else ycc, P.split(back, H, W, C)[0])


# ---- refusals of the C entries that need no device ----------------------------------------------------------------------------------------
def _L():
    from stabnet_amd import _lib
    return _lib.lib()


def _refused(rc, word):
    err = _L().stabnet_last_error()
    assert rc == -1 and word in err, (rc, err)


def test_decode_i420_refuses_before_any_launch():
    L = _L()
    one, al = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    H, W = 16, 32
    blob = L.stabnet_mjpeg_decode_blob_bytes(H, W, 3, 420)
    ws = L.stabnet_mjpeg_decode_workspace_bytes(2, H, W, 3, 420)
    stride = (blob + 4096 + 15) & ~15
    dec = lambda **k: L.stabnet_mjpeg_decode_i420(*[k.get(n, d) for n, d in (
        ("inp", al), ("in_stride", stride), ("N", 2), ("H", H), ("W", W), ("C", 3), ("sub", 420), ("up", 0), ("out", one),
        ("fs", H * W * 3 // 2), ("status", one), ("ws", al), ("wsb", ws), ("st", None), ("prof", None))])
    for bad in (dict(inp=None), dict(out=None), dict(status=None), dict(ws=None)):
        _refused(dec(**bad), b"null")
    _refused(dec(H=17), b"odd side")
    _refused(dec(W=31), b"odd side")
    _refused(dec(sub=444), b"4:4:4")
    _refused(dec(fs=H * W * 3 // 2 - 1), b"frame_stride_bytes")
    _refused(dec(N=1, fs=H * W), b"frame_stride_bytes")                    # a stride is judged for one frame too
    _refused(dec(C=1, sub=0, fs=H * W - 1), b"frame_stride_bytes")
    for bad in (dict(N=0), dict(N=65536), dict(H=0), dict(W=70000), dict(C=2), dict(sub=422)):
        _refused(dec(**bad), b"bad batch")
    _refused(dec(inp=ctypes.c_void_p(4100)), b"16-byte")
    _refused(dec(in_stride=stride + 8), b"16-byte")
    _refused(dec(in_stride=16), b"in_stride")
    _refused(dec(up=1, in_stride=(blob + 15) & ~15), b"in_stride")             # uploaded coefficients need their room
    _refused(dec(ws=ctypes.c_void_p(4100)), b"workspace must be 16-byte")
    assert dec(wsb=ws - 1) == -3 and b"workspace" in L.stabnet_last_error()


def test_decode_sync_i420_refuses_before_any_launch():
    L = _L()
    one, al = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    H, W = 16, 32
    blob = L.stabnet_mjpeg_decode_blob_bytes(H, W, 3, 420)
    stride = (blob + 4096 + 15) & ~15
    ws = L.stabnet_mjpeg_decode_sync_workspace_bytes(1, H, W, 3, 420, stride, 0)
    dec = lambda **k: L.stabnet_mjpeg_decode_sync_i420(*[k.get(n, d) for n, d in (
        ("inp", al), ("in_stride", stride), ("N", 1), ("H", H), ("W", W), ("C", 3), ("sub", 420), ("out", one), ("fs", H * W * 3 // 2),
        ("status", one), ("ws", al), ("wsb", ws), ("chunk", 0), ("rounds", -1), ("stats", None), ("st", None), ("prof", None))])
    for bad in (dict(inp=None), dict(out=None), dict(status=None), dict(ws=None)):
        _refused(dec(**bad), b"null")
    _refused(dec(H=17), b"odd side")
    _refused(dec(W=31), b"odd side")
    _refused(dec(sub=444), b"4:4:4")
    _refused(dec(fs=H * W * 3 // 2 - 1), b"frame_stride_bytes")
    for bad in (dict(N=0), dict(H=0), dict(C=2), dict(sub=422)):
        _refused(dec(**bad), b"bad batch")
    for bad in (dict(chunk=6), dict(chunk=4100), dict(chunk=4)):
        _refused(dec(**bad), b"chunk_bytes")
    for bad in (dict(rounds=-2), dict(rounds=1025)):
        _refused(dec(**bad), b"rounds")
    _refused(dec(inp=ctypes.c_void_p(4100)), b"16-byte")
    _refused(dec(in_stride=16), b"in_stride")
    assert dec(wsb=ws - 1) == -3 and b"workspace" in L.stabnet_last_error()


def test_encode_i420_refuses_before_any_launch():
    L = _L()
    one, al = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    H, W = 16, 32
    hb = L.stabnet_mjpeg_header(H, W, 3, 420, 1, (ctypes.c_ushort * 64)(*[1] * 64), (ctypes.c_ushort * 64)(*[1] * 64), None, 0)
    hb1 = L.stabnet_mjpeg_header(H, W, 1, 420, 1, (ctypes.c_ushort * 64)(*[1] * 64), None, None, 0)
    mb = L.stabnet_mjpeg_max_bytes(H, W, 3, 420, 1)
    ws = L.stabnet_mjpeg_workspace_bytes(2, H, W, 3, 420, 1)
    enc = lambda **k: L.stabnet_mjpeg_encode_i420(*[k.get(n, d) for n, d in (
        ("src", one), ("N", 2), ("H", H), ("W", W), ("planes", 3), ("fs", H * W * 3 // 2), ("R", 1), ("ql", one), ("qc", one), ("hd", one),
        ("hb", hb), ("out", one), ("stride", mb), ("nb", one), ("ws", al), ("wsb", ws), ("st", None), ("prof", None))])
    for bad in (dict(src=None), dict(out=None), dict(nb=None), dict(ws=None), dict(ql=None), dict(qc=None), dict(hd=None)):
        _refused(enc(**bad), b"null")
    for bad in (dict(planes=0), dict(planes=2), dict(planes=4)):
        _refused(enc(**bad), b"planes must be 1")
    _refused(enc(H=17), b"odd side")
    _refused(enc(W=31), b"odd side")
    _refused(enc(fs=H * W * 3 // 2 - 1), b"frame_stride_bytes")
    _refused(enc(N=1, fs=H * W), b"frame_stride_bytes")
    _refused(enc(planes=1, hb=hb1, fs=H * W - 1), b"frame_stride_bytes")
    for bad in (dict(R=0), dict(R=70000), dict(N=0), dict(H=0), dict(W=-4)):
        _refused(enc(**bad), b"bad batch")
    _refused(enc(stride=mb - 1), b"out_stride")
    _refused(enc(hb=hb + 1), b"header_bytes")
    _refused(enc(ws=ctypes.c_void_p(4100)), b"16-byte")
    assert enc(wsb=ws - 1) == -3 and b"workspace" in L.stabnet_last_error()


def test_python_wrappers_refuse_without_a_device():
    from stabnet_amd import _lib, mjpeg
    assert mjpeg.planar_frame_bytes(18, 34, 3) == 18 * 34 * 3 // 2 and mjpeg.planar_frame_bytes(9, 13, 1) == 9 * 13
    assert mjpeg.planar_refusal(18, 34, 3, 420) is None and mjpeg.planar_refusal(9, 13, 1, 0) is None
    assert "4:4:4" in mjpeg.planar_refusal(18, 34, 3, 444)
    assert "odd width 33" in mjpeg.planar_refusal(18, 33, 3, 420) and "odd height 17" in mjpeg.planar_refusal(17, 34, 3, 420)
    with pytest.raises(mjpeg.Unsupported, match="odd"):
        mjpeg.MjpegDecoder(17, 34, 3, "420", device="cpu", planar=True)
    with pytest.raises(mjpeg.Unsupported, match="4:4:4"):
        mjpeg.MjpegDecoder(18, 34, 3, "444", device="cpu", planar=True)
    with pytest.raises(_lib.StabnetError, match="odd side"):
        mjpeg.MjpegEncoder(17, 34, 3, device="cpu", planar=True)
    with pytest.raises(_lib.StabnetError, match="4:2:0"):
        mjpeg.MjpegEncoder(18, 34, 3, subsampling="444", device="cpu", planar=True)


# ---- refusals of deploy_bundle.py --avi-in that precede the GPU ---------------------------------------------------------------------------
def _jpeg(H, W, **opts):
    from PIL import Image
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(3 * x + y) % 256, (x + 5 * y) % 256, (x * y) % 256], -1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img if opts.pop("colour", True) else img[..., 0].copy()).save(buf, "JPEG", **opts)
    return buf.getvalue()


def _avi(path, jpegs, W, H, fps=25):
    from stabnet_amd.avi import AviMjpegWriter
    with AviMjpegWriter(str(path), W, H, fps) as w:
        for j in jpegs:
            w.write(j)
    return str(path)


def _flag_refusal(argv, capsys):
    import deploy_bundle
    with pytest.raises(SystemExit) as e:
        deploy_bundle.parse_args(argv)
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    msg = err.strip().splitlines()[-1]
    assert msg.startswith("deploy_bundle.py: error: ") or ": error: " in msg
    assert msg.count(": error: ") == 1 and "Traceback" not in err
    return msg


@pytest.mark.parametrize("argv,word", [
    (["--avi-in", "a.avi", "--y4m-in", "b.y4m"], "--y4m-in"),
    (["--avi-in", "a.avi", "--jpeg-subsampling", "444"], "444"),
    (["--avi-in", "a.avi", "--pipeline"], "--pipeline"),
    (["--avi-in", "a.avi", "--score"], "--score"),
    (["--avi-in", "a.avi", "--fill", "auto"], "--fill auto"),
    (["--avi-in", "a.avi", "--fill", "adaptive"], "--fill adaptive"),
    (["--avi-in", "a.avi", "--fill", "history"], "--fill history"),
    (["--avi-in", "a.avi", "--mjpg"], "--mjpg"),
    (["--avi-in", "a.avi", "--synthetic", "5"], "--synthetic"),
    (["--avi-in", "a.avi", "--jpeg-quality", "0"], "--jpeg-quality"),
    (["--avi-in", "a.avi", "--fps", "0"], "--fps"),
    (["--avi-out", "o.avi"], "--avi-out needs --avi-in"),
    (["--y4m-out", "o.y4m"], "--y4m-out needs --y4m-in"),
])
def test_driver_flag_refusals_are_one_sentence_each(capsys, argv, word):
    assert word in _flag_refusal(argv, capsys)


def test_driver_flags_of_the_stream_loop():
    import deploy_bundle
    a = deploy_bundle.parse_args(["--avi-in", "a.avi"])                                     # a dry run
    assert (a.avi_in, a.avi_out, a.y4m_out, a.ingest, a.output_size, a.decode, a.fps_given) == ("a.avi", None, None, "device", "source", "device", False)
    a = deploy_bundle.parse_args(["--avi-in", "a.avi", "--avi-out", "o.avi", "--y4m-out", "-", "--fill", "0.8", "--interp", "cubic", "--scene-cut",
                                  "--entropy", "parallel", "--jpeg-quality", "90", "--fps", "24"])
    assert (a.avi_out, a.y4m_out, a.fill, a.interp, a.scene_cut, a.scene_gap, a.entropy, a.jpeg_quality, a.fps, a.fps_given) \
        == ("o.avi", "-", 0.8, "cubic", 0.35, 8, "parallel", 90, 24.0, True)
    # the other loops are as they were
    a = deploy_bundle.parse_args([])
    assert (a.avi_in, a.avi_out, a.fps, a.decode, a.ingest) == (None, None, 30.0, "host", "host")
    a = deploy_bundle.parse_args(["--y4m-in", "-", "--y4m-out", "-"])
    assert a.avi_in is None and a.y4m_in == "-"


def _probe_refusal(path, **flags):
    import deploy_bundle
    args = deploy_bundle.parse_args(["--avi-in", str(path)] + [str(v) for kv in flags.items() for v in kv])
    with pytest.raises(SystemExit) as e:
        deploy_bundle.main_avi(args)
    msg = e.value.code
    assert isinstance(msg, str) and msg.startswith("deploy_bundle.py: --avi-in: ") and "\n" not in msg and "Traceback" not in msg
    return msg


def test_driver_refuses_files_and_first_frames_before_the_gpu(tmp_path, monkeypatch):
    import deploy_bundle
    monkeypatch.setattr(deploy_bundle, "setup_stream", lambda args: pytest.fail("the GPU was about to be touched"))
    assert "No such file" in _probe_refusal(tmp_path / "missing.avi")
    junk = tmp_path / "junk.avi"
    junk.write_bytes(b"this is not a RIFF file at all, not even close" * 4)
    assert "not a RIFF AVI" in _probe_refusal(junk)
    (tmp_path / "empty.avi").write_bytes(b"")
    assert "not a RIFF AVI" in _probe_refusal(tmp_path / "empty.avi")
    m = _probe_refusal(_avi(tmp_path / "none.avi", [], 32, 16))
    assert "holds no frame" in m
    m = _probe_refusal(_avi(tmp_path / "s422.avi", [_jpeg(16, 32, subsampling="4:2:2")] * 2, 32, 16))
    assert "sampling 21 11 11" in m and "test-list route" in m
    m = _probe_refusal(_avi(tmp_path / "s444.avi", [_jpeg(16, 32, subsampling="4:4:4")] * 2, 32, 16))
    assert "4:4:4" in m and "test-list route" in m
    m = _probe_refusal(_avi(tmp_path / "oddw.avi", [_jpeg(16, 31, subsampling="4:2:0")] * 2, 31, 16))
    assert "4:2:0" in m and "odd width 31" in m and "test-list route" in m
    m = _probe_refusal(_avi(tmp_path / "oddh.avi", [_jpeg(17, 32, subsampling="4:2:0")] * 2, 32, 17))
    assert "odd height 17" in m
    m = _probe_refusal(_avi(tmp_path / "prog.avi", [_jpeg(16, 32, progressive=True)] * 2, 32, 16))
    assert "outside the planar decoder's scope" in m
    m = _probe_refusal(_avi(tmp_path / "cut.avi", [_jpeg(16, 32, subsampling="4:2:0")[:300]] * 2, 32, 16))
    assert "no complete baseline JPEG" in m
    # what the loop takes gets past the probe: an even 4:2:0 clip, and a grey one of odd size
    for name, j, W, H in (("ok.avi", _jpeg(16, 32, subsampling="4:2:0"), 32, 16), ("grey.avi", _jpeg(17, 31, colour=False), 31, 17)):
        args = deploy_bundle.parse_args(["--avi-in", _avi(tmp_path / name, [j] * 2, W, H)])
        rd, info = deploy_bundle.avi_probe(args)
        assert (info["H"], info["W"], len(rd), rd.rate, rd.scale) == (H, W, 2, 25, 1)


def test_driver_refusal_in_a_process_of_its_own(tmp_path):
    """The whole program: one sentence on stderr, a non-zero exit, no traceback, nothing on stdout, no output file."""
    path = _avi(tmp_path / "s422.avi", [_jpeg(16, 32, subsampling="4:2:2")] * 3, 32, 16)
    out = tmp_path / "o.avi"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "deploy_bundle.py"), "--avi-in", path, "--avi-out", str(out), "--y4m-out", "-"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == ""
    assert "Traceback" not in r.stderr and "sampling 21 11 11" in r.stderr and "test-list route" in r.stderr
    assert r.stderr.strip().splitlines()[-1].startswith("deploy_bundle.py: --avi-in: ")
    assert not out.exists() and not (tmp_path / "o.avi.json").exists()
