"""CPU: the frame-ingest arithmetic without a GPU.  The NumPy model (tests/ingest_model.py) is pinned by the installed Pillow, the
library's host tap builders by the model, the cv2 restatement by known answers and by float64 bilinear."""
import ctypes
import os
import sys

import numpy as np
import pytest
from PIL import Image  # noqa: F401  (the reference's resize IS Pillow's: it must be there)

import ingest_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", M.CPU_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_model_resize_equals_pillow(shape):
    sh, sw, H, W = shape
    g = np.random.default_rng(sh * 31 + sw).integers(0, 256, (sh, sw), dtype=np.uint8)
    assert int((M.pil_resize(g, H, W) != M.real_pil_resize(g, H, W)).sum()) == 0


def test_model_crop_window_equals_pillow_resize_then_crop():
    g = np.random.default_rng(5).integers(0, 256, (80, 120), dtype=np.uint8)
    rh, rw, dy, dx = M.geometry(64, 96, 0.9)
    assert (rh, rw, dy, dx) == (71, 106, 3, 5)
    got = M.pil_resize(g, rh, rw, dy, dx, 64, 96)
    assert got.shape == (64, 96) and np.array_equal(got, M.real_pil_resize(g, rh, rw, dy, dx, 64, 96))


def _axes():
    s = set()
    for sh, sw, H, W in M.CPU_SHAPES:
        s.add((sh, H)); s.add((sw, W))
    return sorted(s | {(80, 71), (120, 106), (1, 1), (1, 5), (5, 1), (20000, 1)})


@pytest.mark.parametrize("axis", _axes(), ids=lambda a: "%d-%d" % a)
def test_library_tap_tables_equal_the_model(axis):
    from stabnet_amd import ingest
    n_in, n_out = axis
    ks, b, k = ingest.pil_taps(n_in, n_out)
    mks, mb, mk = M.pil_taps(n_in, n_out)
    assert ks == mks and np.array_equal(b, mb) and np.array_equal(k, mk)
    assert np.abs(k.sum(1) - (1 << 22)).max() <= ks                   # each coefficient is rounded on its own
    o, c = ingest.cv_taps(n_in, n_out)
    mo, mc = M.cv_taps(n_in, n_out)
    assert np.array_equal(o, mo) and np.array_equal(c, mc) and c.dtype == np.int16
    assert np.all(c.astype(int).sum(1) == 2048)


def test_tap_table_size_query_and_errors():
    from stabnet_amd import _lib
    L = _lib.lib()
    ks = ctypes.c_int()
    assert L.stabnet_ingest_pil_taps(1280, 512, ctypes.byref(ks), None, None, 0) == 512 * 7 and ks.value == 7
    assert L.stabnet_ingest_pil_taps(512, 32, None, None, None, 0) == 32 * 33
    assert L.stabnet_ingest_pil_taps(0, 4, None, None, None, 0) == -1
    b, k = np.zeros((4, 2), np.int32), np.zeros((4, 3), np.int32)
    assert L.stabnet_ingest_pil_taps(4, 4, None, b.ctypes.data, k.ctypes.data, 11) == -1 and b"cap" in L.stabnet_last_error()
    assert L.stabnet_ingest_pil_taps(4, 4, None, b.ctypes.data, None, 12) == -1
    assert L.stabnet_ingest_cv_taps(4, 0, b.ctypes.data, k.ctypes.data) == -1
    assert L.stabnet_ingest_cv_taps(4, 4, None, None) == -1
    assert L.stabnet_ingest_workspace_bytes(1, 720, 1280, 3, 288, 512, 288, 512) >= (720 * 512)
    assert L.stabnet_ingest_workspace_bytes(1, 720, 1280, 2, 288, 512, 288, 512) == 0
    assert L.stabnet_ingest_workspace_bytes(1, 80, 120, 3, 71, 106, 72, 96) == 0          # window taller than the resize target


def test_argument_errors_need_no_gpu():
    """Every refusal comes before the first launch, so it can be asked for without a device."""
    from stabnet_amd import _lib
    L = _lib.lib()
    p = 4096                                                  # stands for a pointer: never dereferenced on these paths
    grey = lambda **kw: L.stabnet_ingest_grey(*[kw.get(k, v) for k, v in (
        ("img", p), ("N", 1), ("sh", 45), ("sw", 77), ("C", 3), ("stride", 231), ("wb", 1868), ("wg", 9617), ("wr", 4899), ("shift", 14),
        ("rh", 32), ("rw", 48), ("dy", 0), ("dx", 0), ("H", 32), ("W", 48), ("xb", p), ("xk", p), ("xks", 5), ("yb", p), ("yk", p), ("yks", 5),
        ("lut", p), ("out", p), ("ws", p), ("wsb", 1 << 20), ("stream", 0), ("prof", 0))])
    for bad in (dict(img=0), dict(out=0), dict(lut=0), dict(ws=0), dict(xb=0), dict(yk=0), dict(N=0), dict(H=0), dict(sw=0), dict(C=2), dict(C=4),
                dict(stride=230), dict(dy=1), dict(dx=1), dict(H=33), dict(xks=7), dict(shift=0), dict(wb=1 << 14)):
        assert grey(**bad) == -1, bad
    assert grey(wsb=45 * 48 - 1) == -3 and b"workspace" in L.stabnet_last_error()
    # a tap count over the kernel's bound (8193 horizontal taps = a 4096x downscale)
    assert grey(sh=1, sw=20000, C=1, stride=20000, rh=1, rw=1, H=1, W=1, xks=40001) == -1 and b"taps" in L.stabnet_last_error()
    col = lambda **kw: L.stabnet_ingest_colour(*[kw.get(k, v) for k, v in (
        ("img", p), ("N", 1), ("sh", 45), ("sw", 77), ("C", 3), ("stride", 231), ("H", 32), ("W", 48), ("xo", p), ("xc", p), ("yo", p),
        ("yc", p), ("out", p), ("stream", 0), ("prof", 0))])
    for bad in (dict(img=0), dict(out=0), dict(xo=0), dict(yc=0), dict(C=1), dict(N=0), dict(W=0), dict(stride=100)):
        assert col(**bad) == -1, bad


def test_lookup_table_is_the_float64_expression():
    from stabnet_amd import ingest
    lut = ingest.lut256()
    assert lut.dtype == np.float32 and lut.shape == (256,)
    for u in range(256):
        assert lut[u] == np.float32(float(u) * (1. / 255) - 0.5)
    assert np.array_equal(lut, M.lut256()) and np.array_equal(M.train_from_u8(np.arange(256, dtype=np.uint8)), lut)
    # (why a table: the same expression evaluated in float32 is a different number for some u)
    f32 = np.arange(256, dtype=np.float32) * np.float32(1. / 255) - np.float32(0.5)
    assert (f32 != lut).any()


def test_grey_weights():
    from stabnet_amd import ingest
    assert ingest.GRAY_WEIGHTS == M.GRAY_WEIGHTS
    for name, (wb, wg, wr, s) in M.GRAY_WEIGHTS.items():
        assert wb + wg + wr == 1 << s
        assert M.grey_u8(np.full((2, 2, 3), 255, np.uint8), name).tolist() == [[255, 255], [255, 255]]
        assert M.grey_u8(np.zeros((2, 2, 3), np.uint8), name).max() == 0
    # blue, green, red on their own: round(255 * 0.114 / 0.587 / 0.299)
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)
    assert M.grey_u8(px, "cv3").tolist() == [[29, 150, 76]] and M.grey_u8(px, "cv4").tolist() == [[29, 150, 76]]
    assert M.grey_u8(px[..., :1]).shape == (1, 3)                      # one channel passes through


def test_cv_model_known_answers():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(M.cv_resize(img, 64, 96), img)                                   # equal size is a copy
    for sh, sw, H, W in M.CPU_SHAPES:
        assert np.all(M.cv_resize(np.full((sh, sw, 3), 201, np.uint8), H, W) == 201)       # a constant stays constant
    v = img.astype(np.int64)
    box = (v[0::2, 0::2] + v[1::2, 0::2] + v[0::2, 1::2] + v[1::2, 1::2] + 2) >> 2
    assert np.array_equal(M.cv_resize(img, 32, 48), box)                                   # exact 2x = the rounded box mean


@pytest.mark.parametrize("shape", M.CPU_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_cv_model_stays_within_one_level_of_float64_bilinear(shape):
    sh, sw, H, W = shape
    img = np.random.default_rng(sh + 7 * sw).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    d = np.abs(M.cv_resize(img, H, W).astype(np.float64) - M.bilinear_f64(img, H, W)).max()
    print("cv model vs float64 bilinear %s: %.3f grey levels" % (shape, d))
    assert d < 1.0


def test_bilinear_f64_is_torch_interpolate():
    import torch
    img = np.random.default_rng(3).integers(0, 256, (45, 77, 3), dtype=np.uint8)
    t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    ref = torch.nn.functional.interpolate(t, size=(32, 48), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    assert np.abs(M.bilinear_f64(img, 32, 48) - ref).max() < 1e-9


def test_ingest_option_defaults_to_host():
    sys.path.insert(0, ROOT)
    import deploy_bundle
    a = deploy_bundle.build_parser().parse_args([])
    assert a.ingest == "host" and a.gray_weights == "cv3"
    a = deploy_bundle.build_parser().parse_args(["--ingest", "device", "--gray-weights", "cv4"])
    assert a.ingest == "device" and a.gray_weights == "cv4"
    with pytest.raises(SystemExit):
        deploy_bundle.build_parser().parse_args(["--ingest", "gpu"])


def test_frame_ingest_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from stabnet_amd import _lib, ingest
    with pytest.raises(_lib.StabnetError):
        ingest.FrameIngest(45, 77, 2, 32, 48, device="cpu")
    with pytest.raises(_lib.StabnetError):
        ingest.FrameIngest(45, 77, 3, 32, 48, gray="cv5", device="cpu")
    with pytest.raises(_lib.StabnetError):
        ingest.FrameIngest(45, 77, 3, 0, 48, device="cpu")
    ing = ingest.FrameIngest(45, 77, 3, 32, 48, device="cpu")          # tables only: nothing is launched by the constructor
    assert (ing.rh, ing.rw, ing.dy, ing.dx) == (32, 48, 0, 0)
    assert (lambda i: (i.rh, i.rw, i.dy, i.dx))(ingest.FrameIngest(80, 120, 3, 64, 96, crop_rate=0.9, device="cpu")) == (71, 106, 3, 5)
    for bad in (torch.zeros((1, 45, 77, 3), dtype=torch.uint8), np.zeros((1, 45, 77, 3), np.uint8)):
        with pytest.raises(_lib.StabnetError):
            ing.grey(bad)
        with pytest.raises(_lib.StabnetError):
            ing.colour(bad)
