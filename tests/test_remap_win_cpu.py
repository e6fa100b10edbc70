"""CPU: the arithmetic of the remap through a window without a GPU.  The NumPy model (tests/remap_win_model.py) with the whole-frame
window is the source-resolution model (tests/remap_src_model.py) bit for bit, and with an integer window at zoom 1 a slice of it; the
two window helpers on hand-computed cases; the entry point's refusals come before the first launch; the driver's --fill option."""
import math
import os
import sys

import numpy as np
import pytest

import remap_src_model as M
import remap_win_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda s: "%dx%d-%dx%d" % s
SHIFTS = [0.0, 0.45, -0.45]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _inputs(shape, shift):
    H, W, SH, SW = shape
    src = np.random.default_rng(SH * 11 + SW).integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    xm, ym = M.mesh_maps(H, W, seed=H + SW, shift=shift)
    return src, xm, ym


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_whole_frame_window_is_the_source_model(shape, shift):
    H, W, SH, SW = shape
    src, xm, ym = _inputs(shape, shift)
    want, px, py, blk = M.warp_src(src, xm, ym)
    got, gx, gy, gb = WM.warp_win(src, xm, ym, (0, 0, SH, SW))
    assert np.array_equal(_bits(gx), _bits(px)) and np.array_equal(_bits(gy), _bits(py))
    assert np.array_equal(got, want) and np.array_equal(gb, blk)
    if shift:
        assert blk.mean() > 0.1


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_integer_window_at_zoom_one_is_the_slice(shape, shift):
    H, W, SH, SW = shape
    src, xm, ym = _inputs(shape, shift)
    want, px, py, blk = M.warp_src(src, xm, ym)
    for y0, x0, OH, OW in ((0, 0, SH, SW), (3, 5, SH - 7, SW - 9), (SH - 4, SW - 6, 4, 6), (0, SW // 2, SH // 2, SW - SW // 2)):
        got, gx, gy, gb = WM.warp_win(src, xm, ym, (y0, x0, OH, OW), (OH, OW))
        sl = np.s_[y0:y0 + OH, x0:x0 + OW]
        assert np.array_equal(_bits(gx), _bits(px[sl])) and np.array_equal(_bits(gy), _bits(py[sl])), (y0, x0, OH, OW)
        assert np.array_equal(got, want[sl]) and np.array_equal(gb, blk[sl]), (y0, x0, OH, OW)


def test_zoom_keeps_the_middle_of_the_window_in_the_middle():
    """Identity maps, a 2x zoom on a smooth ramp: the output's centre is the window's centre, and a grey source keeps its shape."""
    H, W, SH, SW = 32, 64, 64, 128
    xm, ym = M.identity_maps(H, W)
    ramp = np.broadcast_to((np.arange(SW) * 2).astype(np.uint8)[None, :], (SH, SW)).copy()
    out, px, py, blk = WM.warp_win(ramp, xm, ym, (16, 32, 32, 64), (64, 128))
    assert out.shape == (64, 128) and not blk.any()
    # output pixel j sits at source position 32 + (j + 0.5) / 2 - 0.5
    assert np.abs(px[32] - (32 + (np.arange(128) + 0.5) / 2 - 0.5)).max() < 1e-3


def test_ratio_window():
    from stabnet_amd.warp import ratio_window
    assert ratio_window(1080, 1920, 1.0) == (0.0, 0.0, 1080.0, 1920.0)
    assert ratio_window(77, 131, 1) == (0.0, 0.0, 77.0, 131.0)
    assert ratio_window(100, 200, 0.5) == (25.0, 50.0, 50.0, 100.0)
    y0, x0, wh, ww = ratio_window(77, 131, 0.8)
    assert (wh, ww) == (77 * 0.8, 131 * 0.8) and y0 == (77 - wh) / 2 and x0 == (131 - ww) / 2
    assert math.isclose(y0, 7.7, rel_tol=1e-12) and math.isclose(x0, 13.1, rel_tol=1e-12)
    for SH, SW in ((77, 131), (1080, 1920), (9, 8)):
        for r in (0.1, 0.3, 0.8, 0.95, 1.0):
            y0, x0, wh, ww = ratio_window(SH, SW, r)
            assert y0 >= -1e-9 and x0 >= -1e-9 and y0 + wh <= SH + 1e-9 and x0 + ww <= SW + 1e-9
            assert math.isclose(y0 + wh / 2, SH / 2) and math.isclose(x0 + ww / 2, SW / 2)
    for bad in (0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            ratio_window(77, 131, bad)


def test_fit_window_hand_computed():
    from stabnet_amd.warp import fit_window
    assert fit_window((10, 20, 49, 119), 77, 131) == (10.0, 35.974025974025977, 40.0, 68.051948051948045)
    assert fit_window((0, 0, 76, 130), 77, 131) == (0, 0, 77, 131)
    assert fit_window((5, 5, 70, 40), 1080, 1920) == (27.875, 5.0, 20.25, 36.0)
    assert all(type(v) is float for v in fit_window([0, 0, 76, 130], 77, 131))


def test_fit_window_lies_inside_its_rectangle_with_the_outputs_aspect():
    from stabnet_amd.warp import fit_window
    rng = np.random.default_rng(3)
    for _ in range(200):
        i0, j0 = (int(v) for v in rng.integers(0, 50, 2))
        rh, rw = (int(v) for v in rng.integers(1, 400, 2))
        OH, OW = (int(v) for v in rng.integers(1, 2000, 2))
        y0, x0, wh, ww = fit_window((i0, j0, i0 + rh - 1, j0 + rw - 1), OH, OW)
        assert y0 >= i0 and x0 >= j0 and y0 + wh <= i0 + rh + 1e-9 and x0 + ww <= j0 + rw + 1e-9
        assert wh > 0 and ww > 0 and math.isclose(ww * OH, wh * OW, rel_tol=1e-12)
        assert wh == rh or ww == rw                                             # the largest one: one side of the rectangle binds
        assert math.isclose(y0 + wh / 2, i0 + rh / 2) and math.isclose(x0 + ww / 2, j0 + rw / 2)


def test_argument_errors_need_no_gpu():
    """Every refusal comes before the first launch, so it can be asked for without a device."""
    import ctypes
    from stabnet_amd import _lib
    L = _lib.lib()
    assert L.stabnet_abi_version() >= 3
    p = 4096                                                  # stands for a pointer: never dereferenced on these paths
    win = lambda *v: (ctypes.c_double * 4)(*v)
    call = lambda **kw: L.stabnet_warp_rev_bundle2_win(*[kw.get(k, v) for k, v in (
        ("src", p), ("N", 1), ("SH", 77), ("SW", 131), ("C", 3), ("stride", 393), ("x_map", p), ("y_map", p), ("H", 32), ("W", 64), ("rate", 4),
        ("window", win(0, 0, 77, 131)), ("OH", 60), ("OW", 96), ("out", p), ("black", 0), ("ws", p), ("px", 0), ("py", 0), ("stream", 0),
        ("prof", 0))])
    inf, nan = float("inf"), float("nan")
    for bad in (dict(src=0), dict(x_map=0), dict(y_map=0), dict(out=0), dict(ws=0), dict(C=0), dict(C=2), dict(C=4), dict(N=0), dict(SH=0),
                dict(SW=0), dict(SH=32768), dict(SW=32768, stride=3 * 32768), dict(H=3), dict(W=3), dict(rate=0), dict(rate=33),
                dict(stride=392), dict(px=p), dict(py=p),
                dict(OH=0), dict(OW=0), dict(OH=32768), dict(OW=32768), dict(OH=-1), dict(window=None),
                dict(window=win(nan, 0, 77, 131)), dict(window=win(0, inf, 77, 131)), dict(window=win(0, 0, nan, 131)),
                dict(window=win(0, 0, 77, -inf)), dict(window=win(0, 0, 0, 131)), dict(window=win(0, 0, 77, 0)),
                dict(window=win(0, 0, -5, 131)), dict(window=win(-1e-5, 0, 77, 131)), dict(window=win(0, -1e-5, 77, 131)),
                dict(window=win(0, 0, 77.00001, 131)), dict(window=win(0, 0, 77, 131.00001)), dict(window=win(40, 0, 40, 131)),
                dict(window=win(0, 100, 77, 40))):
        assert call(**bad) == -1, bad
        assert b"warp_rev_bundle2_win" in L.stabnet_last_error()


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from stabnet_amd import _lib, warp
    m = torch.zeros((1, 32, 64))
    for bad in (torch.zeros((1, 45, 77, 3), dtype=torch.uint8), np.zeros((45, 77, 3), np.uint8)):
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_win(bad, m, m, (0, 0, 45, 77))


def test_fill_option():
    sys.path.insert(0, ROOT)
    import deploy_bundle
    assert deploy_bundle.build_parser().parse_args([]).fill is None
    assert deploy_bundle.parse_args([]).fill is None
    assert deploy_bundle.parse_args(["--ingest", "device", "--fill", "0.8"]).fill == 0.8
    assert deploy_bundle.parse_args(["--ingest", "device", "--fill", "1"]).fill == 1.0
    assert deploy_bundle.parse_args(["--ingest", "device", "--fill", "auto"]).fill == "auto"
    assert deploy_bundle.parse_args(["--ingest", "device", "--output-size", "source", "--fill", "0.8", "--pipeline"]).fill == 0.8
    for bad in (["--fill", "0.8"], ["--fill", "auto"], ["--ingest", "host", "--fill", "0.8"],
                ["--ingest", "device", "--fill", "0"], ["--ingest", "device", "--fill", "-0.5"], ["--ingest", "device", "--fill", "1.01"],
                ["--ingest", "device", "--fill", "nan"], ["--ingest", "device", "--fill", "full"], ["--ingest", "device", "--fill", "Auto"]):
        with pytest.raises(SystemExit):
            deploy_bundle.parse_args(bad)
