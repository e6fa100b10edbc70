"""CPU: the arithmetic of the remap at source resolution without a GPU.  The NumPy model (tests/remap_src_model.py) at the network's
own size is the oracle's warpRevBundle2 bit for bit; with identity maps it hands the source frame back away from the border; the
entry point's refusals come before the first launch, the Python layer's before the library is asked."""
import math
import os
import sys

import numpy as np
import pytest

import remap_src_model as M
from oracle import stabnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda s: "%dx%d-%dx%d" % s


def test_constants_at_equal_size_are_one_and_zero():
    assert M.constants(288, 512, 288, 512) == (1.0, 0.0, 1.0, 0.0)
    sx, cx, sy, cy = M.constants(288, 512, 1080, 1920)
    assert (sx, cx, sy, cy) == (np.float32(3.75), np.float32(1.375), np.float32(3.75), np.float32(1.375))


SIZES = sorted({s[:2] for s in M.SHAPES} | {s[2:] for s in M.SHAPES})        # every size of the table, as network and source at once


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_same_size_is_the_oracles_warp_rev_bundle2(size):
    """SH, SW == H, W: sx = 1, cx = 0 -- output, px and py are O.warpRevBundle2's bits."""
    H, W = size
    img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for shift in (0.0, 0.45):
        xm, ym = M.mesh_maps(H, W, seed=H, shift=shift)
        want, xs, ys = O.warpRevBundle2(img, xm, ym)
        got, px, py, blk = M.warp_src(img, xm, ym)
        assert np.array_equal(px.view(np.int32), xs.view(np.int32)) and np.array_equal(py.view(np.int32), ys.view(np.int32))
        assert np.array_equal(got, want)
        # a pixel the rule calls black reads at least one tap outside the frame; away from the frame's last row / column it is 0
        far = blk & ((xs < -1) | (xs > W) | (ys < -1) | (ys > H))
        assert (got[far] == 0).all()


@pytest.mark.parametrize("shape", M.SHAPES + [M.BIG], ids=ids)
def test_identity_maps_give_the_source_back_inside_the_margin(shape):
    H, W, SH, SW = shape
    src = np.random.default_rng(SH * 7 + SW).integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    xm, ym = M.identity_maps(H, W)
    out, px, py, blk = M.warp_src(src, xm, ym)
    my, mx = math.ceil(4 * SH / H) + 1, math.ceil(4 * SW / W) + 1
    assert SH > 2 * my and SW > 2 * mx
    assert np.array_equal(out[my:SH - my, mx:SW - mx], src[my:SH - my, mx:SW - mx])
    assert not blk[my:SH - my, mx:SW - mx].any()


def test_without_the_offset_an_identity_mesh_shifts_the_picture():
    """Why cx exists: px = ux * sx alone lands 0.5 * (SW / W - 1) source pixels off."""
    H, W, SH, SW = 32, 64, 96, 192
    xm, ym = M.identity_maps(H, W)
    px, _ = M.coords(xm, ym, SH, SW)
    sx, cx, _, _ = M.constants(H, W, SH, SW)
    mid = px[SH // 2, 20:SW - 20]
    assert np.abs(mid - np.arange(20, SW - 20)).max() < 1e-3
    assert np.abs((mid - cx) - np.arange(20, SW - 20)).max() == pytest.approx(0.5 * (SW / W - 1), abs=1e-3)


def test_coverage_rule():
    SH, SW = 5, 7
    px = np.array([[0.0, -1 / 64, -1 / 32, SW - 1, SW - 1 + 1 / 64, SW - 1 + 1 / 32, np.nan, 1e30, -1e30]], np.float32)
    py = np.zeros_like(px)
    # -1/64 px = -0.5 in 1/32 px rounds (half to even) to 0: still inside; SW - 1 + 1/64 rounds to 32 * (SW - 1): inside
    assert M.black(px, py, SH, SW).tolist() == [[False, False, True, False, False, True, True, True, True]]
    assert M.black(py, px, SW, SH).tolist() == [[False, False, True, False, False, True, True, True, True]]


def test_argument_errors_need_no_gpu():
    """Every refusal comes before the first launch, so it can be asked for without a device."""
    from stabnet_amd import _lib
    L = _lib.lib()
    p = 4096                                                  # stands for a pointer: never dereferenced on these paths
    call = lambda **kw: L.stabnet_warp_rev_bundle2_src(*[kw.get(k, v) for k, v in (
        ("src", p), ("N", 1), ("SH", 77), ("SW", 131), ("C", 3), ("stride", 393), ("x_map", p), ("y_map", p), ("H", 32), ("W", 64), ("rate", 4),
        ("out", p), ("black", 0), ("ws", p), ("px", 0), ("py", 0), ("stream", 0), ("prof", 0))])
    for bad in (dict(src=0), dict(x_map=0), dict(y_map=0), dict(out=0), dict(ws=0), dict(C=0), dict(C=2), dict(C=4), dict(N=0), dict(SH=0),
                dict(SW=0), dict(SH=32768), dict(SW=32768, stride=3 * 32768), dict(H=3), dict(W=3), dict(rate=0), dict(rate=33),
                dict(stride=392), dict(px=p), dict(py=p)):
        assert call(**bad) == -1, bad
        assert b"warp_rev_bundle2_src" in L.stabnet_last_error()


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from stabnet_amd import _lib, warp
    m = torch.zeros((1, 32, 64))
    for bad in (torch.zeros((1, 45, 77, 3), dtype=torch.uint8), np.zeros((45, 77, 3), np.uint8)):
        with pytest.raises(_lib.StabnetError):
            warp.warpRevBundle2_src(bad, m, m)


def test_output_size_option():
    sys.path.insert(0, ROOT)
    import deploy_bundle
    P = deploy_bundle.build_parser()
    assert P.parse_args([]).output_size == "network"
    assert deploy_bundle.parse_args(["--ingest", "device", "--output-size", "source"]).output_size == "source"
    with pytest.raises(SystemExit):
        deploy_bundle.parse_args(["--output-size", "source"])                        # needs --ingest device
    with pytest.raises(SystemExit):
        P.parse_args(["--output-size", "huge"])
