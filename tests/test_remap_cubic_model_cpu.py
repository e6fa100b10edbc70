"""CPU: tests/remap_cubic_model.py, the NumPy yardstick of the bicubic remap (csrc/remap.hip, --interp cubic): the facts of OpenCV's
fixed-point bicubic table, the host table builder of the library against it, properties of the blend that follow from the algorithm
alone, the input condition the GPU tests rely on (every one of the 1024 phases occurs), the refusals of the C entries and the driver's
flag.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import remap_cubic_model as CM
import remap_src_model as M
from oracle import stabnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_table_facts():
    t = CM.table().astype(np.int64)
    diffs = CM.repaired_diffs()
    assert t.shape == (1024, 16) and CM.table().dtype == np.int16
    assert len(diffs) == 657 and min(diffs) == -2 and max(diffs) == 4
    assert (t.sum(axis=1) == 32768).all()
    e00 = np.zeros(16, np.int64)
    e00[5], e00[10] = 32767, 1                               # tap [1][1] saturated, the missing 1 on tap [2][2]
    assert np.array_equal(t[0], e00)
    assert t[16 * 32 + 16].tolist() == [288, -1824, -1824, 288, -1824, 11552, 11552, -1824, -1824, 11552, 11552, -1824, 288, -1824, -1824, 288]
    assert t.min() == -3638
    assert np.abs(t).sum(axis=1).max() == 61952              # times 255: far inside int32


def test_host_builder_and_golden_equal_the_model():
    from stabnet_amd import _lib
    got = np.full((1024, 16), 0x5A5A, np.int16)
    assert _lib.lib().stabnet_remap_cubic_table(got.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(got, CM.table())                   # all 16384 values
    golden = np.load(os.path.join(ROOT, "tests", "golden", "remap_cubic_tab.npy"))
    assert golden.dtype == np.int16 and np.array_equal(golden, CM.table())
    assert _lib.lib().stabnet_remap_cubic_table(None) == -1 and b"null" in _lib.lib().stabnet_last_error()


def test_integer_coordinates_reproduce_the_source():
    img = np.random.default_rng(0).integers(0, 256, (13, 17, 3), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(13, dtype=F), np.arange(17, dtype=F), indexing="ij")
    out = CM.cv_remap_cubic_u8(img, xx, yy)
    # phase (0, 0) is {[1][1]: 32767, [2][2]: 1}: (32767 v + v' + 16384) >> 15 == v for every byte v, v'
    assert np.array_equal(out[1:-2, 1:-2], img[1:-2, 1:-2])
    # and shifted by whole pixels
    out = CM.cv_remap_cubic_u8(img, xx + F(2), yy + F(1))
    assert np.array_equal(out[1:-4, 1:-5], img[2:-3, 3:-3])


def test_constant_image_stays_constant_at_every_phase():
    for v in (0, 1, 77, 254, 255):
        img = np.full((8, 8, 1), v, np.uint8)
        f = np.arange(32, dtype=F) / F(32)
        px, py = np.meshgrid(F(3) + f, F(3) + f)              # all 1024 phases, taps 2 .. 5: inside
        assert CM.taps_inside(px, py, 8, 8).all()
        assert (CM.cv_remap_cubic_u8(img, px, py) == v).all()
    # with a border value a frame-sized constant stays constant everywhere: the weights sum to 32768
    px, py = np.meshgrid(np.linspace(-3, 10, 57).astype(F), np.linspace(-3, 10, 57).astype(F))
    assert (CM.cv_remap_cubic_u8(np.full((8, 8, 1), 128, np.uint8), px, py, border=128) == 128).all()


def test_cubic_keeps_more_of_a_fine_stripe_pattern_than_linear():
    """One-pixel-wide stripes (one bright column in four) shifted by half a pixel.  Per period bilinear gives (A/2, A/2, 0, 0) over the
    background and bicubic (19/32 A, 19/32 A, -3/32 A, -3/32 A): the same mean, deviations A/4 against 11/32 A, a variance ratio of
    (11/8)^2 = 1.89 before rounding to bytes.  No value clamps (56 - 3/32 * 144 > 0)."""
    img = np.full((16, 64, 1), 56, np.uint8)
    img[:, ::4] = 200
    yy, xx = np.meshgrid(np.arange(16, dtype=F), np.arange(64, dtype=F), indexing="ij")
    half = xx + F(0.5)
    lin = O.cv_remap_linear_u8(img, half, yy)[2:-3, 4:-4].astype(np.float64)
    cub = CM.cv_remap_cubic_u8(img, half, yy)[2:-3, 4:-4].astype(np.float64)
    assert abs(cub.mean() - lin.mean()) <= 0.5 and lin.var() > 0           # (each byte is rounded by at most a half)
    assert cub.var() > 1.8 * lin.var()
    # (alternating columns, period 2, are the degenerate case: at half a pixel both kernels average the two values exactly)
    img[:, ::2], img[:, 1::2] = 200, 56
    assert CM.cv_remap_cubic_u8(img, half, yy)[2:-3, 4:-4].var() == 0 == O.cv_remap_linear_u8(img, half, yy)[2:-3, 4:-4].var()


def test_border_zero_equals_opencv_cval_form():
    """sum(v w) with the border value in place of outside taps == cval * ONE + sum((S - cval) w) over the inside taps."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (6, 7, 1), dtype=np.uint8)
    px = rng.uniform(-3, 9, (40, 40)).astype(F)
    py = rng.uniform(-3, 8, (40, 40)).astype(F)
    ix, iy, fx, fy = CM.quantise(px, py)
    w = CM.table()[fy * 32 + fx].astype(np.int64)
    for cval in (0, 16, 128):
        acc = np.full(px.shape, cval * 32768, np.int64)
        for k1 in range(4):
            for k2 in range(4):
                yy, xx = iy - 1 + k1, ix - 1 + k2
                ok = (xx >= 0) & (xx < 7) & (yy >= 0) & (yy < 6)
                v = img[np.clip(yy, 0, 5), np.clip(xx, 0, 6), 0].astype(np.int64)
                acc += np.where(ok, (v - cval) * w[..., k1 * 4 + k2], 0)
        want = np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)
        assert np.array_equal(CM.cv_remap_cubic_u8(img, px, py, border=cval)[..., 0], want)


def test_gpu_test_inputs_hit_every_phase_and_the_clamp():
    seen = np.zeros(1024, bool)
    for k, (H, W, SH, SW) in enumerate(M.SHAPES):
        xm, ym = M.mesh_maps(H, W, seed=k)
        px, py = M.coords(xm, ym, SH, SW)
        ix, iy, fx, fy = CM.quantise(px, py)
        inside = ~M.black(px, py, SH, SW)
        seen[(fy * 32 + fx)[inside]] = True
    assert seen.all()


def test_coordinates_and_coverage_are_the_linear_model_s():
    H, W, SH, SW = M.SHAPES[2]
    src = np.random.default_rng(1).integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    xm, ym = M.mesh_maps(H, W, seed=2, shift=0.3)
    _, px, py, blk = CM.warp_src(src, xm, ym)
    _, lx, ly, lblk = M.warp_src(src, xm, ym)
    assert np.array_equal(px.view(np.int32), lx.view(np.int32)) and np.array_equal(py.view(np.int32), ly.view(np.int32))
    assert np.array_equal(blk, lblk)


def _cubic(**bad):
    from stabnet_amd import _lib
    good = dict(src=1, N=1, SH=8, SW=8, C=3, stride=24, x_map=1, y_map=1, H=8, W=8, rate=4, kind=0, window=None, OH=8, OW=8, out=1, black=0,
                ws=1, px=0, py=0, stream=0, prof=0)
    L = _lib.lib()
    rc = L.stabnet_warp_rev_bundle2_cubic(*dict(good, **bad).values())
    return rc, L.stabnet_last_error().decode()


def _i420(**bad):
    from stabnet_amd import _lib
    good = dict(src=1, N=1, SH=8, SW=8, planes=3, stride=96, x_map=1, y_map=1, H=8, W=8, rate=4, window=None, OH=8, OW=8, border_y=0, out=1,
                black=0, ws=1, stream=0, prof=0)
    L = _lib.lib()
    rc = L.stabnet_warp_rev_bundle2_i420_cubic(*dict(good, **bad).values())
    return rc, L.stabnet_last_error().decode()


def test_entries_refuse_without_a_gpu():
    """Every refusal comes before anything touches the device (the pointers here are not even valid)."""
    for bad, text in ((dict(src=0), "null pointer"), (dict(out=0), "null pointer"), (dict(ws=0), "null pointer"), (dict(x_map=0), "null pointer"),
                      (dict(C=2), "C must be 1"), (dict(kind=3), "window_kind"), (dict(kind=-1), "window_kind"),
                      (dict(OH=7), "window_kind 0 is the whole frame"), (dict(OW=9), "window_kind 0 is the whole frame"),
                      (dict(kind=1), "null window"), (dict(kind=2), "null window"), (dict(stride=23), "row stride"),
                      (dict(px=1), "px_out and py_out"), (dict(N=0), "batch"), (dict(SH=32768), "outside 1..32767")):
        rc, msg = _cubic(**bad)
        assert rc == -1 and msg.startswith("warp_rev_bundle2_cubic:") and text in msg, (bad, msg)
    win = (ctypes.c_double * 4)(0.0, 0.0, 9.0, 8.0)
    rc, msg = _cubic(kind=1, window=win)
    assert rc == -1 and "leaves the 8x8 frame" in msg
    for bad, text in ((dict(src=0), "null pointer"), (dict(planes=2), "planes must be 1"), (dict(SH=7, OH=7), "even sides"), (dict(OW=6, window=win), "leaves"),
                      (dict(OW=7, window=win), "even sides"), (dict(border_y=256), "border_y 256"), (dict(border_y=-1), "border_y"),
                      (dict(stride=95), "frame stride"), (dict(OH=6), "null window")):
        rc, msg = _i420(**bad)
        assert rc == -1 and msg.startswith("warp_rev_bundle2_i420_cubic:") and text in msg, (bad, msg)
    from stabnet_amd import _lib
    assert _lib.lib().stabnet_remap_cubic_weights_dev(None, None) == -1


def test_python_layer_refuses_an_unknown_interp_before_anything_else():
    from stabnet_amd import _lib, warp
    for fn, nargs in ((warp.warpRevBundle2, 3), (warp.warpRevBundle2_src, 3), (warp.warpRevBundle2_win, 4), (warp.warpRevBundle2_i420, 4)):
        with pytest.raises(_lib.StabnetError, match="interp must be one of"):
            fn(*([None] * nargs), interp="nearest")
    assert warp.INTERPS == ("linear", "cubic")


def test_driver_flag():
    import deploy_bundle as D
    assert D.parse_args([]).interp == "linear"
    assert D.parse_args(["--interp", "linear"]).interp == "linear"
    assert D.parse_args(["--interp", "cubic"]).interp == "cubic"
    assert D.parse_args(["--interp", "cubic", "--pipeline"]).pipeline
    a = D.parse_args(["--interp", "cubic", "--fill", "0.8", "--ingest", "device"])
    assert a.interp == "cubic" and a.fill == 0.8
    a = D.parse_args(["--interp", "cubic", "--fill", "adaptive", "--ingest", "device"])
    assert a.interp == "cubic" and a.fill == "adaptive"
    a = D.parse_args(["--interp", "cubic", "--y4m-in", "a"])
    assert a.interp == "cubic" and a.y4m_in == "a" and a.output_size == "source"
    with pytest.raises(SystemExit):
        D.parse_args(["--interp", "nearest"])
