"""CPU: the NumPy model of the planar 4:2:0 remap (tests/remap_i420_model.py) against the oracle where the oracle can speak (border 0),
the property the border value must have (a uniform plane stays uniform), the chroma plane's coordinates against the luma plane's, and
the refusals of stabnet_warp_rev_bundle2_i420, which need no GPU."""
import ctypes
import functools

import numpy as np
import pytest

import remap_i420_model as IM
import remap_src_model as M
import remap_win_model as WM
from oracle import stabnet_oracle as O

F = np.float32
SEED = 5
MAPS = ["identity", "mesh", "mesh+0.3", "mesh-0.3"]


@functools.lru_cache(maxsize=None)
def _maps(H, W, kind):
    if kind == "identity":
        return M.identity_maps(H, W)
    return M.mesh_maps(H, W, seed=SEED, shift={"mesh": 0.0, "mesh+0.3": 0.3, "mesh-0.3": -0.3}[kind])


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", IM.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_border_zero_gather_is_the_oracles(shape, kind):
    H, W, SH, SW = shape
    xm, ym = _maps(H, W, kind)
    frame = np.random.default_rng(SH * 1000 + SW).integers(0, 256, SH * SW * 3 // 2, dtype=np.uint8)
    for k, plane in enumerate(IM.split(frame, SH, SW)):
        d = 1 if k == 0 else 2
        px, py = IM.plane_coords(xm, ym, SH // d, SW // d, None, SH // d, SW // d)
        want = O.cv_remap_linear_u8(plane[..., None], px, py)[..., 0]
        assert np.count_nonzero(IM.gather(plane, px, py, 0) != want) == 0, k
        # and through a window: the same gather on the window model's coordinates
        win = tuple(v / d for v in (0.1 * SH, 0.1 * SW, 0.8 * SH, 0.8 * SW))
        px, py = IM.plane_coords(xm, ym, SH // d, SW // d, win, SH // d, SW // d)
        want = O.cv_remap_linear_u8(plane[..., None], px, py)[..., 0]
        assert np.count_nonzero(IM.gather(plane, px, py, 0) != want) == 0, k


def test_weights_always_sum_to_32768():
    """Every (fy, fx) of the 32 x 32 table, the repaired entry (0, 0) included: what keeps a uniform plane uniform."""
    fy, fx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    w = IM.weights(fx, fy)
    assert (w.sum(axis=-1) == 32768).all()
    assert tuple(w[0, 0]) == (32767, 0, 0, 1)
    assert np.array_equal(w.reshape(1024, 4), O.cv_bilinear_tab_i())


@pytest.mark.parametrize("b", [0, 16, 128, 255])
@pytest.mark.parametrize("kind", ["mesh+0.3", "mesh-0.3"])
def test_uniform_plane_with_its_own_border_stays_uniform(kind, b):
    H, W, SH, SW = 32, 64, 90, 150
    xm, ym = _maps(H, W, kind)
    px, py = M.coords(xm, ym, SH, SW)
    assert M.black(px, py, SH, SW).mean() >= 0.05                    # the border is read
    plane = np.full((SH, SW), b, np.uint8)
    assert (IM.gather(plane, px, py, b) == b).all()
    if b:
        assert (IM.gather(plane, px, py, 0) != b).any()              # and a zero border shows


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", IM.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_chroma_coordinate_is_the_halved_luma_coordinate_of_the_chroma_sample(shape, kind):
    """Centred siting: chroma sample j covers luma pixels 2j and 2j + 1, its centre is the luma pixel-edge position 2 (j + 0.5); the luma
    coordinate p_L there (the luma model through the whole-frame window at half the output size) is the chroma coordinate
    p_C = (p_L + 0.5) / 2 - 0.5.  The small-map taps are the same bits (every scale is an exact power-of-two multiple), so the two differ
    by the float32 roundings of `u * s` and `+ c` on either side: at most 1 ulp of the largest luma coordinate in all; 2 are allowed."""
    H, W, SH, SW = shape
    xm, ym = _maps(H, W, kind)
    pcx, pcy = M.coords(xm, ym, SH // 2, SW // 2)
    plx, ply = WM.coords(xm, ym, SH, SW, (0.0, 0.0, float(SH), float(SW)), SH // 2, SW // 2)
    for pc, pl in ((pcx, plx), (pcy, ply)):
        want = (pl.astype(np.float64) + 0.5) / 2 - 0.5
        tol = 2 * float(np.spacing(F(np.abs(pl).max())))
        assert np.abs(pc.astype(np.float64) - want).max() <= tol


def test_every_refusal_returns_minus_one_without_a_gpu():
    from stabnet_amd import _lib
    L = _lib.lib()
    SH, SW, H, W = 90, 160, 32, 64
    win = lambda *v: (ctypes.c_double * 4)(*v)
    P = 4096                                                        # a non-null pointer that is never followed: every case is refused first
    good = dict(src=P, N=1, SH=SH, SW=SW, planes=3, stride=SH * SW * 3 // 2, x_map=P, y_map=P, H=H, W=W, rate=4, window=None, OH=SH, OW=SW,
                border_y=16, out=P, black=0, ws=P, stream=0, prof=0)
    inf, nan = float("inf"), float("nan")
    whole = win(0, 0, SH, SW)
    bads = [(dict(src=0), "null"), (dict(out=0), "null"), (dict(x_map=0), "null"), (dict(y_map=0), "null"), (dict(ws=0), "null"),
            (dict(planes=0), "planes"), (dict(planes=2), "planes"), (dict(planes=4), "planes"),
            (dict(SH=89, OH=89), "even"), (dict(SW=159, OW=159), "even"), (dict(OH=89, window=whole), "even"), (dict(OW=159, window=whole), "even"),
            (dict(N=0), "batch"), (dict(N=65536), "batch"),
            (dict(SH=0, OH=0), "outside"), (dict(SW=0, OW=0), "outside"), (dict(SH=32768, OH=32768), "outside"), (dict(SW=32768, OW=32768), "outside"),
            (dict(OH=0, window=whole), "outside"), (dict(OW=32768, window=whole), "outside"),
            (dict(stride=SH * SW * 3 // 2 - 1), "stride"), (dict(planes=1, stride=SH * SW - 1), "stride"),
            (dict(border_y=-1), "border_y"), (dict(border_y=256), "border_y"),
            (dict(rate=0), "rate"), (dict(rate=33), "rate"), (dict(H=3), "rate"), (dict(W=3), "rate"),
            (dict(OH=SH - 2), "null window"), (dict(OW=SW + 2), "null window"),
            (dict(window=win(nan, 0, SH, SW)), "finite"), (dict(window=win(0, nan, SH, SW)), "finite"), (dict(window=win(0, 0, inf, SW)), "finite"),
            (dict(window=win(0, 0, SH, nan)), "finite"), (dict(window=win(0, 0, 0, SW)), "empty"), (dict(window=win(0, 0, SH, 0)), "empty"),
            (dict(window=win(0, 0, -1, SW)), "empty"), (dict(window=win(0, 0, SH, -1)), "empty"),
            (dict(window=win(-1e-5, 0, SH, SW)), "leaves"), (dict(window=win(0, -1e-5, SH, SW)), "leaves"),
            (dict(window=win(0, 0, SH + 1e-5, SW)), "leaves"), (dict(window=win(0, 0, SH, SW + 1e-5)), "leaves"),
            (dict(window=win(1, 0, SH, SW)), "leaves"), (dict(window=win(0, 1, SH, SW)), "leaves")]
    for bad, word in bads:
        assert L.stabnet_warp_rev_bundle2_i420(*dict(good, **bad).values()) == -1, bad
        msg = L.stabnet_last_error().decode()
        assert "warp_rev_bundle2_i420" in msg and word in msg, (bad, msg)
