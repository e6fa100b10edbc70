"""CPU: adaptive borderless output without a GPU.  The rule's safety on the NumPy models (tests/fill_adaptive_model.py decides the
window from the small-map nodes; tests/remap_win_model.py says which output pixels that window leaves uncovered): whenever the rule
finds a ratio > 0, the window of that ratio shows no uncovered pixel.  Hand-computed keys and an update sequence; the driver's
--fill adaptive; the two entries' refusals, which come before any launch."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

import fill_adaptive_model as FM
import remap_src_model as M
import remap_win_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda s: "%dx%d-%dx%d" % s
SEEDS, SHIFTS, SCALES = range(6), (0.0, 0.1, -0.2, 0.45), (0.06, 0.15)


def _ratio_window(SH, SW, r):
    from stabnet_amd.warp import ratio_window
    return ratio_window(SH, SW, r)


@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_the_safe_window_shows_no_uncovered_pixel(shape):
    H, W, SH, SW = shape
    h, w = H // 4, W // 4
    positive = below_one = 0
    for seed in SEEDS:
        for shift in SHIFTS:
            for scale in SCALES:
                xm, ym = M.mesh_maps(H, W, seed, shift=shift, scale=scale)
                key, cnt = FM.key_of(FM.bad_nodes(xm, ym, SH, SW))
                r_safe = FM.r_safe_of(key, h, w)
                assert (cnt == 0) == (key == h * w) and r_safe <= 1.0
                if r_safe <= 0:
                    continue
                positive += 1
                below_one += r_safe < 1.0
                window = _ratio_window(SH, SW, r_safe)
                for OH, OW in ((SH, SW), (SH // 2 + 1, SW // 2 + 3)):
                    px, py = WM.coords(xm, ym, SH, SW, window, OH, OW)
                    uncovered = int(M.black(px, py, SH, SW).sum())
                    assert uncovered == 0, (seed, shift, scale, OH, OW, r_safe, uncovered)
    assert positive >= 12 and below_one >= 6          # the grid exercises the rule: windows that had to shrink, and were safe


def test_identity_maps_have_no_bad_node():
    for H, W, SH, SW in M.SHAPES:
        xm, ym = M.identity_maps(H, W)
        bad = FM.bad_nodes(xm, ym, SH, SW)
        h, w = H // 4, W // 4
        assert bad.shape == (h, w) and FM.key_of(bad) == (h * w, 0)
        assert FM.frame(xm, ym, SH, SW, 1.0) == (1.0, (0.0, 0.0, float(SH), float(SW)), h * w, 0)


def test_a_single_bad_node_hand_computed():
    # 8 x 16 nodes, node (a, b) = (2, 3): (|2*3+1-16| - 2) * 8 = 56 in x, (|2*2+1-8| - 2) * 16 = 16 in y; avoiding it in x is enough
    bad = np.zeros((8, 16), bool)
    bad[2, 3] = True
    assert FM.key_of(bad) == (56, 1)
    assert FM.r_safe_of(56, 8, 16) == 56 / 128
    # the mirrored node gives the same key; two bad nodes: the smaller key binds
    bad[:] = False
    bad[5, 12] = True
    assert FM.key_of(bad) == (56, 1)
    bad[0, 0] = True                                   # (|1-16| - 2) * 8 = 104, (|1-8| - 2) * 16 = 80
    assert FM.key_of(bad) == (56, 2)
    bad[:] = False
    bad[0, 0] = True
    assert FM.key_of(bad) == (104, 1)
    # through the maps (rate 1: the shrink is the identity): one entry of an identity map pushed out of the frame
    xm, ym = M.identity_maps(8, 16)
    xm[2, 3] = -1.5
    got = FM.bad_nodes(xm, ym, 40, 80, rate=1)
    assert got.sum() == 1 and got[2, 3]
    r, win, key, cnt = FM.frame(xm, ym, 40, 80, 1.0, rate=1)
    assert (key, cnt, r) == (56, 1, 0.5) and win == (10.0, 20.0, 20.0, 40.0)          # 0.4375 < r_min: held at 0.5
    assert FM.frame(xm, ym, 40, 80, 1.0, r_min=0.25, rate=1)[:2] == (0.4375, (11.25, 22.5, 17.5, 35.0))


def test_the_margin_decides_a_node_near_the_border():
    # identity maps at rate 1, SH, SW = H, W: node (a, b) sits at source pixel (a, b) exactly, qx = 32 b; column 0 is bad for any margin > 0
    xm, ym = M.identity_maps(8, 16)
    assert not FM.bad_nodes(xm, ym, 8, 16, margin_q=0, rate=1).any()
    bad = FM.bad_nodes(xm, ym, 8, 16, margin_q=8, rate=1)
    assert bad[:, 0].all() and bad[0, :].all() and bad[:, 15].all() and bad[7, :].all() and not bad[1:7, 1:15].any()


def test_an_odd_width_with_the_centre_column_bad_gives_a_negative_key():
    bad = np.zeros((9, 13), bool)
    bad[:, 6] = True                                   # x: (|13-13| - 2) * 9 = -18 on the whole column; y at a = 4: (0 - 2) * 13 = -26
    key, cnt = FM.key_of(bad)
    assert (key, cnt) == (-18, 9)
    assert FM.r_safe_of(key, 9, 13) < 0
    r, win = FM.update(1.0, key, 9, 13, 77, 131, r_min=0.5, up=0.002)
    assert r == 0.5 and win == _ratio_window(77, 131, 0.5)


def test_the_update_sequence():
    """Zooming in is immediate, zooming out limited to `up` per frame, never below r_min or above 1."""
    h, w, SH, SW = 10, 10, 90, 150
    keys = [100, 90, 100, 100, 30, 100, 250, 60, 59, -4]
    want = [1.0, 0.9, 0.95, 1.0, 0.5, 0.55, 0.6, 0.6, 0.59, 0.5]
    state = 1.0
    for key, r_want in zip(keys, want):
        state, win = FM.update(state, key, h, w, SH, SW, r_min=0.5, up=0.05)
        assert math.isclose(state, r_want, rel_tol=1e-12), (key, state, r_want)
        assert win == _ratio_window(SH, SW, state)
    # up = 0: the window never grows back
    state = 1.0
    for key, r_want in zip([80, 100, 70, 100], [0.8, 0.8, 0.7, 0.7]):
        state, _ = FM.update(state, key, h, w, SH, SW, r_min=0.5, up=0.0)
        assert state == r_want


def test_fill_adaptive_option():
    sys.path.insert(0, ROOT)
    import deploy_bundle
    a = deploy_bundle.parse_args(["--ingest", "device", "--fill", "adaptive"])
    assert (a.fill, a.fill_min, a.fill_up) == ("adaptive", 0.5, 0.002)
    a = deploy_bundle.parse_args(["--ingest", "device", "--output-size", "source", "--fill", "adaptive", "--fill-min", "0.7", "--fill-up", "0",
                                  "--pipeline"])
    assert (a.fill, a.fill_min, a.fill_up, a.pipeline) == ("adaptive", 0.7, 0.0, True)
    assert deploy_bundle.parse_args(["--ingest", "device", "--fill", "adaptive", "--fill-min", "1"]).fill_min == 1.0
    # the other modes keep their meaning, and do not grow the new attributes' values
    a = deploy_bundle.parse_args(["--ingest", "device", "--fill", "0.8"])
    assert (a.fill, a.fill_min, a.fill_up) == (0.8, None, None)
    assert deploy_bundle.parse_args(["--ingest", "device", "--fill", "auto"]).fill == "auto"
    assert deploy_bundle.parse_args([]).fill is None
    dev = ["--ingest", "device"]
    for bad in (["--fill", "adaptive"], ["--ingest", "host", "--fill", "adaptive"], dev + ["--fill", "Adaptive"],
                ["--fill-min", "0.5"], ["--fill-up", "0.01"], dev + ["--fill-min", "0.5"], dev + ["--fill", "0.8", "--fill-min", "0.5"],
                dev + ["--fill", "auto", "--fill-up", "0.01"],
                dev + ["--fill", "adaptive", "--fill-min", "0"], dev + ["--fill", "adaptive", "--fill-min", "-0.1"],
                dev + ["--fill", "adaptive", "--fill-min", "1.01"], dev + ["--fill", "adaptive", "--fill-min", "nan"],
                dev + ["--fill", "adaptive", "--fill-up", "-0.001"], dev + ["--fill", "adaptive", "--fill-up", "inf"],
                dev + ["--fill", "adaptive", "--fill-up", "nan"], dev + ["--fill", "adaptive", "--fill-up", "x"]):
        with pytest.raises(SystemExit):
            deploy_bundle.parse_args(bad)


def test_update_entry_refusals_need_no_gpu():
    """Every refusal comes before the first launch, so it can be asked for without a device."""
    from stabnet_amd import _lib
    L = _lib.lib()
    assert L.stabnet_abi_version() >= 4
    p = 4096                                                  # stands for a pointer: never dereferenced on these paths
    names = ("x_map", "y_map", "N", "H", "W", "rate", "SH", "SW", "r_min", "up", "margin_q", "state", "window", "stats", "ws", "stream")
    good = dict(x_map=p, y_map=p, N=1, H=32, W=64, rate=4, SH=77, SW=131, r_min=0.5, up=0.002, margin_q=8, state=p, window=p, stats=p,
                ws=p, stream=0)
    assert tuple(good) == names
    inf, nan = float("inf"), float("nan")
    for bad in (dict(x_map=0), dict(y_map=0), dict(state=0), dict(window=0), dict(stats=0), dict(ws=0), dict(N=0), dict(N=65536),
                dict(SH=0), dict(SW=0), dict(SH=32768), dict(SW=32768), dict(H=3), dict(W=3), dict(rate=0), dict(rate=33), dict(H=0),
                dict(r_min=0.0), dict(r_min=-0.5), dict(r_min=1.0000001), dict(r_min=nan), dict(r_min=inf),
                dict(up=-1e-9), dict(up=nan), dict(up=inf), dict(up=-inf),
                dict(margin_q=-1), dict(margin_q=16 * 77 + 1), dict(SH=5, SW=9, margin_q=81)):
        assert L.stabnet_fill_window_update(*dict(good, **bad).values()) == -1, bad
        assert b"fill_window_update" in L.stabnet_last_error()


def test_win_dev_entry_refusals_need_no_gpu():
    """_win's refusals, except those about the window's values (the host never sees them)."""
    from stabnet_amd import _lib
    L = _lib.lib()
    p = 4096
    good = dict(src=p, N=1, SH=77, SW=131, C=3, stride=393, x_map=p, y_map=p, H=32, W=64, rate=4, window=p, OH=60, OW=96, out=p, black=0,
                ws=p, px=0, py=0, stream=0, prof=0)
    for bad in (dict(src=0), dict(x_map=0), dict(y_map=0), dict(out=0), dict(ws=0), dict(C=0), dict(C=2), dict(C=4), dict(N=0), dict(SH=0),
                dict(SW=0), dict(SH=32768), dict(SW=32768, stride=3 * 32768), dict(H=3), dict(W=3), dict(rate=0), dict(rate=33),
                dict(stride=392), dict(px=p), dict(py=p),
                dict(OH=0), dict(OW=0), dict(OH=32768), dict(OW=32768), dict(OH=-1), dict(window=0)):
        assert L.stabnet_warp_rev_bundle2_win_dev(*dict(good, **bad).values()) == -1, bad
        assert b"warp_rev_bundle2_win_dev" in L.stabnet_last_error()


def test_python_layer_needs_no_gpu_to_refuse():
    import torch
    from stabnet_amd import _lib, warp
    assert warp.check_fill_params() == (0.5, 0.002, 8)
    assert warp.check_fill_params(1, 0, 0, 77, 131) == (1.0, 0.0, 0)
    assert warp.check_fill_params(0.25, 0.5, 16 * 77, 77, 131) == (0.25, 0.5, 16 * 77)
    for bad in (dict(r_min=0), dict(r_min=1.5), dict(r_min=float("nan")), dict(up=-1), dict(up=float("inf")), dict(up=float("nan")),
                dict(margin_q=-1), dict(margin_q=2.5), dict(margin_q=16 * 77 + 1, SH=77, SW=131), dict(r_min="x")):
        with pytest.raises(ValueError):
            warp.check_fill_params(**bad)
    with pytest.raises(ValueError):
        warp.AdaptiveFill(1, 77, 131, r_min=0.0, device="cpu")
    with pytest.raises(_lib.StabnetError):
        warp.AdaptiveFill(1, 77, 131, device="cpu")
    m = torch.zeros((1, 32, 64))
    with pytest.raises(_lib.StabnetError):
        warp.fill_window_update(m, m, 77, 131, torch.ones(1, dtype=torch.float64), torch.zeros((1, 4), dtype=torch.float64),
                                torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(_lib.StabnetError):                    # a window tensor does not make a CPU frame acceptable
        warp.warpRevBundle2_win(torch.zeros((1, 45, 77, 3), dtype=torch.uint8), m, m, torch.zeros(4, dtype=torch.float64))
