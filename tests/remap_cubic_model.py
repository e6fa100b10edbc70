"""NumPy model of the bicubic remap (csrc/remap.hip, stabnet_warp_rev_bundle2_cubic / _i420_cubic): cv2.remap(u8, map_x, map_y,
INTER_CUBIC, BORDER_CONSTANT) restated from OpenCV's published imgwarp.cpp (RemapInvoker, initInterTab2D(INTER_CUBIC, fixpt=true),
remapBicubic<FixedPtCast<int, uchar, 15>, short, 32768>).  [external]: no OpenCV build was at hand when this was written, so equality
with a real cv2.remap is unverified; tools/check_cubic_against_cv2.py closes the gap wherever cv2 is installed.  The coordinates are
those of the bilinear path (remap_src_model / remap_win_model / remap_i420_model); only the taps and the blend differ.  The oracle is
not edited."""
import numpy as np

import remap_i420_model as MI
import remap_src_model as M
import remap_win_model as MW

F = np.float32
ONE = 32768
_tab_cache = None
_repaired = None


def coeffs(i):
    """interpolateCubic(i / 32): the four 1-D weights of taps -1, 0, 1, 2, float32, evaluated left to right."""
    A, x, one = F(-0.75), F(i) * (F(1.0) / F(32)), F(1)
    x1, xm = x + one, one - x
    c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
    c1 = ((A + F(2)) * x - (A + F(3))) * x * x + one
    c2 = ((A + F(2)) * xm - (A + F(3))) * xm * xm + one
    c3 = F(1.0) - c0 - c1 - c2
    return [F(c0), F(c1), F(c2), F(c3)]


def table():
    """BicubicTab_i: int16 [1024, 16], entry fy * 32 + fx, tap k1 * 4 + k2 (k1 the row).  Each tap is
    saturate_cast<short>(rint(float32(cy[k1] * cx[k2]) * 32768)); an entry that does not sum to 32768 is repaired by OpenCV's loop over
    taps k1, k2 in {2, 3} (the minimum with strict <, otherwise the maximum with strict >, both starting at [2][2])."""
    global _tab_cache, _repaired
    if _tab_cache is not None:
        return _tab_cache
    tab1 = [coeffs(i) for i in range(32)]
    out = np.zeros((1024, 16), np.int64)
    diffs = []
    for i in range(32):
        for j in range(32):
            t = out[i * 32 + j]
            for k1 in range(4):
                for k2 in range(4):
                    v = F(tab1[i][k1] * tab1[j][k2])
                    t[k1 * 4 + k2] = int(np.clip(np.rint(np.float64(F(v * F(ONE)))), -32768, 32767))
            diff = int(t.sum()) - ONE
            if diff != 0:
                diffs.append(diff)
                mk = Mk = 2 * 4 + 2
                for k1 in (2, 3):
                    for k2 in (2, 3):
                        k = k1 * 4 + k2
                        if t[k] < t[mk]:
                            mk = k
                        elif t[k] > t[Mk]:
                            Mk = k
                if diff < 0:
                    t[Mk] -= diff
                else:
                    t[mk] -= diff
    assert out.min() >= -32768 and out.max() <= 32767
    _tab_cache, _repaired = out.astype(np.int16), diffs
    return _tab_cache


def repaired_diffs():
    """The non-zero `sum - 32768` of the entries before their repair, in table order."""
    table()
    return list(_repaired)


def quantise(px, py):
    """-> (ix, iy, fx, fy) int64: the coordinate in 1/32 px (half to even, clamped, NaN -> -2e9), integer part saturated to int16."""
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.clip(np.asarray(px, F) * F(32), F(-2.0e9), F(2.0e9))
        qy = np.clip(np.asarray(py, F) * F(32), F(-2.0e9), F(2.0e9))
    sx = np.rint(np.nan_to_num(qx, nan=-2.0e9)).astype(np.int64)
    sy = np.rint(np.nan_to_num(qy, nan=-2.0e9)).astype(np.int64)
    return np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767), sx & 31, sy & 31


def cv_remap_cubic_u8(img, map_x, map_y, border=0):
    """img uint8 [H, W, C]; map_x, map_y float32 [h, w] -> uint8 [h, w, C].  Taps at rows iy - 1 .. iy + 2, columns ix - 1 .. ix + 2; a
    tap outside the frame reads `border` (the weights sum to 32768, so this is OpenCV's cval * ONE + sum((S - cval) * w));
    out = clamp((sum(v * w) + 16384) >> 15, 0, 255)."""
    img = np.asarray(img, np.uint8)
    H, W, C = img.shape
    ix, iy, fx, fy = quantise(map_x, map_y)
    w = table()[fy * 32 + fx].astype(np.int64)               # [h, w, 16]
    acc = np.zeros(ix.shape + (C,), np.int64)
    for k1 in range(4):
        yy = iy - 1 + k1
        for k2 in range(4):
            xx = ix - 1 + k2
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
            acc += np.where(ok[..., None], v, int(border)) * w[..., k1 * 4 + k2][..., None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def taps_inside(px, py, SH, SW):
    """bool: all 16 taps of the pixel lie inside the SH x SW frame."""
    ix, iy, _, _ = quantise(px, py)
    return (ix - 1 >= 0) & (ix + 2 < SW) & (iy - 1 >= 0) & (iy + 2 < SH)


def warp_src(src, x_map, y_map, rate=4):
    """remap_src_model.warp_src under INTER_CUBIC -> (out like src, px, py, black bool [SH, SW])."""
    src = np.asarray(src, np.uint8)
    img = src[..., None] if src.ndim == 2 else src
    SH, SW = img.shape[:2]
    px, py = M.coords(np.asarray(x_map, F), np.asarray(y_map, F), SH, SW, rate)
    return cv_remap_cubic_u8(img, px, py).reshape(src.shape), px, py, M.black(px, py, SH, SW)


def warp_win(src, x_map, y_map, window, out_size=None, rate=4):
    """remap_win_model.warp_win under INTER_CUBIC -> (out [OH, OW(, C)], px, py, black bool [OH, OW])."""
    src = np.asarray(src, np.uint8)
    img = src[..., None] if src.ndim == 2 else src
    SH, SW = img.shape[:2]
    OH, OW = (SH, SW) if out_size is None else out_size
    px, py = MW.coords(np.asarray(x_map, F), np.asarray(y_map, F), SH, SW, window, OH, OW, rate)
    return cv_remap_cubic_u8(img, px, py).reshape((OH, OW) + src.shape[2:]), px, py, M.black(px, py, SH, SW)


def warp_i420(frame, x_map, y_map, SH, SW, planes=3, window=None, out_size=None, border_y=0, rate=4):
    """remap_i420_model.warp_i420 under INTER_CUBIC: every plane as the single-channel image it is, chroma through the halved window,
    taps outside a plane read border_y (Y) or 128 (U, V).  -> (uint8 [bytes of the output frame], black bool [OH, OW])."""
    OH, OW = (SH, SW) if out_size is None else out_size
    outs, black = [], None
    for k, plane in enumerate(MI.split(frame, SH, SW, planes)):
        d = 1 if k == 0 else 2
        win = None if window is None else tuple(float(v) / d for v in window)        # halving a double is exact
        px, py = MI.plane_coords(x_map, y_map, SH // d, SW // d, win, OH // d, OW // d, rate)
        outs.append(cv_remap_cubic_u8(plane[..., None], px, py, border=border_y if k == 0 else 128).reshape(-1))
        if k == 0:
            black = M.black(px, py, SH, SW)
    return np.concatenate(outs), black
