"""NumPy model of the remap through a window (csrc/remap.hip, stabnet_warp_rev_bundle2_win): output pixel (i, j) of OH x OW is the
stabilised frame, at the source's size SH x SW, sampled at a fractional position inside window = (y0, x0, wh, ww).  Composed from
remap_src_model (the four constants, the coverage rule) and the oracle's restatements of cv2.resize (the 4x shrink) and cv2.remap; the
step back up is a fractional-position version of the oracle's taps(): the position e in pixel-edge units takes the place of d + 0.5."""
import numpy as np

import remap_src_model as M
from oracle import stabnet_oracle as O

F = np.float32


def positions(o0, wlen, n_out):
    """e float64 [n_out]: o0 + (j + 0.5) * (wlen / n_out) -- the quotient, the product, the sum."""
    return float(o0) + (np.arange(n_out, dtype=np.float64) + 0.5) * (float(wlen) / n_out)


def taps_at(e, n_src, scale):
    """The oracle's taps() (cv_resize_linear_f32) at fractional destination positions e (float64, pixel-edge units)."""
    f = (e * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(F)
    lo = s < 0
    f[lo] = 0
    s[lo] = 0
    hi = s >= n_src - 1
    f[hi] = 0
    s[hi] = n_src - 1
    return s, np.minimum(s + 1, n_src - 1), (F(1.0) - f).astype(F), f.astype(F)


def resize_at(small, ex, ey, SW, SH):
    """small float32 [h, w] -> float32 [len(ey), len(ex)]: cv2.resize(small, (SW, SH)) read at the positions ex, ey of the big map.
    Horizontal pass on every row of `small`, then the vertical pass, float32 (as cv_resize_linear_f32)."""
    h, w = small.shape
    x0, x1, ax0, ax1 = taps_at(ex, w, float(w) / SW)
    y0, y1, by0, by1 = taps_at(ey, h, float(h) / SH)
    rows = small[:, x0] * ax0[None, :] + small[:, x1] * ax1[None, :]
    return rows[y0, :] * by0[:, None] + rows[y1, :] * by1[:, None]


def coords(x_map, y_map, SH, SW, window, OH, OW, rate=4):
    """px, py float32 [OH, OW]: the source-pixel coordinates cv2.remap receives for the output's pixels."""
    H, W = x_map.shape
    h, w = H // rate, W // rate
    wy0, wx0, wh, ww = window
    ex, ey = positions(wx0, ww, OW), positions(wy0, wh, OH)
    with np.errstate(invalid="ignore", over="ignore"):
        bx = resize_at(O.cv_resize_linear_f32(x_map, w, h), ex, ey, SW, SH)
        by = resize_at(O.cv_resize_linear_f32(y_map, w, h), ex, ey, SW, SH)
        ux = (bx + F(1)) / F(2) * F(W)
        uy = (by + F(1)) / F(2) * F(H)
        sx, cx, sy, cy = M.constants(H, W, SH, SW)
        return (ux * sx + cx).astype(F), (uy * sy + cy).astype(F)


def warp_win(src, x_map, y_map, window, out_size=None, rate=4):
    """src uint8 [SH, SW, C] or [SH, SW]; x_map, y_map float32 [H, W]; window (y0, x0, wh, ww); out_size (OH, OW), default the source's
    -> (out uint8 [OH, OW(, C)], px, py float32 [OH, OW], black bool [OH, OW]: the coverage rule of the SOURCE frame at the output pixel)."""
    src = np.asarray(src, np.uint8)
    img = src[..., None] if src.ndim == 2 else src
    SH, SW = img.shape[:2]
    OH, OW = (SH, SW) if out_size is None else out_size
    px, py = coords(np.asarray(x_map, F), np.asarray(y_map, F), SH, SW, window, OH, OW, rate)
    with np.errstate(invalid="ignore", over="ignore"):
        out = O.cv_remap_linear_u8(img, px, py)
    return out.reshape((OH, OW) + src.shape[2:]), px, py, M.black(px, py, SH, SW)
