"""NumPy model of the adaptive window (csrc/remap.hip, stabnet_fill_window_update): the bad nodes of the small maps from the oracle's
restatement of cv2.resize, remap_src_model's four constants and its coverage rule shrunk by the margin; the key in integers; the update
in Python floats (IEEE doubles, the kernel's order).  Not a test module."""
import numpy as np

import remap_src_model as M
from oracle import stabnet_oracle as O

F = np.float32


def node_q(x_map, y_map, SH, SW, rate=4):
    """qx, qy int64 [h, w]: the coordinate of every small-map node in 1/32 source px, as the remap computes it with all the weight on
    the node (v * 1 + v * 0 in both passes: an infinite entry becomes NaN there), rounded half to even; NaN -> -2e9."""
    H, W = x_map.shape
    h, w = H // rate, W // rate
    sx, cx, sy, cy = M.constants(H, W, SH, SW)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for m, size, s, c in ((x_map, W, sx, cx), (y_map, H, sy, cy)):
            v = O.cv_resize_linear_f32(np.asarray(m, F), w, h).astype(F)
            v = v * F(1) + v * F(0)
            v = v * F(1) + v * F(0)
            p = ((v + F(1)) / F(2) * F(size)) * s + c
            q = np.clip(p.astype(F) * F(32), F(-2.0e9), F(2.0e9))
            out.append(np.rint(np.nan_to_num(q, nan=-2.0e9)).astype(np.int64))
    return out[0], out[1]


def bad_nodes(x_map, y_map, SH, SW, margin_q=8, rate=4):
    """bool [h, w]: remap_src_model.black's rule on the node's own coordinate, with the box shrunk by margin_q on every side."""
    qx, qy = node_q(x_map, y_map, SH, SW, rate)
    return (qx < margin_q) | (qx > 32 * (SW - 1) - margin_q) | (qy < margin_q) | (qy > 32 * (SH - 1) - margin_q)


def key_of(bad):
    """(key, bad count): key = min over bad nodes (a, b) of max((|2b+1-w| - 2) * h, (|2a+1-h| - 2) * w); h * w when none is bad."""
    h, w = bad.shape
    a, b = np.nonzero(bad)
    if len(a) == 0:
        return h * w, 0
    k = np.maximum((np.abs(2 * b.astype(np.int64) + 1 - w) - 2) * h, (np.abs(2 * a.astype(np.int64) + 1 - h) - 2) * w)
    return int(k.min()), int(len(a))


def r_safe_of(key, h, w):
    return 1.0 if key >= h * w else float(key) / float(h * w)


def update(state, key, h, w, SH, SW, r_min=0.5, up=0.002):
    """One frame: -> (new state r, window (y0, x0, wh, ww)).  Python floats, the kernel's order."""
    r = min(r_safe_of(key, h, w), state + up)
    r = max(r, r_min)
    r = min(r, 1.0)
    wh, ww = SH * r, SW * r
    return r, ((SH - wh) / 2, (SW - ww) / 2, wh, ww)


def frame(x_map, y_map, SH, SW, state, r_min=0.5, up=0.002, margin_q=8, rate=4):
    """One frame from its maps: -> (new state, window, key, bad count)."""
    bad = bad_nodes(x_map, y_map, SH, SW, margin_q, rate)
    key, cnt = key_of(bad)
    r, win = update(state, key, bad.shape[0], bad.shape[1], SH, SW, r_min, up)
    return r, win, key, cnt
