"""NumPy model of the planar 4:2:0 remap (csrc/remap.hip, stabnet_warp_rev_bundle2_i420): every plane is the remap of a single-channel
image of the plane's own size -- coordinates from remap_src_model.coords (the whole frame) or remap_win_model.coords (a window; a chroma
plane takes the halved window) -- gathered by a short fixed-point bilinear with a BORDER VALUE for the taps outside the plane (cv2.remap's
borderValue), which the oracle's cv_remap_linear_u8 does not have (border 0 only) and which is therefore stated here; the oracle is not
edited.  With border 0 the gather is cv_remap_linear_u8's, byte for byte (tests/test_remap_i420_model_cpu.py)."""
import numpy as np

import remap_src_model as M
import remap_win_model as WM

F = np.float32

# (network H, W, source SH, SW): the network's own size; both plane kinds on the four-pixel path with an odd chroma height (45);
# Y four-pixel and chroma width 66 one-pixel; both one-pixel; a second network size
SHAPES = [(32, 64, 32, 64), (32, 64, 90, 160), (32, 64, 78, 132), (32, 64, 90, 150), (36, 52, 136, 240)]


def weights(qx, qy):
    """The four 15-bit weights of taps [0][0], [0][1], [1][0], [1][1] for coordinates in 1/32 px: exact multiples of 32, except the
    entry (0, 0) of OpenCV's table, {32767, 0, 0, 1} (the saturated 1.0 and its repair).  -> int64 [..., 4], every sum 32768."""
    fx, fy = qx & 31, qy & 31
    w = np.stack([(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32], axis=-1).astype(np.int64)
    w[(fx | fy) == 0] = (32767, 0, 0, 1)
    return w


def quantise(px, py):
    """The coordinates in 1/32 px as the remap rounds them (float32 product, clamped, half to even; NaN: far outside)."""
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.clip(np.asarray(px, F) * F(32), F(-2.0e9), F(2.0e9))
        qy = np.clip(np.asarray(py, F) * F(32), F(-2.0e9), F(2.0e9))
    return np.rint(np.nan_to_num(qx, nan=-2.0e9)).astype(np.int64), np.rint(np.nan_to_num(qy, nan=-2.0e9)).astype(np.int64)


def gather(plane, px, py, border):
    """plane uint8 [h, w]; px, py float32 [oh, ow] -> uint8 [oh, ow]: the fixed-point bilinear remap, taps outside the plane = border."""
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape
    qx, qy = quantise(px, py)
    ix, iy = np.clip(qx >> 5, -32768, 32767), np.clip(qy >> 5, -32768, 32767)
    wt = weights(qx, qy)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, plane[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), int(border))

    acc = tap(iy, ix) * wt[..., 0] + tap(iy, ix + 1) * wt[..., 1] + tap(iy + 1, ix) * wt[..., 2] + tap(iy + 1, ix + 1) * wt[..., 3]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def split(frame, SH, SW, planes=3):
    """frame uint8 [bytes] -> [Y [SH,SW]] or [Y, U [SH/2,SW/2], V]: views."""
    frame = np.asarray(frame, np.uint8).reshape(-1)
    y = frame[:SH * SW].reshape(SH, SW)
    if planes == 1:
        return [y]
    c = (SH // 2) * (SW // 2)
    return [y, frame[SH * SW:SH * SW + c].reshape(SH // 2, SW // 2), frame[SH * SW + c:SH * SW + 2 * c].reshape(SH // 2, SW // 2)]


def plane_coords(x_map, y_map, sh, sw, window, oh, ow, rate=4):
    """px, py float32 [oh, ow] of one plane of size sh x sw: the source-resolution model's, or the window model's."""
    if window is None:
        assert (oh, ow) == (sh, sw)
        return M.coords(np.asarray(x_map, F), np.asarray(y_map, F), sh, sw, rate)
    return WM.coords(np.asarray(x_map, F), np.asarray(y_map, F), sh, sw, window, oh, ow, rate)


def warp_i420(frame, x_map, y_map, SH, SW, planes=3, window=None, out_size=None, border_y=0, rate=4):
    """frame uint8 [SH*SW*3/2] (planes == 1: [SH*SW]); x_map, y_map float32 [H, W]; window (y0, x0, wh, ww) of the luma frame or None
    -> (out uint8 [OH*OW*3/2], black bool [OH, OW]: the coverage rule at the luma output pixel)."""
    OH, OW = (SH, SW) if out_size is None else out_size
    outs, black = [], None
    for k, plane in enumerate(split(frame, SH, SW, planes)):
        d = 1 if k == 0 else 2
        win = None if window is None else tuple(float(v) / d for v in window)        # halving a double is exact
        px, py = plane_coords(x_map, y_map, SH // d, SW // d, win, OH // d, OW // d, rate)
        outs.append(gather(plane, px, py, border_y if k == 0 else 128).reshape(-1))
        if k == 0:
            black = M.black(px, py, SH, SW)
    return np.concatenate(outs), black
