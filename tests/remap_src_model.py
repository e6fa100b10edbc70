"""NumPy model of the remap at source resolution (csrc/remap.hip, stabnet_warp_rev_bundle2_src): the frame as read, warped at its own
size by the network-size maps.  Composed from the oracle's restatements of cv2.resize and cv2.remap, plus the four constants of the
change of coordinates and the coverage rule; the oracle itself is not edited."""
import numpy as np

from oracle import stabnet_oracle as O

F = np.float32

# (network H, W, source SH, SW)
SHAPES = [(32, 64, 32, 64), (32, 64, 90, 150), (32, 64, 77, 131), (64, 96, 48, 80), (36, 52, 135, 240)]
BIG = (288, 512, 1080, 1920)


def constants(H, W, SH, SW):
    """sx, cx, sy, cy: computed in double, rounded once.  The reference's normalised coordinate counts pixel INDICES ((m + 1) / 2 * W
    is a pixel index of the network-size frame), so under cv2's half-pixel convention index u of W maps to (u + 0.5) * SW / W - 0.5
    of SW: the offset c = 0.5 * SW / W - 0.5 is what keeps an identity mesh in place."""
    return F(SW / W), F(0.5 * SW / W - 0.5), F(SH / H), F(0.5 * SH / H - 0.5)


def coords(x_map, y_map, SH, SW, rate=4):
    """px, py float32 [SH, SW]: the source-pixel coordinates cv2.remap receives.  x_map, y_map [H, W] normalised."""
    H, W = x_map.shape
    h, w = H // rate, W // rate
    bx = O.cv_resize_linear_f32(O.cv_resize_linear_f32(x_map, w, h), SW, SH)
    by = O.cv_resize_linear_f32(O.cv_resize_linear_f32(y_map, w, h), SW, SH)
    ux = (bx + F(1)) / F(2) * F(W)
    uy = (by + F(1)) / F(2) * F(H)
    sx, cx, sy, cy = constants(H, W, SH, SW)
    return (ux * sx + cx).astype(F), (uy * sy + cy).astype(F)


def black(px, py, SH, SW):
    """bool [SH, SW]: the coordinate rounded to 1/32 px (half to even, as the remap rounds it) lies outside the frame; NaN too."""
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.clip(px * F(32), F(-2.0e9), F(2.0e9))
        qy = np.clip(py * F(32), F(-2.0e9), F(2.0e9))
    qx = np.rint(np.nan_to_num(qx, nan=-2.0e9)).astype(np.int64)
    qy = np.rint(np.nan_to_num(qy, nan=-2.0e9)).astype(np.int64)
    return (qx < 0) | (qx > 32 * (SW - 1)) | (qy < 0) | (qy > 32 * (SH - 1))


def warp_src(src, x_map, y_map, rate=4):
    """src uint8 [SH, SW, C] or [SH, SW]; x_map, y_map float32 [H, W] -> (out like src, px, py, black bool [SH, SW])."""
    src = np.asarray(src, np.uint8)
    img = src[..., None] if src.ndim == 2 else src
    SH, SW = img.shape[:2]
    px, py = coords(np.asarray(x_map, F), np.asarray(y_map, F), SH, SW, rate)
    with np.errstate(invalid="ignore", over="ignore"):
        out = O.cv_remap_linear_u8(img, px, py)
    return out.reshape(src.shape), px, py, black(px, py, SH, SW)


def identity_maps(H, W):
    """m = 2 * i / n - 1: pixel i of n maps onto itself."""
    x = (2.0 * np.arange(W, dtype=np.float64) / W - 1.0).astype(F)
    y = (2.0 * np.arange(H, dtype=np.float64) / H - 1.0).astype(F)
    return np.broadcast_to(x[None, :], (H, W)).copy(), np.broadcast_to(y[:, None], (H, W)).copy()


def mesh_maps(H, W, seed, shift=0.0, scale=0.06):
    """Maps of a random mesh (theta ~ N(0, scale), as tests/test_remap_gpu.py draws them), shifted.  -> x_map, y_map float32 [H, W]."""
    ocfg = O.Config(height=H, width=W)
    theta = (np.random.default_rng(seed).standard_normal((1, 50)) * scale).astype(F)
    _, pts2 = O.get_4_pts(theta, ocfg)
    x_map, y_map, _ = O.maps_from_Hs(O.get_Hs(pts2, ocfg), H, W, ocfg)
    return (x_map[0] + F(shift)).astype(F), (y_map[0] + F(shift)).astype(F)
