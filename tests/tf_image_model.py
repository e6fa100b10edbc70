"""NumPy model of the reference's get_img (get_data_mini_after.py:149-156) from the decoded frame on: tf.image.rgb_to_grayscale,
convert_image_dtype(float32), resize_images(method=0), - 0.5, with TensorFlow 1.3's arithmetic, float32 throughout.

TensorFlow cannot run here, so THIS MODEL IS THE YARDSTICK of csrc/tf_image.hip (tests/test_tf_image_gpu.py compares bit for bit);
every line that restates TensorFlow is marked [external], as stabnet_amd/data.py marks its own."""
import numpy as np

F = np.float32
K255 = F(1.0 / 255.0)                     # [external] convert_image_dtype uint8 -> float32: scale = 1. / dtype.max, a float32 multiply
WR, WG, WB = F(0.2989), F(0.5870), F(0.1140)    # [external] rgb_to_grayscale's rgb_weights
TO_U8 = F(255.5)                          # [external] convert_image_dtype float32 -> uint8: scale = dtype.max + 0.5, then a truncating cast


def grey_u8(rgb, order="ltr"):
    """uint8 [..., 3] (R, G, B) -> uint8 [...]: rgb_to_grayscale on a uint8 image.  order: how the three products are summed --
    'ltr' is the model ((r + g) + b); 'rtl' (r + (g + b)) and 'f64' exist for the order-sensitivity count only."""
    rgb = np.asarray(rgb, np.uint8)
    r = rgb[..., 0].astype(F) * K255                                  # [external] convert_image_dtype(image, float32)
    g = rgb[..., 1].astype(F) * K255
    b = rgb[..., 2].astype(F) * K255
    if order == "ltr":
        s = (r * WR + g * WG) + b * WB                                # [external] reduce_sum(rgb_weights * flt_image): left to right, no fma
    elif order == "rtl":
        s = r * WR + (g * WG + b * WB)
    else:                                                             # the same formula in float64 from the bytes on
        x = rgb.astype(np.float64)
        s64 = (x[..., 0] / 255 * 0.2989 + x[..., 1] / 255 * 0.5870) + x[..., 2] / 255 * 0.1140
        return (s64 * 255.5).astype(np.int32).astype(np.uint8)
    assert s.dtype == F
    return (s * TO_U8).astype(np.int32).astype(np.uint8)              # [external] saturate_cast(s * 255.5) to uint8: truncation (s in [0, 1))


def _axis(n_in, n_out):
    scale = F(n_in) / F(n_out)                                        # [external] CalculateResizeScale: in / static_cast<float>(out)
    f = np.arange(n_out, dtype=F) * scale                             # [external] in_y = y * height_scale
    lo = np.floor(f)                                                  # [external] top_y_index = floor(in_y)
    hi = np.where(f < F(n_in - 1), np.ceil(f), F(n_in - 1))           # [external] bottom_y_index = in_y < in - 1 ? ceil(in_y) : in - 1
    lerp = f - lo                                                     # [external] y_lerp = in_y - top_y_index
    assert lerp.dtype == F
    return lo.astype(np.int64), hi.astype(np.int64), lerp


def resize_legacy(f, H, W):
    """float32 [h, w] -> float32 [H, W]: resize_images(method=0), align_corners=False, no half-pixel centres."""
    f = np.asarray(f, F)
    y0, y1, yl = _axis(f.shape[0], H)
    x0, x1, xl = _axis(f.shape[1], W)
    tl, tr = f[y0][:, x0], f[y0][:, x1]
    bl, br = f[y1][:, x0], f[y1][:, x1]
    top = tl + (tr - tl) * xl[None, :]                                # [external] top = top_left + (top_right - top_left) * x_lerp
    bot = bl + (br - bl) * xl[None, :]                                # [external] bottom likewise
    out = top + (bot - top) * yl[:, None]                             # [external] top + (bottom - top) * y_lerp
    assert out.dtype == F
    return out


def get_img(rgb, H, W):
    """uint8 [h, w, 3] (R, G, B, as decode_jpeg gives it) -> float32 [H, W]."""
    u = grey_u8(rgb)
    f = u.astype(F) * K255                                            # [external] convert_image_dtype(image, float32)
    return resize_legacy(f, H, W) - F(0.5)                            # get_data_mini_after.py:153-154


def get_img_bgr(bgr, H, W):
    """The same for a frame stored B, G, R (what the project's decoder writes)."""
    return get_img(np.asarray(bgr)[..., ::-1], H, W)
