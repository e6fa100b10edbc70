"""CPU: tests/tf_image_model.py, the NumPy restatement of TensorFlow 1.3's rgb_to_grayscale / convert_image_dtype / legacy bilinear
resize that csrc/tf_image.hip is held to.  TensorFlow cannot run here; these tests pin the properties that follow from its
arithmetic and record how order-sensitive the grey sum is."""
import numpy as np

import tf_image_model as M

F = np.float32


def _all_triples():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8)


def test_white_and_black():
    assert M.grey_u8(np.array([[255, 255, 255]], np.uint8)).tolist() == [255]
    assert M.grey_u8(np.array([[0, 0, 0]], np.uint8)).tolist() == [0]


def test_grey_sum_is_order_sensitive_counts():
    """Of the 2^24 triples, 47 change their byte when the products are summed right to left, and 237 differ from the same formula in
    float64: the kernel has to pin the order and must not contract into fused multiply-adds."""
    rgb = _all_triples()
    ltr = M.grey_u8(rgb)
    assert int((ltr != M.grey_u8(rgb, "rtl")).sum()) == 47
    assert int((ltr != M.grey_u8(rgb, "f64")).sum()) == 237


def test_same_size_resize_is_exact():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    got = M.get_img(rgb, 16, 24)
    assert got.dtype == F
    assert np.array_equal(got, M.grey_u8(rgb).astype(F) * M.K255 - F(0.5))


def test_bottom_and_right_clamp_when_upscaling():
    rng = np.random.default_rng(2)
    f = rng.random((8, 8)).astype(F)
    out = M.resize_legacy(f, 16, 24)
    # 8 -> 16: in_y of row 15 is 7.5, past in - 1 = 7: top = bottom = row 7; 8 -> 24: columns 22, 23 (7.33, 7.67) both read column 7
    assert np.array_equal(out[15], out[14])
    assert np.array_equal(out[:, 22], out[:, 21]) and np.array_equal(out[:, 23], out[:, 21])
    assert out[15, 23] == f[7, 7] and out[0, 0] == f[0, 0]
    # an interior sample: row 3 = in_y 1.5 -> halfway between rows 1 and 2; column 3 = in_x 1.0 exactly
    assert out[3, 3] == f[1, 1] + (f[2, 1] - f[1, 1]) * F(0.5)
    y0, y1, yl = M._axis(8, 16)
    assert y0.tolist()[-2:] == [7, 7] and y1.tolist()[-2:] == [7, 7] and yl.tolist()[-2:] == [0.0, 0.5]


def test_bgr_entry_is_the_rgb_one_reversed():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    assert np.array_equal(M.get_img_bgr(rgb[..., ::-1], 5, 6), M.get_img(rgb, 5, 6))
