"""NumPy statements of the frame-ingest arithmetic (csrc/ingest.hip): what the reference does to every frame before the network sees it.

  grey    cv2.cvtColor(BGR2GRAY) on uint8 [external: restated from the published algorithm, cv2 is not a dependency]:
          (b*WB + g*WG + r*WR + (1 << (S-1))) >> S, OpenCV 3: 1868, 9617, 4899, S = 14; OpenCV 4: 3735, 19235, 9798, S = 15
  resize  PIL.Image.resize((rw, rh), Image.BILINEAR) on the 8-bit image: Pillow's triangle filter with support max(scale, 1), horizontal
          pass first, rounded and clipped to 8 bits, then the vertical pass; 22-bit fixed-point coefficients.  The real Pillow pins
          this statement (tests/test_ingest_cpu.py), and the GPU tests compare against the real Pillow too.
  norm    float32(float64(u) * (1./255) - 0.5): config.cvt_img2train computes in float64, TensorFlow casts the feed to float32
  colour  cv2.resize(img, (W, H)), INTER_LINEAR, uint8 [external]: 11-bit coefficients, horizontal int32 sums, the vertical pass
          (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
"""
import numpy as np

GRAY_WEIGHTS = {"cv3": (1868, 9617, 4899, 14), "cv4": (3735, 19235, 9798, 15)}       # (WB, WG, WR, shift)
PRECISION_BITS = 22


def pil_taps(n_in, n_out):
    """(ksize, bounds int32 [n_out, 2] = (xmin, n), kk int32 [n_out, ksize]) of Pillow's BILINEAR for one axis."""
    scale = float(n_in) / float(n_out)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / filterscale
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        a = np.abs((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss)
        k = np.where(a < 1.0, 1.0 - a, 0.0)
        ww = 0.0
        for v in k:                                   # Pillow sums in index order
            ww += v
        if ww != 0.0:
            k = k / ww
        bounds[i] = (xmin, n)
        kk[i, :n] = (0.5 + k * (1 << PRECISION_BITS)).astype(np.int64)      # (int) truncates; every value is >= 0
    return ksize, bounds, kk


def cv_taps(n_src, n_dst):
    """(ofs int32 [n_dst, 2], coef int16 [n_dst, 2]) of cv2.resize INTER_LINEAR for one axis."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    ofs = np.zeros((n_dst, 2), np.int32)
    coef = np.zeros((n_dst, 2), np.int16)
    for d in range(n_dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= n_src - 1:
            s, f = n_src - 1, np.float32(0)
        ofs[d] = (s, min(s + 1, n_src - 1))
        coef[d] = (int(np.rint((np.float32(1) - f) * np.float32(2048))), int(np.rint(f * np.float32(2048))))
    return ofs, coef


def grey_u8(img, weights="cv3"):
    """uint8 [..., H, W, 3] BGR (or [..., H, W] / [..., H, W, 1]: returned as it is) -> uint8 [..., H, W]."""
    img = np.asarray(img)
    if img.ndim >= 3 and img.shape[-1] == 1:
        return img[..., 0]
    if img.ndim < 3 or img.shape[-1] != 3:
        return img
    wb, wg, wr, s = GRAY_WEIGHTS[weights] if isinstance(weights, str) else weights
    v = img.astype(np.int64)
    return ((v[..., 0] * wb + v[..., 1] * wg + v[..., 2] * wr + (1 << (s - 1))) >> s).astype(np.uint8)


def _pass(img, bounds, kk, axis, lo, cnt, round8=True):
    """One Pillow pass along `axis` of a 2-D uint8 image: outputs lo .. lo + cnt."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.zeros((cnt,) + src.shape[1:], np.int64)
    for j in range(cnt):
        xmin, n = bounds[lo + j]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[lo + j, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
        out[j] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def pil_resize(grey, rh, rw, dy=0, dx=0, H=None, W=None):
    """Image.fromarray(grey).resize((rw, rh), BILINEAR).crop((dx, dy, dx + W, dy + H)) of a 2-D uint8 image."""
    H, W = rh if H is None else H, rw if W is None else W
    sh, sw = grey.shape
    img = grey
    if rw != sw:
        _, b, k = pil_taps(sw, rw)
        img = _pass(img, b, k, 1, dx, W)
    else:
        img = img[:, dx:dx + W]
    if rh != sh:
        _, b, k = pil_taps(sh, rh)
        img = _pass(img, b, k, 0, dy, H)
    else:
        img = img[dy:dy + H]
    return np.ascontiguousarray(img)


def real_pil_resize(grey, rh, rw, dy=0, dx=0, H=None, W=None):
    """The same through the installed Pillow."""
    from PIL import Image
    H, W = rh if H is None else H, rw if W is None else W
    im = Image.fromarray(np.ascontiguousarray(grey)).resize((rw, rh), Image.BILINEAR)
    return np.asarray(im.crop((dx, dy, dx + W, dy + H)))


def lut256():
    return (np.arange(256, dtype=np.float64) * (1. / 255) - 0.5).astype(np.float32)


def train_from_u8(u8):
    """config.cvt_img2train's last step as TensorFlow receives it."""
    return (u8.astype(np.float64) * (1. / 255) - 0.5).astype(np.float32)


def cv_resize(img, H, W):
    """uint8 [sh, sw, C] (or [sh, sw]) -> [H, W, C]."""
    img = np.asarray(img)
    sh, sw = img.shape[:2]
    if (sh, sw) == (H, W):
        return img.copy()
    xo, xc = cv_taps(sw, W)
    yo, yc = cv_taps(sh, H)
    v = img.astype(np.int32)
    a = xc.astype(np.int32).reshape((1, W, 2) + (1,) * (img.ndim - 2))
    S = v[:, xo[:, 0]] * a[:, :, 0] + v[:, xo[:, 1]] * a[:, :, 1]            # [sh, W, ...] int32
    b = yc.astype(np.int32).reshape((H, 2, 1) + (1,) * (img.ndim - 2))
    out = (((b[:, 0] * (S[yo[:, 0]] >> 4)) >> 16) + ((b[:, 1] * (S[yo[:, 1]] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def bilinear_f64(img, H, W):
    """float64 half-pixel bilinear with edge clamping (torch.nn.functional.interpolate, align_corners=False), NumPy."""
    v = np.asarray(img, np.float64)
    sh, sw = v.shape[:2]

    def axis(n_src, n_dst):
        f = np.maximum((np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5, 0.0)
        i0 = np.minimum(np.floor(f).astype(int), n_src - 1)
        return i0, np.minimum(i0 + 1, n_src - 1), f - i0
    y0, y1, wy = axis(sh, H)
    x0, x1, wx = axis(sw, W)
    wy = wy.reshape((H, 1) + (1,) * (v.ndim - 2)); wx = wx.reshape((1, W) + (1,) * (v.ndim - 2))
    top = v[y0][:, x0] * (1 - wx) + v[y0][:, x1] * wx
    bot = v[y1][:, x0] * (1 - wx) + v[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def geometry(H, W, crop_rate=1):
    """(rh, rw, dy, dx) of config.cvt_img2train (config.py:8-17)."""
    if crop_rate == 1:
        return H, W, 0, 0
    rh, rw = int(H / crop_rate), int(W / crop_rate)
    return rh, rw, int((rh - H) / 2), int((rw - W) / 2)


# (sh, sw, C, rh, rw, dy, dx, H, W, N): the window [dy, dy+H) x [dx, dx+W) of the (rh, rw) resize of N frames
GPU_CASES = [
    (45, 77, 3, 32, 48, 0, 0, 32, 48, 1),          # non-integer downscale, odd row bytes, unaligned rows
    (180, 320, 3, 72, 128, 0, 0, 72, 128, 1),      # the 2.5x of 720p -> 288x512: 7 taps
    (37, 53, 3, 64, 96, 0, 0, 64, 96, 1),          # upscale
    (64, 96, 3, 64, 96, 0, 0, 64, 96, 1),          # both passes skipped
    (100, 96, 1, 64, 96, 0, 0, 64, 96, 1),         # vertical only, grey input
    (64, 130, 3, 64, 96, 0, 0, 64, 96, 1),         # horizontal only
    (9, 7, 3, 64, 96, 0, 0, 64, 96, 1),            # every tap clamped
    (512, 96, 3, 32, 96, 0, 0, 32, 96, 1),         # 16x: 33 taps
    (64, 96, 3, 32, 48, 0, 0, 32, 48, 1),          # exact 2x
    (80, 120, 3, 71, 106, 3, 5, 64, 96, 1),        # crop_rate = 0.9
    (45, 77, 3, 32, 48, 0, 0, 32, 48, 2),          # batch
]
assert geometry(64, 96, 0.9) == (71, 106, 3, 5)

# source -> network sizes of the CPU comparison with the real Pillow (the GPU list, plus the full-size ones of the reference's use)
CPU_SHAPES = [(720, 1280, 288, 512), (1080, 1920, 720, 1280), (45, 77, 32, 48), (37, 53, 64, 96), (64, 96, 64, 96), (100, 96, 64, 96),
              (64, 130, 64, 96), (31, 200, 64, 96), (9, 7, 64, 96), (180, 320, 72, 128), (512, 96, 32, 96), (64, 96, 32, 48)]

INPUT_KINDS = ("random", "white", "black", "hramp", "vramp")


def case_id(case):
    sh, sw, C, rh, rw, dy, dx, H, W, N = case
    s = "%dx%dx%d-%dx%d" % (sh, sw, C, H, W)
    if (rh, rw) != (H, W):
        s += "-of%dx%d@%d,%d" % (rh, rw, dy, dx)
    return s + ("-n%d" % N if N > 1 else "")


def make_input(kind, sh, sw, C, N=1, seed=0):
    """uint8 [N, sh, sw, C]."""
    if kind == "random":
        return np.random.default_rng(seed + 7919 * sh + sw).integers(0, 256, (N, sh, sw, C), dtype=np.uint8)
    if kind == "white":
        return np.full((N, sh, sw, C), 255, np.uint8)
    if kind == "black":
        return np.zeros((N, sh, sw, C), np.uint8)
    ramp = (np.arange(sw) * 255 // max(sw - 1, 1))[None, :] if kind == "hramp" else (np.arange(sh) * 255 // max(sh - 1, 1))[:, None]
    img = np.broadcast_to(ramp, (sh, sw)).astype(np.uint8)
    out = np.stack([np.roll(img, 3 * c + n, axis=1 if kind == "hramp" else 0) for n in range(N) for c in range(C)], 0)
    return np.ascontiguousarray(out.reshape(N, C, sh, sw).transpose(0, 2, 3, 1))
