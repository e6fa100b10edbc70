"""Helper of the planar MJPEG tests (not a test): the YCbCr route written down in NumPy on top of jpeg_decode_model and jpeg_model,
independent of the HIP code.

  decode_i420()       the decoder's planes() cropped to the dense frame Y [H,W] | U [H/2,W/2] | V [H/2,W/2] (grey: Y alone), uint8
                      [frame_bytes]: what stabnet_mjpeg_decode_i420 writes
  transform_planes()  the planar encoder's arithmetic: edge-pad every plane to whole MCUs, - 128, D @ blk @ D.T / Q, zig-zag, the
                      encoder's clamps; (coef, ratio) as jpeg_model.transform returns them
  encode_i420()       a whole stream: jpeg_model.header + jpeg_model.entropy_encode of those coefficients + EOI
"""
import os

import numpy as np

import jpeg_decode_model as D
import jpeg_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mjpeg_planar_streams.npz")


def frame_bytes(H, W, C):
    return H * W * 3 // 2 if C == 3 else H * W


def split(frame, H, W, C):
    """uint8 [frame_bytes] -> (Y [H,W], Cb [H/2,W/2] | None, Cr | None)"""
    frame = np.asarray(frame).reshape(-1)
    assert frame.size == frame_bytes(H, W, C)
    y = frame[:H * W].reshape(H, W)
    if C == 1:
        return y, None, None
    q = (H // 2) * (W // 2)
    return y, frame[H * W:H * W + q].reshape(H // 2, W // 2), frame[H * W + q:].reshape(H // 2, W // 2)


def join(y, cb=None, cr=None):
    parts = [np.asarray(y, np.uint8).reshape(-1)]
    if cb is not None:
        parts += [np.asarray(cb, np.uint8).reshape(-1), np.asarray(cr, np.uint8).reshape(-1)]
    return np.concatenate(parts)


def decode_planes(jpeg):
    """(info, Y [H,W], Cb, Cr at the true chroma size ceil(H/2) x ceil(W/2); None, None for grey)"""
    info = D.coefficients(jpeg)
    H, W = info["H"], info["W"]
    p = D.planes(info)
    if info["C"] == 1:
        return info, p[0][:H, :W].copy(), None, None
    assert info["sampling"][0] == (2, 2), "planar frames are 4:2:0 or grey"
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return info, p[0][:H, :W].copy(), p[1][:ch, :cw].copy(), p[2][:ch, :cw].copy()


def decode_i420(jpeg):
    """The dense planar frame of a grey or an even-sided 4:2:0 stream: uint8 [frame_bytes]."""
    info, y, cb, cr = decode_planes(jpeg)
    assert info["C"] == 1 or (info["H"] % 2 == 0 and info["W"] % 2 == 0), "a dense I420 frame needs even sides"
    return join(y, cb, cr)


def transform_planes(y, cb=None, cr=None, q_luma=None, q_chroma=None, dtype=np.float64):
    """y uint8 [H,W]; cb, cr uint8 [H/2,W/2] or None (grey).  Returns (coef int [nmcu, bpm, 64] zig-zag, ratio [nmcu, bpm, 64])."""
    y = np.asarray(y)
    H, W = y.shape
    C = 1 if cb is None else 3
    ms, bpm, mcux, mcuy, comps = M.geometry(H, W, C, "420")
    if C == 3:
        assert H % 2 == 0 and W % 2 == 0 and np.asarray(cb).shape == (H // 2, W // 2) == np.asarray(cr).shape
    pad = lambda p, s: np.pad(np.asarray(p), ((0, mcuy * s - p.shape[0]), (0, mcux * s - p.shape[1])), mode="edge").astype(dtype) - dtype(128.0)
    planes = [pad(y, ms)] + ([pad(np.asarray(cb), 8), pad(np.asarray(cr), 8)] if C == 3 else [])
    Dm = M.dct_matrix().astype(dtype)
    ratio = np.zeros((mcuy, mcux, bpm, 64), dtype)
    qn = [np.asarray(q_luma, dtype).reshape(8, 8)] + [np.asarray(q_chroma if q_chroma is not None else q_luma, dtype).reshape(8, 8)] * 2
    for c, plane in enumerate(planes):
        blk = M._blocks(plane)
        co = (Dm @ blk @ Dm.T) / qn[c]
        co = co.reshape(co.shape[0], co.shape[1], 64)[..., M.ZIGZAG]
        if C == 3 and c == 0:
            for j in range(4):
                ratio[:, :, j] = co[(j >> 1)::2, (j & 1)::2]
        else:
            ratio[:, :, comps.index(c)] = co
    ratio = ratio.reshape(mcuy * mcux, bpm, 64)
    coef = np.rint(ratio).astype(np.int64)
    coef[..., 1:] = np.clip(coef[..., 1:], -1023, 1023)
    coef[..., 0] = np.clip(coef[..., 0], -1024, 1024)
    return coef, ratio


def encode_i420(frame, H, W, C, quality=75, restart_mcus=1, q_luma=None, q_chroma=None):
    """A complete JFIF stream (4:2:0, or grey for C = 1) of a dense planar frame."""
    if q_luma is None:
        q_luma, q_chroma = M.quant_tables(quality)
    y, cb, cr = split(frame, H, W, C)
    coef, _ = transform_planes(y, cb, cr, q_luma, q_chroma)
    return M.header(H, W, C, "420", restart_mcus, q_luma, q_chroma) + M.entropy_encode(coef, C, "420", restart_mcus) + b"\xff\xd9"


def pillow_draft_planes(jpeg):
    """Pillow's own decode left in YCbCr (im.draft): libjpeg-turbo's Y exactly and its fancy-upsampled Cb, Cr; uint8 [H,W,3]
    ([H,W] for grey)."""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(jpeg)))
    if im.mode == "L":
        return np.asarray(im).copy()
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    return np.asarray(im).copy()


def load_golden():
    """{name: (jpeg bytes, Pillow's draft planes)} in the file's order."""
    z = np.load(GOLDEN)
    names = [str(n) for n in z["names"]]
    return {n: (z["jpeg_" + n].tobytes(), z["ycc_" + n]) for n in names}


# ---- encoder inputs and cases shared by the CPU and the GPU tests ----------------------------------------------------------------------
def make_planes(kind, H, W, C, batch=1, seed=0):
    """uint8 [batch, frame_bytes].  texture: smooth planes + sinusoid + step + mild noise; noise120: mid-grey + sigma 120 noise, clipped;
    checker1 / checker8: 0 / 255 checkerboards of 1 / 8 samples on every plane."""
    rng = np.random.default_rng(2200 + seed)
    out = np.zeros((batch, frame_bytes(H, W, C)), np.uint8)
    shapes = [(H, W)] + ([(H // 2, W // 2)] * 2 if C == 3 else [])
    for b in range(batch):
        planes = []
        for c, (h, w) in enumerate(shapes):
            yy, xx = np.mgrid[0:h, 0:w]
            if kind == "texture":
                f = 110 + 20 * c + 60 * np.sin(xx / (7.0 + 3 * c) + b) * np.cos(yy / (11.0 - 2 * c)) + 30 * np.sin(2 * np.pi * (xx + 2 * yy) / (5.0 + c)) \
                    + 50.0 * ((xx > w // 2 + c) ^ (yy > h // 3)) + rng.normal(0, 6, (h, w))
            elif kind == "noise120":
                f = 128 + rng.normal(0, 120, (h, w))
            elif kind in ("checker1", "checker8"):
                s = 1 if kind == "checker1" else 8
                f = 255.0 * (((xx // s) + (yy // s)) & 1)
            else:
                raise ValueError(kind)
            planes.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        out[b] = join(*planes)
    return out


# (kind, H, W, planes, quality, restart, batch)
ENCODE_CASES = [
    ("texture", 16, 16, 3, 75, 1, 1),
    ("texture", 18, 34, 3, 75, "row", 3),
    ("texture", 2, 2, 3, 100, "all", 1),
    ("texture", 46, 78, 3, 30, 3, 2),
    ("noise120", 64, 96, 3, 100, 1, 1),
    ("texture", 9, 13, 1, 75, 2, 1),
]


def case_id(c):
    return "%s-%dx%d-p%d-q%d-r%s-n%d" % c
