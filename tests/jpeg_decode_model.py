"""Helper of the MJPEG decoder tests (not a test): libjpeg-turbo's default decoder (JDCT_ISLOW, fancy upsampling; what Pillow runs)
written down in NumPy, independent of the HIP code.  Entropy decoding is tests/jpeg_model.py's; from the coefficients on:
dequantisation, jidctint's 13-bit integer IDCT in int32, + 128 and a plain clamp (libjpeg's range table wraps for values no real
encoder produces; the clamp is the project's contract), h2v2_fancy_upsample with the neighbours clamped at the true chroma size,
jdcolor's 16-bit fixed point.  Colour comes back as BGR, as the project keeps it."""
import os

import numpy as np

import jpeg_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mjpeg_decode_streams.npz")
NAT_OF_ZZ = M.ZIGZAG                       # coefficient k of the scan sits at natural position ZIGZAG[k]


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def annexk_dht():
    body = b""
    for tc_th, (bits, vals) in ((0x00, M.DC_LUMA), (0x10, M.AC_LUMA), (0x01, M.DC_CHROMA), (0x11, M.AC_CHROMA)):
        body += bytes([tc_th]) + bytes(bits) + bytes(vals)
    return _segment(0xC4, body)


def segments(data):
    """[(marker, offset of the FF, total length)] up to and including SOS."""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        ln = (data[p + 2] << 8) | data[p + 3]
        out.append((data[p + 1], p, 2 + ln))
        p += 2 + ln
        if out[-1][0] == 0xDA:
            return out


def strip_dht(data):
    """The same stream without its DHT segments (only meaningful when they are the Annex K tables)."""
    data = bytes(data)
    keep, p = data[:2], 2
    for mk, off, ln in segments(data):
        if mk != 0xC4:
            keep += data[off:off + ln]
        p = off + ln
    return keep + data[p:]


def with_dht(data):
    """Streams without DHT are coded with the Annex K tables: put them in front of SOS."""
    data = bytes(data)
    segs = segments(data)
    if any(mk == 0xC4 for mk, _, _ in segs):
        return data
    sos = segs[-1][1]
    return data[:sos] + annexk_dht() + data[sos:]


def coefficients(data):
    """jpeg_model.decode with the coefficients in NATURAL order: info["coef"] int32 [nmcu, blocks of the MCU, 64], not dequantised."""
    info = M.decode(with_dht(data))
    nat = np.zeros(info["coef"].shape, np.int32)
    nat[..., NAT_OF_ZZ] = info["coef"]
    info["coef"] = nat
    return info


def _idct8(x, shift):
    """One pass of jidctint over the FIRST axis of int32 [8, ...]."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[k] for k in range(8))
    z1 = (i2 + i6) * 4433
    tmp2 = z1 - i6 * 15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    rnd = np.int32(1 << (shift - 1))
    out = [tmp10 + a3, tmp11 + a2, tmp12 + a1, tmp13 + a0, tmp13 - a0, tmp12 - a1, tmp11 - a2, tmp10 - a3]
    return np.stack([(o + rnd) >> shift for o in out]).astype(np.int32)


def idct(coef, q):
    """coef int [..., 64] natural order, q [64] natural order -> uint8 [..., 8, 8]."""
    d = (np.asarray(coef, np.int32) * np.asarray(q, np.int32)).reshape(coef.shape[:-1] + (8, 8))
    ws = _idct8(np.moveaxis(d, -2, 0), 11)                     # pass 1: columns (over the row index); ws [k, ..., c]
    ws = np.moveaxis(ws, 0, -2)                                # [..., k, c]
    out = _idct8(np.moveaxis(ws, -1, 0), 18)                   # pass 2: rows (over the column index); out [x, ..., r]
    out = np.moveaxis(out, 0, -1)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(info):
    """-> [Y, (Cb, Cr)]: uint8 planes at MCU-padded size."""
    H, W, C = info["H"], info["W"], info["C"]
    samp = info["sampling"]
    h0 = samp[0][0] if C == 3 else 1
    ms = 8 * h0
    mcux, mcuy = -(-W // ms), -(-H // ms)
    coef = info["coef"]
    qt = [info["qtables"][t] for t in info["tq"]]
    out = []
    if C == 1 or h0 == 1:
        for c in range(C):
            px = idct(coef[:, c], qt[c]).reshape(mcuy, mcux, 8, 8)
            out.append(px.transpose(0, 2, 1, 3).reshape(mcuy * 8, mcux * 8))
    else:
        y = idct(coef[:, :4], qt[0]).reshape(mcuy, mcux, 2, 2, 8, 8)          # [my, mx, by, bx, r, c]
        out.append(y.transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * 16, mcux * 16))
        for c in (1, 2):
            px = idct(coef[:, 3 + c], qt[c]).reshape(mcuy, mcux, 8, 8)
            out.append(px.transpose(0, 2, 1, 3).reshape(mcuy * 8, mcux * 8))
    return out


def upsample_h2v2(plane, H, W):
    """jdsample.c h2v2_fancy_upsample on the true chroma size ceil(H/2) x ceil(W/2) -> int32 [H, W]."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    c = plane[:ch, :cw].astype(np.int32)
    out = np.zeros((2 * ch, 2 * cw), np.int32)
    rows = np.arange(ch)
    cols = np.arange(cw)
    for v in (0, 1):
        nb = np.clip(rows - 1 if v == 0 else rows + 1, 0, ch - 1)
        s = 3 * c + c[nb]
        out[v::2, 0::2] = (3 * s + s[:, np.maximum(cols - 1, 0)] + 8) >> 4
        out[v::2, 1::2] = (3 * s + s[:, np.minimum(cols + 1, cw - 1)] + 7) >> 4
    return out[:H, :W]


def colour(y, cb, cr):
    """jdcolor.c ycc_rgb_convert -> uint8 [H, W, 3] in B, G, R order."""
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data):
    """The whole decoder: uint8 [H, W] (grey) or [H, W, 3] BGR."""
    info = coefficients(data)
    H, W = info["H"], info["W"]
    p = planes(info)
    if info["C"] == 1:
        return p[0][:H, :W].copy()
    if info["sampling"][0] == (2, 2):
        cb, cr = upsample_h2v2(p[1], H, W), upsample_h2v2(p[2], H, W)
    else:
        cb, cr = p[1][:H, :W], p[2][:H, :W]
    return colour(p[0][:H, :W], cb, cr)


def pillow_bgr(data):
    """Pillow's decode of the stream, in the project's layout."""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    if im.mode == "L":
        return np.asarray(im).copy()
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def have_turbo():
    try:
        from PIL import features
        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:
        return False


def load_golden():
    """{name: (jpeg bytes, golden pixels)} in the file's order."""
    z = np.load(GOLDEN)
    names = [str(n) for n in z["names"]]
    return {n: (z["jpeg_" + n].tobytes(), z["pixels_" + n]) for n in names}
